#!/usr/bin/env python3
"""Vector-quantisation timings: device time (HIP events, median of --iters calls after warm-up, the
callables taking turns inside one loop) of
  vq_assign_        voxe_vq_assign with dist: the float32 MFMA kernel, arg-min folded in
  vq_accumulate_    voxe_vq_accumulate in both variants (one atomic per lane / runs of equal index merged in the wave), on the
                    points as they come and on points sorted by index (the sort itself is timed separately)
  lloyd             one full Lloyd iteration as train_codebook runs it: assign, sort by index and gather, zero the sums,
                    accumulate (shipped variant), the float64 division
next to a float32 torch restatement on the same GPU: chunked x @ C.T + argmin for the assignment, index_add_ for the sums.
Sizes: N = 2^20 and 2^21 uniform points, K = 4096, F = 3 / 12 / 27 / 48; with --grid also the real VQ set of the bench's 160^3
SH-2 grid (importance over --views cameras, VQRF's default shares), for which it also reports what compress_voxel_grid.py
would: label shares, bytes before and after, the distortion curve, the k-means time and the PSNR of the decompressed model's
renders.  The achieved FLOP/s of the assign kernel (2 N K F per call) is printed next to the programming guide's 122 TF for an
untuned float32 MFMA GEMM.  Exits 1 when the assign call, the shipped accumulate call on sorted points or the Lloyd
iteration loses to torch.  One JSON line per case, also written to --out.

    python tools/vq_bench.py [--iters 10] [--grid] [--out profiles/vq_bench.txt]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "vox-e_amd"), ROOT]

from thre3d_atom.thre3d_reprs import compression as CP  # noqa: E402
from voxe_hip import ops, workload  # noqa: E402

DEV = torch.device("cuda:0")
GUIDE_GEMM_TF = 122.0


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _alternating_medians(fns, iters):
    times = [[] for _ in fns]
    for i in range(iters + 2):
        for k, fn in enumerate(fns):
            t = _timed(fn)
            if i >= 2:
                times[k].append(t)
    return [sorted(t)[len(t) // 2] for t in times]


def torch_assign(x, c, chunk=1 << 16):
    """float32 restatement: chunked x @ C.T + argmin (the N x K scores of a chunk are materialised)"""
    cn = (c * c).sum(1)
    out = torch.empty(x.shape[0], dtype=torch.int64, device=x.device)
    for lo in range(0, x.shape[0], chunk):
        out[lo:lo + chunk] = torch.argmin(cn[None, :] - 2.0 * (x[lo:lo + chunk] @ c.T), dim=1)
    return out


def torch_accumulate(x, w, index, K):
    sum_wx = torch.zeros((K, x.shape[1]), dtype=torch.float32, device=x.device).index_add_(0, index, w[:, None] * x)
    sum_w = torch.zeros((K,), dtype=torch.float32, device=x.device).index_add_(0, index, w)
    return sum_wx, sum_w


def case_times(name, x, w, K, iters, seed=0):
    N, F = x.shape
    rows = torch.randperm(N, generator=torch.Generator().manual_seed(seed))[:K].to(DEV)
    c = x[rows].contiguous()
    index = torch.empty(N, dtype=torch.int32, device=DEV)
    dist = torch.empty(N, dtype=torch.float32, device=DEV)
    ops.vq_assign_(x, c, index, dist)
    order = torch.argsort(index.long(), stable=True)
    xs, ws, idx_s = x[order].contiguous(), w[order].contiguous(), index[order].contiguous()
    index64 = index.long()
    sum_wx = torch.zeros((K, F), dtype=torch.int64, device=DEV)
    sum_w = torch.zeros((K,), dtype=torch.int64, device=DEV)

    def assign():
        ops.vq_assign_(x, c, index, dist)

    def accumulate(mode, sorted_points):
        def run():
            ops.vq_debug_merge(mode)
            if sorted_points:
                ops.vq_accumulate_(xs, ws, idx_s, sum_wx, sum_w, check_index=False)
            else:
                ops.vq_accumulate_(x, w, index, sum_wx, sum_w, check_index=False)
            ops.vq_debug_merge(ops.VQ_MERGE_SHIPPED)
        return run

    def sort_points():
        by_code, o = torch.sort(index)
        return x[o], w[o], by_code

    def lloyd():
        ops.vq_assign_(x, c, index, dist)
        sum_wx.zero_()
        sum_w.zero_()
        by_code, o = torch.sort(index)
        ops.vq_accumulate_(x[o], w[o], by_code, sum_wx, sum_w, check_index=False)
        return CP.lloyd_update(c, sum_wx, sum_w)

    def t_assign():
        return torch_assign(x, c)

    def t_accumulate():
        return torch_accumulate(x, w, index64, K)

    def t_lloyd():
        i = torch_assign(x, c)
        swx, sw = torch_accumulate(x, w, i, K)
        return torch.where((sw > 0)[:, None], swx / sw.clamp(min=1e-30)[:, None], c)

    fns = [assign, accumulate(ops.VQ_MERGE_PER_LANE, False), accumulate(ops.VQ_MERGE_RUNS, False),
           accumulate(ops.VQ_MERGE_PER_LANE, True), accumulate(ops.VQ_MERGE_RUNS, True), sort_points, lloyd,
           t_assign, t_accumulate, t_lloyd, accumulate(ops.VQ_MERGE_SHIPPED, True)]
    t = _alternating_medians(fns, iters)
    agree = float((torch_assign(x, c) == index64).float().mean())
    tf = 2.0 * N * K * F / (t[0] * 1e-3) / 1e12
    shipped = t[10]      # what a Lloyd iteration calls: the shipped variant on points sorted by index
    return {"case": name, "N": N, "K": K, "F": F, "assign_ms": round(t[0], 4), "assign_tflops": round(tf, 2),
            "guide_f32_mfma_gemm_tflops": GUIDE_GEMM_TF, "accumulate_per_lane_ms": round(t[1], 4),
            "accumulate_runs_ms": round(t[2], 4), "accumulate_per_lane_sorted_ms": round(t[3], 4),
            "accumulate_runs_sorted_ms": round(t[4], 4), "accumulate_shipped_sorted_ms": round(shipped, 4), "sort_and_gather_ms": round(t[5], 4), "lloyd_ms": round(t[6], 4),
            "torch_assign_ms": round(t[7], 4), "torch_index_add_ms": round(t[8], 4), "torch_lloyd_ms": round(t[9], 4),
            "torch_over_assign": round(t[7] / t[0], 2), "torch_over_accumulate_shipped": round(t[8] / shipped, 2),
            "torch_over_lloyd": round(t[9] / t[6], 2), "index_agreement_with_torch": round(agree, 6),
            "loses": bool(t[0] > t[7] or shipped > t[8] or t[6] > t[9])}


def bench_grid(side, views, image, iterations, iters):
    """the bench's 160^3 SH-2 random grid through the whole compression; returns (report line, the VQ set)"""
    from thre3d_atom.modules.volumetric_model import VolumetricModel
    from thre3d_atom.thre3d_reprs.renderers import SHVoxGridRenderConfig, render_sh_voxel_grid
    from thre3d_atom.thre3d_reprs.voxels import VoxelGrid, VoxelSize
    from thre3d_atom.utils.imaging_utils import CameraBounds, CameraIntrinsics, get_thre360_animation_poses

    dens, _ = workload.random_grid(side)
    _, feat = workload.random_grid(side, nfeat=27, seed=44)
    grid = VoxelGrid(dens.to(DEV), feat.to(DEV), VoxelSize(*(3.0 / side,) * 3), density_preactivation=torch.nn.Identity(),
                     density_postactivation=torch.nn.Softplus(), expected_density_scale=100.0 / 3.0, tunable=True)
    model = VolumetricModel(grid, render_sh_voxel_grid, SHVoxGridRenderConfig(256, CameraBounds(workload.NEAR, workload.FAR)),
                            device=DEV)
    intr = CameraIntrinsics(image, image, workload.focal_for(image))
    poses = get_thre360_animation_poses(workload.RADIUS, 60.0, views)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    ev[0].record()
    importance = CP.voxel_importance(model, poses, intr)
    ev[1].record()
    comp = CP.compress(model, importance, iterations=iterations)
    ev[2].record()
    torch.cuda.synchronize()
    labels = torch.from_numpy(comp.labels().reshape(-1))
    n = labels.numel()
    data = model.get_save_info({})
    before = CP.checkpoint_bytes(data)
    after = CP.checkpoint_bytes(CP.compress_checkpoint_(data, comp))
    vq = (labels == CP.LABEL_VQ).to(DEV)
    x = grid.features.detach().reshape(n, -1)[vq].contiguous()
    w = (importance.reshape(-1)[vq].to(torch.float64) / float(1 << 32)).to(torch.float32)
    # k-means alone (the partition and the container are host work around it)
    km = _alternating_medians([lambda: CP.train_codebook(x, w, CP.DEFAULT_CODEBOOK_SIZE, iterations)], max(1, iters // 5))[0]
    d, f = CP.decompress(comp)
    small = VolumetricModel(VoxelGrid(d.to(DEV), f.to(DEV), VoxelSize(*(3.0 / side,) * 3), density_preactivation=torch.nn.Identity(),
                                      density_postactivation=torch.nn.Softplus(), expected_density_scale=100.0 / 3.0, tunable=True),
                            render_sh_voxel_grid, model.render_config, device=DEV)
    psnr = []
    for pose in poses[:: max(1, views // 6)]:
        a = model.render(pose, intr, perturb_sampled_points=False).colour.double()
        b = small.render(pose, intr, perturb_sampled_points=False).colour.double()
        psnr.append(float(-10.0 * torch.log10(((a - b) ** 2).mean().clamp(min=1e-30))))
    line = {"case": f"random{side}_sh2_compress_{views}views_{image}x{image}", "voxels": n,
            "share_pruned": round(float((labels == 0).float().mean()), 4), "share_vq": round(float((labels == 1).float().mean()), 4),
            "share_kept": round(float((labels == 2).float().mean()), 4), "bytes_before": before, "bytes_after": after,
            "ratio": round(before / after, 2), "container_bytes_before_deflate": comp.nbytes(),
            "importance_ms": round(ev[0].elapsed_time(ev[1]), 2), "compress_ms": round(ev[1].elapsed_time(ev[2]), 2),
            "kmeans_iterations": iterations, "kmeans_ms": round(km, 2), "distortion": [float(f"{v:.6e}") for v in comp.distortion],
            "psnr_db_mean": round(sum(psnr) / len(psnr), 2), "psnr_db_min": round(min(psnr), 2), "psnr_views": len(psnr)}
    return line, (x / x.abs().max(), w / w.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--grid", action="store_true", help="also the bench's 160^3 SH-2 grid through the whole compression")
    ap.add_argument("--side", type=int, default=160)
    ap.add_argument("--views", type=int, default=36)
    ap.add_argument("--image", type=int, default=400)
    ap.add_argument("--kmeans_iterations", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="*", default=[20, 21], help="log2 of the synthetic N")
    ap.add_argument("--channels", type=int, nargs="*", default=[3, 12, 27, 48])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vq_bench.txt"))
    a = ap.parse_args()
    lines = []

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)

    g = torch.Generator().manual_seed(1)
    for log_n in a.sizes:
        for F in a.channels:
            x = (torch.rand((1 << log_n, F), generator=g) * 2 - 1).to(DEV)
            w = torch.rand((1 << log_n,), generator=g).to(DEV)
            emit(case_times(f"uniform_N2^{log_n}_K4096_F{F}", x, w, 4096, a.iters))
            del x, w
    if a.grid:
        line, (x, w) = bench_grid(a.side, a.views, a.image, a.kmeans_iterations, a.iters)
        emit(line)
        emit(case_times(f"random{a.side}_sh2_vq_set_K4096_F27", x.contiguous(), w.contiguous(), 4096, a.iters))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")
    sys.exit(1 if any(line.get("loses") for line in lines) else 0)


if __name__ == "__main__":
    main()
