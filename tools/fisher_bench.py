#!/usr/bin/env python3
"""Fisher-information timings: device time (HIP events, median of --iters calls after warm-up) of
voxe_fisher_rays in its three uses -- accumulate (fisher), gather (ray_var with a voxel_var), both outputs in one call -- on the
bench's 160^3 random grid with S = 256, SH degree 0 and 2:
  (1) one 400 x 400 camera, image order;
  (2) a 32 768-ray random batch over 8 cameras, linear order: the trainer's shape.
Next to it, timed alternately in the same loop on the same GPU:
  (a) the SH-0 voxe_render_fwd + voxe_render_bwd of the same rays on a reused packed grid;
  (b) voxe_distortion_fwd_bwd with its gradient on the same rays: the same atomics-bound class of kernel;
  (c) a float32 torch evaluation of the exact quantity on a slice of --ref_rays rays, scaled to the launch's ray count: the
      per-sample coefficients (tests/fisher_ref.sample_terms on the forward's probed samples), the (ray, voxel) keys sorted, the
      deposits summed per key, squared, and index_add_-ed into the grid.
Exits 1 when a kernel call loses to (c).  One JSON line per case, also written to --out.

    python tools/fisher_bench.py [--iters 20] [--ref_rays 2048] [--out profiles/fisher_bench.txt]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "vox-e_amd"), os.path.join(ROOT, "tests"), ROOT]

import fisher_ref as FR  # noqa: E402
from thre3d_atom.utils.imaging_utils import pose_spherical  # noqa: E402
from voxe_hip import abi, ops, workload  # noqa: E402

DEV = torch.device("cuda:0")
RNG = (42, 7)


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _alternating_medians(fns, iters):
    """median ms of each callable, the callables taking turns inside one loop (3 warm-up rounds)"""
    times = [[] for _ in fns]
    for i in range(iters + 3):
        for k, fn in enumerate(fns):
            t = _timed(fn)
            if i >= 3:
                times[k].append(t)
    return [sorted(t)[len(t) // 2] for t in times]


def _rays(hw, cams):
    rays = [ops.cast_rays(hw, hw, workload.focal_for(hw), *pose_spherical(*workload.synth_pose_angles(cam, 100), workload.RADIUS), DEV)
            for cam in cams]
    return torch.cat([r[0] for r in rays]).contiguous(), torch.cat([r[1] for r in rays]).contiguous()


def torch_fisher(samples, dens, feat, ro, rd, spec, params, chunk=512, counts=None):
    """H [V] float32 of the exact quantity in torch: per chunk of rays the per-sample deposits keyed by (ray, voxel), keys sorted,
    deposits summed per key, squared, added to the grid.  `counts` (a dict) receives the number of non-zero (ray, voxel) sums --
    the emits of the kernel -- and of samples inside the box"""
    V = dens.numel()
    Hg = torch.zeros(V, dtype=torch.float32, device=dens.device)
    for lo in range(0, ro.shape[0], chunk):
        sl = slice(lo, lo + chunk)
        a, flat, cf = FR.sample_terms(tuple(s[sl] for s in samples), dens, feat, ro[sl], rd[sl], spec, params, dtype=torch.float32)
        n = flat.shape[0]
        key = (torch.arange(n, device=flat.device)[:, None, None] * V + flat).reshape(-1)
        dep = (a[:, :, None, :] * cf[..., None]).reshape(-1, 3)
        uniq, inv = torch.unique(key, return_inverse=True)
        seg = torch.zeros((uniq.numel(), 3), dtype=torch.float32, device=dens.device).index_add_(0, inv, dep)
        sq = (seg * seg).sum(dim=1)
        Hg.index_add_(0, uniq % V, sq)
        if counts is not None:
            counts["emits"] = counts.get("emits", 0) + int((sq != 0).sum())
            counts["inside_samples"] = counts.get("inside_samples", 0) + int(samples[1][sl].bool().sum())
    return Hg


def case_times(spec, dens, feat0, feat, deg, ro, rd, S, width, iters, ref_rays):
    R = ro.shape[0]
    params = ops.RenderParams(num_samples=S, near=workload.NEAR, far=workload.FAR, perturb=True, white_bkgd=True, sh_degree=deg,
                              image_width=width)
    fisher = torch.zeros(dens.shape[:3], device=DEV)
    var = torch.rand(dens.shape[:3], generator=torch.Generator().manual_seed(5)).to(DEV) + 0.5

    def accumulate():
        ops.fisher_rays_(spec, params, dens, feat, ro, rd, fisher=fisher, rng=RNG)

    def gather():
        ops.fisher_rays_(spec, params, dens, feat, ro, rd, voxel_var=var, want_ray_var=True, rng=RNG)

    def both():
        ops.fisher_rays_(spec, params, dens, feat, ro, rd, fisher=fisher, voxel_var=var, want_ray_var=True, rng=RNG)

    # (a) the SH-0 render forward + backward of the same rays (kernels alone: packed grid reused)
    params0 = ops.RenderParams(**{**vars(params), "sh_degree": 0})
    g = torch.Generator().manual_seed(43)
    g_col = torch.randn((R, 3), generator=g).to(DEV)
    g_zero = torch.zeros((R, 1), device=DEV)
    outs = [torch.empty((R, n), dtype=torch.float32, device=DEV) for n in (3, 1, 1, 1)]
    r_dens, r_feat = torch.zeros_like(dens), torch.zeros_like(feat0)
    ws = ops.Workspace()

    def render():
        ops.render_fwd_into(spec, params0, dens, feat0, ro, rd, None, *outs, ws, RNG)
        ops.render_bwd_into(spec, params0, dens, feat0, ro, rd, None, outs[0], outs[1], outs[2], g_col, g_zero, g_zero, r_dens, r_feat,
                            ws, RNG)

    # (b) the distortion loss with its gradient
    d_dist = torch.zeros_like(dens)

    def distortion():
        ops.distortion_fwd_bwd(spec, params0, dens, ro, rd, None, RNG, want_loss=True, d_densities=d_dist)

    # (c) the torch evaluation on a slice of the rays
    n = min(ref_rays, R)
    pick = torch.linspace(0, R - 1, n, device=DEV).round().long()
    sub = ops.RenderParams(**{**vars(params), "image_width": 0})
    probe = ops.sample_probe(spec, params, dens, feat, ro, rd, None, rng=RNG, outputs=("z", "inside", "idx"))
    samples = tuple(probe[k][pick].contiguous() for k in ("z", "inside", "idx"))
    so, sd = ro[pick].contiguous(), rd[pick].contiguous()
    del probe

    def restatement():
        return torch_fisher(samples, dens, feat, so, sd, spec, sub)

    t_acc, t_gat, t_both, t_render, t_dist, t_ref = _alternating_medians([accumulate, gather, both, render, distortion, restatement],
                                                                          iters)
    # the timed kernel computes what the torch evaluation computes (the picked rays in a launch of their own: a ray's samples
    # depend on its index in the launch through the jitter stream, so the slice is compared without jitter)
    plain = ops.RenderParams(**{**vars(sub), "perturb": False})
    pr = ops.sample_probe(spec, plain, dens, feat, so, sd, None, rng=(0, 0), outputs=("z", "inside", "idx"))
    counts = {}
    want = torch_fisher(tuple(pr[k] for k in ("z", "inside", "idx")), dens, feat, so, sd, spec, plain, counts=counts)
    got = torch.zeros(dens.shape[:3], device=DEV)
    ops.fisher_rays_(spec, plain, dens, feat, so, sd, fisher=got)
    err = float((got.reshape(-1).double() - want.double()).norm() / want.double().norm())
    t_ref_scaled = t_ref * R / n
    return {"rays": R, "sh_degree": deg, "accumulate_ms": round(t_acc, 4), "gather_ms": round(t_gat, 4), "both_ms": round(t_both, 4),
            "sh0_render_fwd_bwd_ms": round(t_render, 4), "distortion_fwd_bwd_ms": round(t_dist, 4),
            "torch_f32_ms": round(t_ref, 3), "torch_rays": n, "torch_f32_scaled_ms": round(t_ref_scaled, 2),
            "accumulate_over_sh0_render": round(t_acc / t_render, 3), "accumulate_over_distortion": round(t_acc / t_dist, 3),
            "torch_over_accumulate": round(t_ref_scaled / t_acc, 1), "rel_l2_vs_torch_f32": float(f"{err:.3e}"),
            "emits_per_inside_sample": round(counts["emits"] / max(counts["inside_samples"], 1), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--ref_rays", type=int, default=2048)
    ap.add_argument("--side", type=int, default=160)
    ap.add_argument("--image", type=int, default=400)
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fisher_bench.txt"))
    a = ap.parse_args()
    spec = ops.GridSpec(aabb=((-1.5, 1.5),) * 3, density_scale=100.0 / 3.0, density_pre_act=abi.ACT_IDENTITY,
                        density_post_act=abi.ACT_SOFTPLUS)
    d, f0 = workload.random_grid(a.side)
    dens, feat0 = d.to(DEV).contiguous(), f0.to(DEV).contiguous()
    _, f2 = workload.random_grid(a.side, nfeat=27, seed=44)
    feats = {0: feat0, 2: f2.to(DEV).contiguous()}
    lines, slower = [], False
    ro_i, rd_i = _rays(a.image, [3])
    ro_b, rd_b = _rays(a.image, [3 + 12 * j for j in range(8)])
    pick = torch.randperm(ro_b.shape[0], generator=torch.Generator().manual_seed(11))[:32768].to(DEV)
    ro_b, rd_b = ro_b[pick].contiguous(), rd_b[pick].contiguous()
    for deg in (0, 2):
        for name, ro, rd, width in ((f"random{a.side}_{a.image}x{a.image}_S{a.samples}_image", ro_i, rd_i, a.image),
                                    (f"random{a.side}_batch{ro_b.shape[0]}_of_8cams_S{a.samples}_linear", ro_b, rd_b, 0)):
            lines.append({"case": f"{name}_sh{deg}", **case_times(spec, dens, feat0, feats[deg], deg, ro, rd, a.samples, width, a.iters,
                                                                   a.ref_rays)})
            print(json.dumps(lines[-1]), flush=True)
            line = lines[-1]
            slower = slower or max(line["accumulate_ms"], line["gather_ms"], line["both_ms"]) > line["torch_f32_scaled_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")
    sys.exit(1 if slower else 0)


if __name__ == "__main__":
    main()
