#!/usr/bin/env python3
"""Ray-gradient timings: device time (HIP events, median of --iters calls after warm-up) of
voxe_render_bwd_rays for every lanes-per-ray split, on the bench's 160^3 random grid with S = 256, SH degree 0 and 2:
  (a) one 400 x 400 camera, image order;
  (b) a 32 768-ray random batch over 8 cameras, linear order: the trainer's shape.
Next to it, timed alternately in the same loop on the same GPU:
  - the SH-0 voxe_render_fwd + voxe_render_bwd of the same rays on a reused packed grid (what the grid's gradient costs);
  - the float32 torch restatement's autograd to the rays (tests/ray_grad_ref.py on the forward's probed samples), on a slice of
    --ref_rays rays, scaled to the launch's ray count (the whole launch does not fit torch's [R,S,F] intermediates).
Exits non-zero when the kernel is the slower one of kernel and restatement.  One JSON line per case, also written to --out.

    python tools/ray_grad_bench.py [--iters 20] [--ref_rays 4096] [--out profiles/ray_grad_bench.txt]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "vox-e_amd"), os.path.join(ROOT, "tests")]

import ray_grad_ref as RR  # noqa: E402
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


def case_times(spec, dens, feat0, feat, deg, ro, rd, S, width, iters, ref_rays):
    R = ro.shape[0]
    params = ops.RenderParams(num_samples=S, near=workload.NEAR, far=workload.FAR, perturb=True, white_bkgd=True, sh_degree=deg,
                              image_width=width)
    g = torch.Generator().manual_seed(43)
    g_col = torch.randn((R, 3), generator=g).to(DEV)
    g_dep, g_acc = (torch.randn((R,), generator=g) * 0.25).to(DEV), (torch.randn((R,), generator=g) * 0.25).to(DEV)
    d_o, d_d = torch.empty((R, 3), device=DEV), torch.empty((R, 3), device=DEV)

    def kernel(lanes=0):
        ops.render_bwd_rays(spec, params, dens, feat, ro, rd, None, RNG, g_col, g_dep, g_acc, lanes=lanes, d_rays_o=d_o, d_rays_d=d_d)

    # the SH-0 render forward + backward of the same rays (kernels alone: packed grid reused)
    params0 = ops.RenderParams(**{**vars(params), "sh_degree": 0})
    outs = [torch.empty((R, n), dtype=torch.float32, device=DEV) for n in (3, 1, 1, 1)]
    r_dens, r_feat = torch.zeros_like(dens), torch.zeros_like(feat0)
    ws = ops.Workspace()

    def render():
        ops.render_fwd_into(spec, params0, dens, feat0, ro, rd, None, *outs, ws, RNG)
        ops.render_bwd_into(spec, params0, dens, feat0, ro, rd, None, outs[0], outs[1], outs[2], g_col, g_dep[:, None].contiguous(),
                            g_acc[:, None].contiguous(), r_dens, r_feat, ws, RNG)

    # the float32 restatement's autograd on a slice of the rays
    n = min(ref_rays, R)
    pick = torch.linspace(0, R - 1, n, device=DEV).round().long()
    sub = ops.RenderParams(**{**vars(params), "image_width": 0})
    probe = ops.sample_probe(spec, params, dens, feat, ro, rd, None, rng=RNG, outputs=("z", "inside", "idx"))
    samples = tuple(probe[k][pick].contiguous() for k in ("z", "inside", "idx"))
    so, sd = ro[pick].contiguous(), rd[pick].contiguous()
    del probe

    def restatement():
        return RR.ray_gradients(samples, dens, feat, so, sd, spec, sub, g_col[pick], g_dep[pick], g_acc[pick], dtype=torch.float32)

    t_kernel, t_render, t_ref = _alternating_medians([kernel, render, restatement], iters)
    by_lanes = {}
    for lanes in (1, 2, 4, 8):
        by_lanes[str(lanes)] = round(_alternating_medians([lambda: kernel(lanes)], iters)[0], 4)
    # the timed kernel computes what the restatement computes
    kernel()
    want = restatement()
    err = [float((a[pick].double() - b.double()).norm() / b.double().norm()) for a, b in zip((d_o, d_d), want)]
    t_ref_scaled = t_ref * R / n
    return {"rays": R, "sh_degree": deg, "lanes_chosen": _lanes_for(R),
            "render_bwd_rays_ms": round(t_kernel, 4), "ms_by_lanes": by_lanes, "sh0_render_fwd_bwd_ms": round(t_render, 4),
            "torch_f32_restatement_ms": round(t_ref, 4), "restatement_rays": n, "torch_f32_restatement_scaled_ms": round(t_ref_scaled, 3),
            "kernel_over_sh0_render": round(t_kernel / t_render, 3), "restatement_over_kernel": round(t_ref_scaled / t_kernel, 1),
            "rel_l2_vs_f32_restatement": [float(f"{e:.3e}") for e in err]}


def _lanes_for(R):
    """lanes_per_ray() of the library (voxe_ray_march.hpp)"""
    for G in (1, 2, 4):
        if R * G >= (1 << 20):
            return G
    return 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--ref_rays", type=int, default=4096)
    ap.add_argument("--side", type=int, default=160)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ray_grad_bench.txt"))
    a = ap.parse_args()
    spec = ops.GridSpec(aabb=((-1.5, 1.5),) * 3, density_scale=100.0 / 3.0, density_pre_act=abi.ACT_IDENTITY,
                        density_post_act=abi.ACT_SOFTPLUS)
    d, f0 = workload.random_grid(a.side)
    dens, feat0 = d.to(DEV).contiguous(), f0.to(DEV).contiguous()
    _, f2 = workload.random_grid(a.side, nfeat=27, seed=44)
    feats = {0: feat0, 2: f2.to(DEV).contiguous()}
    lines, slower = [], False
    ro_i, rd_i = _rays(400, [3])
    ro_b, rd_b = _rays(400, [3 + 12 * j for j in range(8)])
    pick = torch.randperm(ro_b.shape[0], generator=torch.Generator().manual_seed(11))[:32768].to(DEV)
    ro_b, rd_b = ro_b[pick].contiguous(), rd_b[pick].contiguous()
    for deg in (0, 2):
        for name, ro, rd, width in ((f"random{a.side}_400x400_S256_image", ro_i, rd_i, 400),
                                    (f"random{a.side}_batch32768_of_8cams_S256_linear", ro_b, rd_b, 0)):
            lines.append({"case": f"{name}_sh{deg}", **case_times(spec, dens, feat0, feats[deg], deg, ro, rd, 256, width, a.iters,
                                                                   a.ref_rays)})
            print(json.dumps(lines[-1]), flush=True)
            slower = slower or lines[-1]["render_bwd_rays_ms"] > lines[-1]["torch_f32_restatement_scaled_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")
    sys.exit(1 if slower else 0)


if __name__ == "__main__":
    main()
