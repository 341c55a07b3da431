#!/usr/bin/env python3
"""Robust-loss timings: device time (HIP events around --reps back-to-back calls, divided by --reps;
median, minimum and maximum over --iters rounds after 3 warm-up rounds, the contenders taking turns inside every round) of
  (a) voxe_robust_fwd_bwd with all outputs (loss, mse, tau, mask, stats, d_x), L1, quantile 0.5;
  (b) the mask alone (mask, tau, stats: ops.robust_mask);
  (c) the same call with mask_in given (loss, mse, mask, d_x under another call's mask: the trainer's diffuse term);
  (d) a float32 torch restatement of (a) on the same GPU: residual, torch.kthvalue, avg_pool2d with zero padding, the
      reductions, autograd for d_x;
  (e) the SH-0 voxe_render_fwd + voxe_render_bwd of as many rays of the bench's 160^3 grid, for scale
on the trainer's batch (N = 128 patches of 16 x 16 x 3), on N = 32 patches of 32 x 32 x 3, and on one 400 x 400 image cut into
625 patches of 16 x 16.  A call is a handful of launches of a few microseconds each: the figures say what the calls cost in a
training iteration, not what the kernels reach of the memory system.  One JSON line per case, also written to --out.  Exit
status 1 when (a) is slower than (d) at any size; no other time threshold.

    python tools/robust_bench.py [--iters 20] [--reps 50] [--out profiles/robust_bench.txt]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "vox-e_amd")]

from thre3d_atom.utils.imaging_utils import pose_spherical  # noqa: E402
from voxe_hip import abi, ops, workload  # noqa: E402

DEV = torch.device("cuda:0")
RNG = (42, 7)
CAMS = 8
CASES = (("trainer_batch_128x16x16x3", 128, 16), ("32x32x32x3", 32, 32), ("image_400x400_as_625x16x16x3", 625, 16))
# launches per call, from launch_robust (voxe_robust.hip): the clear of the histograms, three counting passes, the patch pass,
# the finalize; with mask_in the patch pass and the finalize
LAUNCHES = {"all_outputs": 6, "mask_only": 6, "mask_in": 2}


def _turns(fns, iters, reps):
    """(median, min, max) device time (ms) of one call of each of `fns`, taking turns inside every round"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {name: [] for name in fns}
    for i in range(iters + 3):
        for name, fn in fns.items():
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            if i >= 3:
                times[name].append(e0.elapsed_time(e1) / reps)
    return {name: (sorted(t)[len(t) // 2], min(t), max(t)) for name, t in times.items()}


def torch_robust(x, y, rank, smooth_min, patch_min, inner):
    """float32 torch restatement of the call with all outputs: (loss, mse, tau, mask, stats, d_x)"""
    xr = x.detach().requires_grad_(True)
    d = xr - y
    e = (d.detach() * d.detach()).sum(-1)
    tau = torch.kthvalue(e.reshape(-1), rank + 1).values
    a = (e <= tau).to(torch.float32)
    count = torch.nn.functional.avg_pool2d(a[:, None], 3, stride=1, padding=1, divisor_override=1)[:, 0]
    c = torch.maximum(a, (count >= smooth_min).to(torch.float32))
    whole = (c.sum(dim=(1, 2)) >= patch_min).to(torch.float32)
    w = torch.maximum(c, whole[:, None, None] * inner)
    loss = (w[..., None] * d.abs()).mean()
    mse = (d.detach() * d.detach()).mean()
    (d_x,) = torch.autograd.grad(loss, xr)
    stats = torch.stack([a.sum(), c.sum(), w.sum()])
    return loss.detach(), mse, tau, w.to(torch.uint8), stats, d_x


def case(name, N, P, render_setup, iters, reps):
    g = torch.Generator().manual_seed(11 + N)
    y = torch.rand((N, P, P, 3), generator=g)
    x = y + 0.02 * torch.randn((N, P, P, 3), generator=g)
    blob = torch.rand((N, P, P), generator=g) < 0.2            # a fifth of the pixels far from the photographs
    x[blob] = torch.rand((int(blob.sum()), 3), generator=g)
    x, y = x.to(DEV).contiguous(), y.to(DEV).contiguous()
    M = N * P * P
    rank, smooth_min, patch_min = ops.robust_parameters(M, P, 0.5, 5, 0.6)
    i = torch.arange(P, device=DEV)
    one = ((i >= P // 4) & (i < P // 4 + P // 2)).to(torch.float32)
    inner = one[:, None] * one[None, :]
    d_x = torch.empty_like(x)
    mask = ops.robust_mask(x, y)[0]

    def all_outputs():
        return ops.robust_fwd_bwd(x, y, rank, smooth_min, patch_min, "l1", d_x=d_x)

    def mask_in():
        return ops.robust_fwd_bwd(x, y, kind="l1", mask=mask, want_tau=False, want_stats=False, d_x=d_x)

    fns = {"all_outputs": all_outputs, "mask_only": lambda: ops.robust_mask(x, y), "mask_in": mask_in,
           "torch": lambda: torch_robust(x, y, rank, smooth_min, patch_min, inner), "render": render_setup(M)}
    t = _turns(fns, iters, reps)
    med = {k: round(v[0], 5) for k, v in t.items()}
    spread = {k: [round(v[1], 5), round(v[2], 5)] for k, v in t.items()}
    loss, mse, tau, m, stats = all_outputs()
    t_loss, t_mse, t_tau, t_m, t_stats, t_dx = torch_robust(x, y, rank, smooth_min, patch_min, inner)
    agree = {"mask_bytes_that_differ": int((m != t_m).sum()), "tau": abs(float(tau) - float(t_tau)),
             "loss": abs(float(loss) - float(t_loss)),
             "d_x_rel_l2": float((d_x.double() - t_dx.double()).norm() / t_dx.double().norm().clamp_min(1e-300))}
    return {"case": name, "N": N, "P": P, "C": 3, "pixels": M, "all_outputs_ms": med["all_outputs"], "mask_only_ms": med["mask_only"],
            "mask_in_ms": med["mask_in"], "torch_ms": med["torch"], "render_fwd_bwd_ms": med["render"],
            "all_outputs_over_torch": round(med["all_outputs"] / med["torch"], 4),
            "all_outputs_over_render": round(med["all_outputs"] / med["render"], 4), "launches_per_call": LAUNCHES,
            "inlier_fractions": [round(int(v) / M, 4) for v in stats.tolist()], "min_max_ms": spread,
            "agreement_with_torch": {k: (v if isinstance(v, int) else float(f"{v:.3e}")) for k, v in agree.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "robust_bench.txt"))
    a = ap.parse_args()
    torch.manual_seed(3)
    # the render step the term sits next to: SH-0 forward + backward of as many random rays over 8 cameras, bench grid, S = 256
    spec = ops.GridSpec(aabb=((-1.5, 1.5),) * 3, density_scale=100.0 / 3.0, density_pre_act=abi.ACT_IDENTITY,
                        density_post_act=abi.ACT_SOFTPLUS)
    d, f = workload.random_grid(160)
    dens, feat = d.to(DEV).contiguous(), f.to(DEV).contiguous()
    rays = [ops.cast_rays(400, 400, workload.focal_for(400), *pose_spherical(*workload.synth_pose_angles(3 + 12 * j, 100), workload.RADIUS),
                          DEV) for j in range(CAMS)]
    ro_all, rd_all = torch.cat([r[0] for r in rays]), torch.cat([r[1] for r in rays])
    params = ops.RenderParams(num_samples=256, near=workload.NEAR, far=workload.FAR, perturb=True, white_bkgd=True, sh_degree=0)
    r_dens, r_feat = torch.zeros_like(dens), torch.zeros_like(feat)
    ws = ops.Workspace()

    def render_setup(R):
        pick = torch.randperm(ro_all.shape[0], generator=torch.Generator().manual_seed(11))[:R].to(DEV)
        ro, rd = ro_all[pick].contiguous(), rd_all[pick].contiguous()
        outs = [torch.empty((R, n), dtype=torch.float32, device=DEV) for n in (3, 1, 1, 1)]
        g_colour = torch.randn((R, 3), generator=torch.Generator().manual_seed(43)).to(DEV)

        def render():
            ops.render_fwd_into(spec, params, dens, feat, ro, rd, None, *outs, ws, RNG)
            ops.render_bwd_into(spec, params, dens, feat, ro, rd, None, outs[0], outs[1], outs[2], g_colour, None, None, r_dens,
                                r_feat, ws, RNG)

        return render

    lines = []
    for name, N, P in CASES:
        lines.append(case(name, N, P, render_setup, a.iters, a.reps))
        print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")
    lost = [line["case"] for line in lines if line["all_outputs_over_torch"] > 1.0]
    if lost:
        print(f"voxe_robust_fwd_bwd is slower than its torch restatement: {lost}", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
