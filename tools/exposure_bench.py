#!/usr/bin/env python3
"""Exposure-compensation timings: device time (HIP events around --reps back-to-back calls, divided by
--reps; median, minimum and maximum over --iters rounds after 3 warm-up rounds, the contenders taking turns inside every round)
of
  (a) voxe_exposure_fwd_bwd -- loss, mse, d_x and d_delta in one call, L1 -- on the trainer's batch, 32 768 rays over 8 of 100
      cameras, once sorted by camera (memory_order=True) and once shuffled, next to a float32 torch restatement of the same
      outputs (gather of the rows, bmm, l1 / mse, autograd to x and delta) and to the SH-0 voxe_render_fwd + voxe_render_bwd of as
      many rays of the bench's 160^3 grid (the 0.7 ms step the term sits next to);
  (b) voxe_exposure_apply_bwd on the same batch (the chain rule the SSIM term needs), next to torch's autograd of the same;
  (c) voxe_exposure_fit_sums on one 400 x 400 image, next to a float64 torch restatement (the 4 x 4 and 4 x 3 products of
      [x 1] and y).
A call of 10 to 30 us is launch-bound: the figures say what the calls cost in a training iteration, not what the kernels reach
of the memory system.  One JSON line per case, also written to --out.  Exit status 1 when a kernel is slower than its torch
restatement; no other time threshold.

    python tools/exposure_bench.py [--iters 20] [--reps 50] [--out profiles/exposure_bench.txt]
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
R, CAMS, N = 32768, 8, 100


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


def torch_exposure(x, y, ids, delta):
    """float32 torch restatement: (loss, mse, d_x, d_delta)"""
    xr, dl = x.detach().requires_grad_(True), delta.detach().requires_grad_(True)
    rows = dl[ids.long()]
    A = rows[:, :9].reshape(-1, 3, 3) + torch.eye(3, device=x.device)
    c = torch.bmm(A, xr[:, :, None])[:, :, 0] + rows[:, 9:]
    loss = torch.nn.functional.l1_loss(c, y)
    mse = torch.nn.functional.mse_loss(c.detach(), y)
    d_x, d_delta = torch.autograd.grad(loss, (xr, dl))
    return loss.detach(), mse, d_x, d_delta


def torch_apply_bwd(x, ids, delta, g):
    xr, dl = x.detach().requires_grad_(True), delta.detach().requires_grad_(True)
    rows = dl[ids.long()]
    A = rows[:, :9].reshape(-1, 3, 3) + torch.eye(3, device=x.device)
    c = torch.bmm(A, xr[:, :, None])[:, :, 0] + rows[:, 9:]
    return torch.autograd.grad(c, (xr, dl), g)


def torch_fit_sums(x, y):
    u = torch.cat([x.double(), torch.ones_like(x[..., :1], dtype=torch.float64)], dim=-1)
    yd = y.double()
    return u.transpose(1, 2) @ u, u.transpose(1, 2) @ yd, (yd * yd).sum(dim=1)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def _stats(t):
    return ({name: round(v[0], 5) for name, v in t.items()}, {name: [round(v[1], 5), round(v[2], 5)] for name, v in t.items()})


def batch_case(order, render, iters, reps):
    g = torch.Generator().manual_seed(11)
    x, y = torch.rand((R, 3), generator=g).to(DEV), torch.rand((R, 3), generator=g).to(DEV)
    cams = torch.randperm(N, generator=g)[:CAMS]
    ids = cams[torch.randint(0, CAMS, (R,), generator=g)]
    ids = (torch.sort(ids).values if order == "sorted" else ids).to(torch.int32).to(DEV)
    delta = ((torch.rand((N, 12), generator=g) - 0.5) * 0.2).to(DEV)
    up = ((torch.rand((R, 3), generator=g) - 0.5) / R).to(DEV)
    d_x, d_delta = torch.empty_like(x), torch.empty_like(delta)

    def kernel():
        return ops.exposure_fwd_bwd(x, y, ids, delta, "l1", want_mse=True, d_colour=d_x, d_delta=d_delta)

    def kernel_bwd():
        ops.exposure_apply_bwd(x, ids, delta, up, d_colour=d_x, d_delta=d_delta)

    fns = {"kernel": kernel, "torch": lambda: torch_exposure(x, y, ids, delta), "apply_bwd": kernel_bwd,
           "torch_apply_bwd": lambda: torch_apply_bwd(x, ids, delta, up), "render": render}
    med, spread = _stats(_turns(fns, iters, reps))
    loss, mse, _ = kernel()
    t_loss, t_mse, t_dx, t_dd = torch_exposure(x, y, ids, delta)
    agree = {"loss": abs(float(loss) - float(t_loss)), "d_x_rel_l2": _rel(d_x, t_dx), "d_delta_rel_l2": _rel(d_delta, t_dd)}
    return {"case": f"batch{R}_of_{CAMS}_of_{N}_images_{order}", "fwd_bwd_ms": med["kernel"], "torch_fwd_bwd_ms": med["torch"],
            "apply_bwd_ms": med["apply_bwd"], "torch_apply_bwd_ms": med["torch_apply_bwd"], "render_fwd_bwd_ms": med["render"],
            "fwd_bwd_over_torch": round(med["kernel"] / med["torch"], 4),
            "apply_bwd_over_torch": round(med["apply_bwd"] / med["torch_apply_bwd"], 4),
            "fwd_bwd_over_render": round(med["kernel"] / med["render"], 4), "min_max_ms": spread,
            "agreement_with_torch": {k: float(f"{v:.3e}") for k, v in agree.items()}}


def fit_case(iters, reps):
    g = torch.Generator().manual_seed(12)
    x, y = torch.rand((1, 160000, 3), generator=g).to(DEV), torch.rand((1, 160000, 3), generator=g).to(DEV)
    fns = {"kernel": lambda: ops.exposure_fit_sums(x, y), "torch": lambda: torch_fit_sums(x, y)}
    med, spread = _stats(_turns(fns, iters, reps))
    s = ops.exposure_fit_sums(x, y)[0]
    G, h, yy = torch_fit_sums(x, y)
    agree = max(_rel(s[torch.tensor([0, 4, 7, 9])], torch.diagonal(G[0])), _rel(s[10:22], h[0].reshape(-1)), _rel(s[22:], yy[0]))
    return {"case": "fit_sums_1_image_400x400", "fit_sums_ms": med["kernel"], "torch_fit_sums_ms": med["torch"],
            "fit_sums_over_torch": round(med["kernel"] / med["torch"], 4), "min_max_ms": spread,
            "agreement_with_torch_rel_l2": float(f"{agree:.3e}")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exposure_bench.txt"))
    a = ap.parse_args()
    torch.manual_seed(3)
    # the render step the term sits next to: SH-0 forward + backward of 32 768 random rays over 8 cameras, bench grid, S = 256
    spec = ops.GridSpec(aabb=((-1.5, 1.5),) * 3, density_scale=100.0 / 3.0, density_pre_act=abi.ACT_IDENTITY,
                        density_post_act=abi.ACT_SOFTPLUS)
    d, f = workload.random_grid(160)
    dens, feat = d.to(DEV).contiguous(), f.to(DEV).contiguous()
    rays = [ops.cast_rays(400, 400, workload.focal_for(400), *pose_spherical(*workload.synth_pose_angles(3 + 12 * j, 100), workload.RADIUS),
                          DEV) for j in range(CAMS)]
    ro_all, rd_all = torch.cat([r[0] for r in rays]), torch.cat([r[1] for r in rays])
    pick = torch.randperm(ro_all.shape[0], generator=torch.Generator().manual_seed(11))[:R].to(DEV)
    ro, rd = ro_all[pick].contiguous(), rd_all[pick].contiguous()
    params = ops.RenderParams(num_samples=256, near=workload.NEAR, far=workload.FAR, perturb=True, white_bkgd=True, sh_degree=0)
    outs = [torch.empty((R, n), dtype=torch.float32, device=DEV) for n in (3, 1, 1, 1)]
    g_colour = torch.randn((R, 3), generator=torch.Generator().manual_seed(43)).to(DEV)
    r_dens, r_feat = torch.zeros_like(dens), torch.zeros_like(feat)
    ws = ops.Workspace()

    def render():
        ops.render_fwd_into(spec, params, dens, feat, ro, rd, None, *outs, ws, RNG)
        ops.render_bwd_into(spec, params, dens, feat, ro, rd, None, outs[0], outs[1], outs[2], g_colour, None, None, r_dens, r_feat,
                            ws, RNG)

    lines = []
    for order in ("sorted", "shuffled"):
        lines.append(batch_case(order, render, a.iters, a.reps))
        print(json.dumps(lines[-1]), flush=True)
    lines.append(fit_case(a.iters, a.reps))
    print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")
    lost = [(line["case"], key) for line in lines for key in ("fwd_bwd_over_torch", "apply_bwd_over_torch", "fit_sums_over_torch")
            if line.get(key, 0.0) > 1.0]
    if lost:
        print(f"an exposure kernel is slower than its torch restatement: {lost}", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
