#!/usr/bin/env python3
"""Depth-supervision timings: device time (HIP events; median over --iters rounds after warm-up, the
contenders taking turns inside every round) of voxe_depth_fwd_bwd -- loss only, and loss plus gradient, the latter for every
lanes-per-ray split (voxe_depth_debug_lanes) -- next to the SH-0 voxe_render_fwd + voxe_render_bwd of the same rays, cfg and
jitter stream (packed grid reused: the kernels alone) and to a float32 torch restatement (ops.sample_probe, ops.query_points,
cumprod, autograd), on the bench's 160^3 random grid with S = 256:
  (a) 4 096 keypoint rays over 8 cameras, linear order: the trainer's default depth batch;
  (b) 32 768 keypoint rays over 8 cameras, linear order.
The targets sit around each ray's closest approach to the origin, s = max(D / focal, (far - near) / S): a one-pixel reprojection
error.  One JSON line per case, also written to --out.  Exit status 1 when the kernel is slower than the torch restatement.

    python tools/depth_bench.py [--iters 20] [--out profiles/depth_bench.txt]
"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "vox-e_amd")]

from thre3d_atom.utils.imaging_utils import pose_spherical  # noqa: E402
from voxe_hip import abi, ops, workload  # noqa: E402
from voxe_hip.desc import make_grid_desc, make_render_cfg  # noqa: E402

DEV = torch.device("cuda:0")
RNG = (42, 7)
EPS = 1e-5


def _rays(hw, cams):
    rays = [ops.cast_rays(hw, hw, workload.focal_for(hw), *pose_spherical(*workload.synth_pose_angles(cam, 100), workload.RADIUS), DEV)
            for cam in cams]
    return torch.cat([r[0] for r in rays]).contiguous(), torch.cat([r[1] for r in rays]).contiguous()


def _turns(fns, iters):
    """median device time (ms) of each of `fns`, taking turns inside every round"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {name: [] for name in fns}
    for i in range(iters + 3):
        for name, fn in fns.items():
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= 3:
                times[name].append(e0.elapsed_time(e1))
    return {name: sorted(t)[len(t) // 2] for name, t in times.items()}


def torch_depth(spec, params, dens, feat, ro, rd, D, s, ws):
    """the restatement in float32 torch ops: the forward's samples from ops.sample_probe, sigma from the point query, weights
    by cumprod with alpha = -expm1(-x); returns (loss, d loss / d densities)"""
    probe = ops.sample_probe(spec, params, dens, feat, ro, rd, None, rng=RNG, outputs=("z", "inside"))
    z, inside = probe["z"], probe["inside"]
    R, S = z.shape
    d = dens.detach().requires_grad_(True)
    pts = (ro[:, None, :] + rd[:, None, :] * z[:, :, None]).reshape(-1, 3)
    sigma = ops.query_points(spec, d, feat, pts, ws)[:, -1].reshape(R, S) * inside
    dl = torch.cat([z[:, 1:] - z[:, :-1], torch.full((R, 1), 1e10, device=z.device)], dim=1)
    alpha = -torch.expm1(-sigma * (dl * rd.norm(dim=1)[:, None]))
    T = torch.cumprod(torch.cat([torch.ones((R, 1), device=z.device), 1.0 - alpha[:, :-1]], dim=1), dim=1)
    dz = torch.cat([z[:, 1:] - z[:, :-1], torch.zeros((R, 1), device=z.device)], dim=1)
    t = (z - D[:, None]) / s[:, None]
    loss = -(torch.exp(-0.5 * t * t) * dz * torch.log(alpha * T + EPS)).sum(dim=1).mean()
    (g,) = torch.autograd.grad(loss, d)
    return loss.detach(), g


def case_times(spec, dens, feat, ro, rd, S, iters):
    R = ro.shape[0]
    dims = tuple(int(n) for n in dens.shape[:3])
    L = ops.lib()
    g = make_grid_desc(dens.data_ptr(), 0, dims, 0, spec.aabb, spec.density_scale, spec.density_pre_act, spec.density_post_act)
    c = make_render_cfg(S, workload.NEAR, workload.FAR, True, seed=RNG[0], rng_offset=RNG[1])
    st = torch.cuda.current_stream().cuda_stream
    D = -(ro * rd).sum(dim=1) / (rd * rd).sum(dim=1) + torch.empty(R, device=DEV).uniform_(-0.4, 0.4, generator=None)
    s = (D / workload.focal_for(400)).clamp_min((workload.FAR - workload.NEAR) / S).contiguous()
    loss = torch.zeros((), dtype=torch.float32, device=DEV)
    ray_loss = torch.empty((R,), dtype=torch.float32, device=DEV)
    d_d = torch.empty_like(dens)
    sc = torch.empty(L.voxe_depth_scratch_bytes(R), dtype=torch.uint8, device=DEV)

    def depth(grad):
        assert L.voxe_depth_fwd_bwd(ctypes.byref(g), ctypes.byref(c), ro.data_ptr(), rd.data_ptr(), R, None, D.data_ptr(),
                                    s.data_ptr(), None, EPS, 1.0, loss.data_ptr(), ray_loss.data_ptr(),
                                    d_d.data_ptr() if grad else None, 0, sc.data_ptr(), sc.numel(), st) == 0

    def depth_lanes(lanes):
        assert L.voxe_depth_debug_lanes(lanes) == 0
        depth(True)
        assert L.voxe_depth_debug_lanes(0) == 0

    params = ops.RenderParams(num_samples=S, near=workload.NEAR, far=workload.FAR, perturb=True, white_bkgd=True, sh_degree=0)
    outs = [torch.empty((R, n), dtype=torch.float32, device=DEV) for n in (3, 1, 1, 1)]
    g_colour = torch.randn((R, 3), generator=torch.Generator().manual_seed(43)).to(DEV)
    r_dens, r_feat = torch.zeros_like(dens), torch.zeros_like(feat)
    ws, ws_query = ops.Workspace(), ops.Workspace()

    def render():
        ops.render_fwd_into(spec, params, dens, feat, ro, rd, None, *outs, ws, RNG)
        ops.render_bwd_into(spec, params, dens, feat, ro, rd, None, outs[0], outs[1], outs[2], g_colour, None, None, r_dens, r_feat,
                            ws, RNG)

    fns = {"loss": lambda: depth(False), "loss_grad": lambda: depth(True), "render": render,
           "torch": lambda: torch_depth(spec, params, dens, feat, ro, rd, D, s, ws_query)}
    fns.update({f"lanes{n}": (lambda n=n: depth_lanes(n)) for n in (1, 2, 4, 8)})
    t = _turns(fns, iters)
    depth(True)
    t_loss, t_grad = torch_depth(spec, params, dens, feat, ro, rd, D, s, ws_query)
    agree = float((d_d.double() - t_grad.double()).norm() / t_grad.double().norm())
    return {"rays": R, "depth_loss_ms": round(t["loss"], 4), "depth_loss_grad_ms": round(t["loss_grad"], 4),
            "loss_grad_ms_by_lanes": {str(n): round(t[f"lanes{n}"], 4) for n in (1, 2, 4, 8)},
            "render_fwd_bwd_ms": round(t["render"], 4), "torch_loss_grad_ms": round(t["torch"], 4),
            "loss_grad_over_render": round(t["loss_grad"] / t["render"], 3),
            "loss_grad_over_torch": round(t["loss_grad"] / t["torch"], 4), "loss": round(float(loss), 6),
            "torch_loss": round(float(t_loss), 6), "grad_rel_l2_to_torch": float(f"{agree:.3e}"),
            "voxels_with_gradient": int((d_d != 0).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_bench.txt"))
    a = ap.parse_args()
    torch.manual_seed(3)
    spec = ops.GridSpec(aabb=((-1.5, 1.5),) * 3, density_scale=100.0 / 3.0, density_pre_act=abi.ACT_IDENTITY,
                        density_post_act=abi.ACT_SOFTPLUS)
    d, f = workload.random_grid(160)
    dens, feat = d.to(DEV).contiguous(), f.to(DEV).contiguous()
    ro_all, rd_all = _rays(400, [3 + 12 * j for j in range(8)])
    lines = []
    for R in (4096, 32768):
        pick = torch.randperm(ro_all.shape[0], generator=torch.Generator().manual_seed(11))[:R].to(DEV)
        ro, rd = ro_all[pick].contiguous(), rd_all[pick].contiguous()
        lines.append({"case": f"random160_keypoints{R}_of_8cams_S256_linear", **case_times(spec, dens, feat, ro, rd, 256, a.iters)})
        print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")
    lost = [line["case"] for line in lines if line["loss_grad_over_torch"] > 1.0]
    if lost:
        print(f"the depth kernel is slower than the torch restatement: {lost}", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
