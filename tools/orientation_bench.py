#!/usr/bin/env python3
"""Orientation-loss timings: device time (HIP events; median, minimum and maximum over --iters rounds
after 3 warm-up rounds, the contenders taking turns inside every round) of voxe_orientation_fwd_bwd -- loss only, and loss plus
gradient, the latter for every lanes-per-ray split (voxe_orientation_debug_lanes) -- next to the SH-0 voxe_render_fwd +
voxe_render_bwd of the same rays, cfg and jitter stream (packed grid reused: the kernels alone), to voxe_distortion_fwd_bwd
(loss plus gradient) on the same rays, and to a float32 torch restatement (ops.sample_probe, one gather of the 8 corners for the
value and the cell gradient, cumprod, autograd), on the bench's 160^3 random grid with S = 256:
  (a) one 400 x 400 camera, image order;
  (b) the trainer's batch, 32 768 random rays over 8 cameras, linear order.
One JSON line per case, also written to --out.  Exit status 1 when the kernel is slower than the torch restatement; no other
time threshold.

    python tools/orientation_bench.py [--iters 10] [--out profiles/orientation_bench.txt]
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
from voxe_hip.desc import make_grid_desc, make_render_cfg, norm_constants  # noqa: E402

DEV = torch.device("cuda:0")
RNG = (42, 7)
EPS = 1e-2


def _rays(hw, cams):
    rays = [ops.cast_rays(hw, hw, workload.focal_for(hw), *pose_spherical(*workload.synth_pose_angles(cam, 100), workload.RADIUS), DEV)
            for cam in cams]
    return torch.cat([r[0] for r in rays]).contiguous(), torch.cat([r[1] for r in rays]).contiguous()


def _turns(fns, iters):
    """(median, min, max) device time (ms) of each of `fns`, taking turns inside every round"""
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
    return {name: (sorted(t)[len(t) // 2], min(t), max(t)) for name, t in times.items()}


def torch_orientation(spec, params, dens, feat, ro, rd, image_width):
    """the restatement in float32 torch ops: the forward's samples from ops.sample_probe, the 8 corners gathered once (zero
    padding) for the interpolated value and the cell gradient, weights by cumprod; returns (loss, d loss / d densities)"""
    p = ops.RenderParams(num_samples=params.num_samples, near=params.near, far=params.far, perturb=True, image_width=image_width)
    probe = ops.sample_probe(spec, p, dens, feat, ro, rd, None, rng=RNG, outputs=("z", "inside"))
    z, inside = probe["z"], probe["inside"]
    R, S = z.shape
    X, Y, Z = (int(n) for n in dens.shape[:3])
    d = dens.detach().requires_grad_(True)
    v = d.reshape(-1) * spec.density_scale
    pts = (ro[:, None, :] + rd[:, None, :] * z[:, :, None]).reshape(-1, 3)
    scale, bias = (torch.tensor(a, device=DEV) for a in norm_constants(spec.aabb))
    dims = torch.tensor([X, Y, Z], device=DEV, dtype=torch.float32)
    u = ((pts * scale + bias + 1.0) * dims - 1.0) * 0.5
    fl = torch.floor(u)
    i0, w1 = fl.long(), u - fl
    w = torch.stack([1.0 - w1, w1], dim=-1)
    c = {}
    for q in range(8):
        dx, dy, dz = q & 1, (q >> 1) & 1, q >> 2
        i, j, k = i0[:, 0] + dx, i0[:, 1] + dy, i0[:, 2] + dz
        ok = (i >= 0) & (i < X) & (j >= 0) & (j < Y) & (k >= 0) & (k < Z)
        c[dx, dy, dz] = v[(i.clamp(0, X - 1) * Y + j.clamp(0, Y - 1)) * Z + k.clamp(0, Z - 1)] * ok
    val = sum(w[:, 0, a] * w[:, 1, b] * w[:, 2, e] * c[a, b, e] for a in range(2) for b in range(2) for e in range(2))
    gx = sum(w[:, 1, b] * w[:, 2, e] * (c[1, b, e] - c[0, b, e]) for b in range(2) for e in range(2))
    gy = sum(w[:, 0, a] * w[:, 2, e] * (c[a, 1, e] - c[a, 0, e]) for a in range(2) for e in range(2))
    gz = sum(w[:, 0, a] * w[:, 1, b] * (c[a, b, 1] - c[a, b, 0]) for a in range(2) for b in range(2))
    G = torch.stack([gx, gy, gz], dim=1) * (dims * scale * 0.5)
    sigma = torch.nn.functional.softplus(val).reshape(R, S) * inside
    dnorm = rd.norm(dim=1)
    dl = torch.cat([z[:, 1:] - z[:, :-1], torch.full((R, 1), 1e10, device=DEV)], dim=1)
    alpha = 1.0 - torch.exp(-sigma * (dl * dnorm[:, None]))
    T = torch.cumprod(torch.cat([torch.ones((R, 1), device=DEV), 1.0 - alpha[:, :-1]], dim=1), dim=1)
    un = (rd / dnorm[:, None])[:, None, :].expand(R, S, 3).reshape(-1, 3)
    cc = torch.relu(-(G * un).sum(dim=1)) / torch.sqrt((G * G).sum(dim=1) + EPS * EPS)
    loss = (alpha * T * (cc * cc).reshape(R, S)).sum(dim=1).mean()
    (g,) = torch.autograd.grad(loss, d)
    return loss.detach(), g


def case_times(spec, dens, feat, ro, rd, S, image_width, iters):
    R = ro.shape[0]
    dims = tuple(int(n) for n in dens.shape[:3])
    L = ops.lib()
    g = make_grid_desc(dens.data_ptr(), 0, dims, 0, spec.aabb, spec.density_scale, spec.density_pre_act, spec.density_post_act)
    c = make_render_cfg(S, workload.NEAR, workload.FAR, True, seed=RNG[0], rng_offset=RNG[1], image_width=image_width)
    st = torch.cuda.current_stream().cuda_stream
    loss = torch.zeros((), dtype=torch.float32, device=DEV)
    ray_loss = torch.empty((R,), dtype=torch.float32, device=DEV)
    d_d, d_dist = torch.empty_like(dens), torch.empty_like(dens)
    sc = torch.empty(max(L.voxe_orientation_scratch_bytes(R), L.voxe_distortion_scratch_bytes(R)), dtype=torch.uint8, device=DEV)

    def orientation(grad):
        assert L.voxe_orientation_fwd_bwd(ctypes.byref(g), ctypes.byref(c), ro.data_ptr(), rd.data_ptr(), R, None, None, EPS, 1.0,
                                          loss.data_ptr(), ray_loss.data_ptr(), d_d.data_ptr() if grad else None, 0, sc.data_ptr(),
                                          sc.numel(), st) == 0

    def orientation_lanes(lanes):
        assert L.voxe_orientation_debug_lanes(lanes) == 0
        orientation(True)
        assert L.voxe_orientation_debug_lanes(0) == 0

    def distortion():
        assert L.voxe_distortion_fwd_bwd(ctypes.byref(g), ctypes.byref(c), ro.data_ptr(), rd.data_ptr(), R, None, 1.0, loss.data_ptr(),
                                         ray_loss.data_ptr(), d_dist.data_ptr(), 0, sc.data_ptr(), sc.numel(), st) == 0

    params = ops.RenderParams(num_samples=S, near=workload.NEAR, far=workload.FAR, perturb=True, white_bkgd=True, sh_degree=0,
                              image_width=image_width)
    outs = [torch.empty((R, n), dtype=torch.float32, device=DEV) for n in (3, 1, 1, 1)]
    g_colour = torch.randn((R, 3), generator=torch.Generator().manual_seed(43)).to(DEV)
    r_dens, r_feat = torch.zeros_like(dens), torch.zeros_like(feat)
    ws = ops.Workspace()

    def render():
        ops.render_fwd_into(spec, params, dens, feat, ro, rd, None, *outs, ws, RNG)
        ops.render_bwd_into(spec, params, dens, feat, ro, rd, None, outs[0], outs[1], outs[2], g_colour, None, None, r_dens, r_feat,
                            ws, RNG)

    fns = {"loss": lambda: orientation(False), "loss_grad": lambda: orientation(True), "render": render, "distortion": distortion,
           "torch": lambda: torch_orientation(spec, params, dens, feat, ro, rd, image_width)}
    fns.update({f"lanes{n}": (lambda n=n: orientation_lanes(n)) for n in (1, 2, 4, 8)})
    t = _turns(fns, iters)
    orientation(True)
    torch.cuda.synchronize()
    k_loss = float(loss)
    t_loss, t_grad = torch_orientation(spec, params, dens, feat, ro, rd, image_width)
    agree = float((d_d.double() - t_grad.double()).norm() / t_grad.double().norm())
    med = {name: v[0] for name, v in t.items()}
    return {"rays": R, "orientation_loss_ms": round(med["loss"], 4), "orientation_loss_grad_ms": round(med["loss_grad"], 4),
            "loss_grad_ms_by_lanes": {str(n): round(med[f"lanes{n}"], 4) for n in (1, 2, 4, 8)},
            "render_fwd_bwd_ms": round(med["render"], 4), "distortion_loss_grad_ms": round(med["distortion"], 4),
            "torch_loss_grad_ms": round(med["torch"], 4),
            "min_max_ms": {name: [round(v[1], 4), round(v[2], 4)] for name, v in t.items()},
            "loss_grad_over_render": round(med["loss_grad"] / med["render"], 3),
            "loss_grad_over_distortion": round(med["loss_grad"] / med["distortion"], 3),
            "loss_grad_over_torch": round(med["loss_grad"] / med["torch"], 4), "loss": round(k_loss, 6),
            "torch_loss": round(float(t_loss), 6), "grad_rel_l2_to_torch": float(f"{agree:.3e}"),
            "voxels_with_gradient": int((d_d != 0).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orientation_bench.txt"))
    a = ap.parse_args()
    torch.manual_seed(3)
    spec = ops.GridSpec(aabb=((-1.5, 1.5),) * 3, density_scale=100.0 / 3.0, density_pre_act=abi.ACT_IDENTITY,
                        density_post_act=abi.ACT_SOFTPLUS)
    d, f = workload.random_grid(160)
    dens, feat = d.to(DEV).contiguous(), f.to(DEV).contiguous()
    lines = []
    ro, rd = _rays(400, [3])
    lines.append({"case": "random160_cam3_400x400_S256_image", **case_times(spec, dens, feat, ro, rd, 256, 400, a.iters)})
    print(json.dumps(lines[-1]), flush=True)
    ro_all, rd_all = _rays(400, [3 + 12 * j for j in range(8)])
    pick = torch.randperm(ro_all.shape[0], generator=torch.Generator().manual_seed(11))[:32768].to(DEV)
    ro, rd = ro_all[pick].contiguous(), rd_all[pick].contiguous()
    lines.append({"case": "random160_batch32768_of_8cams_S256_linear", **case_times(spec, dens, feat, ro, rd, 256, 0, a.iters)})
    print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")
    lost = [line["case"] for line in lines if line["loss_grad_over_torch"] > 1.0]
    if lost:
        print(f"the orientation kernel is slower than the torch restatement: {lost}", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
