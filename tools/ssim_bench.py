#!/usr/bin/env python3
"""SSIM timings: device time (HIP events; warm-up, then the median of --iters rounds in which the
candidates take turns, all in this one process) of
  voxe_ssim_fwd_bwd      loss only (mean + per-image), and loss plus gradient;
  a float32 torch restatement (separable grouped conv2d, autograd for the gradient) of the same definition;
  the SH-0 voxe_render_fwd + voxe_render_bwd of as many rays on the bench's 160^3 random grid with S = 256 (packed grid reused),
on three shapes: one 400 x 400 x 3 image, one 800 x 800 x 3 image, and the trainer's 32 patches of 32 x 32 x 3 (a 32 768-ray batch).
One JSON line per shape, also written to --out.  Exits 1 when loss plus gradient is slower than torch on any shape.

    python tools/ssim_bench.py [--iters 50] [--out profiles/ssim_bench.txt]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "vox-e_amd")]

from thre3d_atom.utils.imaging_utils import pose_spherical  # noqa: E402
from voxe_hip import abi, ops, workload  # noqa: E402

DEV = torch.device("cuda:0")
RNG = (42, 7)
WARMUP = 5


def _window():
    g = torch.exp(-((torch.arange(11, dtype=torch.float64) - 5) ** 2) / 4.5)
    return (g / g.sum()).float().to(DEV)


def torch_ssim(x, y, wh, wv):
    """float32, channel-last in, the textbook variance form: the mean over valid windows"""
    C = x.shape[-1]
    xc, yc = x.permute(0, 3, 1, 2), y.permute(0, 3, 1, 2)

    def blur(t):
        return F.conv2d(F.conv2d(t, wh, groups=C), wv, groups=C)

    mx, my = blur(xc), blur(yc)
    vx, vy, vxy = blur(xc * xc) - mx * mx, blur(yc * yc) - my * my, blur(xc * yc) - mx * my
    S = (2 * mx * my + 1e-4) * (2 * vxy + 9e-4) / ((mx * mx + my * my + 1e-4) * (vx + vy + 9e-4))
    return S.mean()


def _turns_ms(candidates, iters):
    """median device time of each candidate; within a round every candidate runs once, and the order rotates from round to round"""
    names = list(candidates)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {n: [] for n in names}
    for i in range(iters + WARMUP):
        for k in range(len(names)):
            name = names[(i + k) % len(names)]
            e0.record()
            candidates[name]()
            e1.record()
            e1.synchronize()
            if i >= WARMUP:
                times[name].append(e0.elapsed_time(e1))
    return {n: sorted(t)[len(t) // 2] for n, t in times.items()}


def _rays(hw, cams):
    rays = [ops.cast_rays(hw, hw, workload.focal_for(hw), *pose_spherical(*workload.synth_pose_angles(cam, 100), workload.RADIUS), DEV)
            for cam in cams]
    return torch.cat([r[0] for r in rays]).contiguous(), torch.cat([r[1] for r in rays]).contiguous()


def case_times(shape, spec, dens, feat, ro, rd, width, iters):
    N, H, W, C = shape
    gen = torch.Generator().manual_seed(17)
    y = torch.rand(shape, generator=gen).to(DEV)
    x = (y + 0.1 * torch.randn(shape, generator=gen).to(DEV)).clamp(0, 1).contiguous()
    d_x = torch.empty_like(x)
    g = _window()
    wh, wv = g.view(1, 1, 1, 11).repeat(C, 1, 1, 1), g.view(1, 1, 11, 1).repeat(C, 1, 1, 1)
    xg = x.clone().requires_grad_(True)

    def torch_grad():
        xg.grad = None
        torch_ssim(xg, y, wh, wv).backward()

    def torch_loss():
        with torch.no_grad():
            torch_ssim(x, y, wh, wv)

    R = ro.shape[0]
    assert R == N * H * W
    params = ops.RenderParams(num_samples=256, near=workload.NEAR, far=workload.FAR, perturb=True, white_bkgd=True, sh_degree=0,
                              image_width=width)
    outs = [torch.empty((R, n), dtype=torch.float32, device=DEV) for n in (3, 1, 1, 1)]
    g_colour = torch.randn((R, 3), generator=torch.Generator().manual_seed(43)).to(DEV)
    r_dens, r_feat = torch.zeros_like(dens), torch.zeros_like(feat)
    ws = ops.Workspace()

    def render():
        ops.render_fwd_into(spec, params, dens, feat, ro, rd, None, *outs, ws, RNG)
        ops.render_bwd_into(spec, params, dens, feat, ro, rd, None, outs[0], outs[1], outs[2], g_colour, None, None, r_dens, r_feat,
                            ws, RNG)

    t = _turns_ms({"voxe_loss": lambda: ops.ssim_fwd_bwd(x, y), "voxe_loss_grad": lambda: ops.ssim_fwd_bwd(x, y, d_x=d_x),
                   "torch_loss": torch_loss, "torch_loss_grad": torch_grad, "render": render}, iters)
    mean = float(ops.ssim_fwd_bwd(x, y, d_x=d_x)[0])
    want = float(torch_ssim(x, y, wh, wv))
    rel = float((d_x - xg.grad).norm() / xg.grad.norm())
    return {"shape": list(shape), "rays": R, "ssim_loss_ms": round(t["voxe_loss"], 4), "ssim_loss_grad_ms": round(t["voxe_loss_grad"], 4),
            "torch_loss_ms": round(t["torch_loss"], 4), "torch_loss_grad_ms": round(t["torch_loss_grad"], 4),
            "render_fwd_bwd_ms": round(t["render"], 4), "torch_over_voxe_loss": round(t["torch_loss"] / t["voxe_loss"], 2),
            "torch_over_voxe_loss_grad": round(t["torch_loss_grad"] / t["voxe_loss_grad"], 2),
            "loss_grad_over_render": round(t["voxe_loss_grad"] / t["render"], 4), "ssim": round(mean, 6),
            "ssim_minus_torch": float(f"{mean - want:.2e}"), "grad_rel_l2_to_torch": float(f"{rel:.2e}")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssim_bench.txt"))
    a = ap.parse_args()
    spec = ops.GridSpec(aabb=((-1.5, 1.5),) * 3, density_scale=100.0 / 3.0, density_pre_act=abi.ACT_IDENTITY,
                        density_post_act=abi.ACT_SOFTPLUS)
    d, f = workload.random_grid(160)
    dens, feat = d.to(DEV).contiguous(), f.to(DEV).contiguous()
    lines = []
    for hw in (400, 800):
        ro, rd = _rays(hw, [3])
        lines.append({"case": f"image_{hw}x{hw}x3", **case_times((1, hw, hw, 3), spec, dens, feat, ro, rd, hw, a.iters)})
        print(json.dumps(lines[-1]), flush=True)
    # 32 patches of 32 x 32 over 8 cameras of 400 x 400: the trainer's batch at ray_batch_size 32768, ssim_patch_size 32
    ro, rd = _rays(400, [3 + 12 * j for j in range(8)])
    gen = torch.Generator().manual_seed(11)
    cams, top, left = (torch.randint(0, n, (32,), generator=gen) for n in (8, 400 - 31, 400 - 31))
    offs = torch.arange(32)
    flat = ((cams[:, None, None] * 400 + top[:, None, None] + offs[None, :, None]) * 400 + left[:, None, None] + offs[None, None, :])
    flat = flat.reshape(-1).to(DEV)
    lines.append({"case": "patches_32_of_32x32x3", **case_times((32, 32, 32, 3), spec, dens, feat, ro[flat].contiguous(),
                                                               rd[flat].contiguous(), 0, a.iters)})
    print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")
    slower = [line["case"] for line in lines if line["ssim_loss_grad_ms"] > line["torch_loss_grad_ms"]]
    if slower:
        print(f"loss + gradient is slower than the torch restatement on: {slower}", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
