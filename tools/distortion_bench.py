#!/usr/bin/env python3
"""Distortion-loss timings: device time (HIP events, median of --iters calls after warm-up) of
voxe_distortion_fwd_bwd -- loss only, and loss plus gradient -- next to the SH-0 voxe_render_fwd + voxe_render_bwd and
voxe_render_normals of the same rays, cfg and jitter stream, on the bench's 160^3 random grid with S = 256:
  (a) one 400 x 400 camera, image order;
  (b) a 32 768-ray random batch over 8 cameras, linear order: the trainer's shape.
The render is timed twice: on a packed grid that is reused (the kernels alone) and with the grid re-packed before and the
gradient un-packed after, as a training iteration runs it.  The loss-plus-gradient call is also timed for every lanes-per-ray
split (voxe_distortion_debug_lanes).  One JSON line per case, also written to --out.

    python tools/distortion_bench.py [--iters 20] [--out profiles/distortion_bench.txt]
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


def _median_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for i in range(iters + 3):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i >= 3:
            times.append(e0.elapsed_time(e1))
    return sorted(times)[len(times) // 2]


def _rays(hw, cams):
    rays = [ops.cast_rays(hw, hw, workload.focal_for(hw), *pose_spherical(*workload.synth_pose_angles(cam, 100), workload.RADIUS), DEV)
            for cam in cams]
    return torch.cat([r[0] for r in rays]).contiguous(), torch.cat([r[1] for r in rays]).contiguous()


def case_times(spec, dens, feat, ro, rd, S, width, iters):
    R = ro.shape[0]
    dims = tuple(int(n) for n in dens.shape[:3])
    L = ops.lib()
    g = make_grid_desc(dens.data_ptr(), 0, dims, 0, spec.aabb, spec.density_scale, spec.density_pre_act, spec.density_post_act)
    c = make_render_cfg(S, workload.NEAR, workload.FAR, True, seed=RNG[0], rng_offset=RNG[1], image_width=width)
    st = torch.cuda.current_stream().cuda_stream
    loss = torch.zeros((), dtype=torch.float32, device=DEV)
    ray_loss = torch.empty((R,), dtype=torch.float32, device=DEV)
    d_d = torch.empty_like(dens)
    sc = torch.empty(L.voxe_distortion_scratch_bytes(R), dtype=torch.uint8, device=DEV)
    nrm = torch.empty((R, 3), dtype=torch.float32, device=DEV)
    depth, acc = (torch.empty((R, 1), dtype=torch.float32, device=DEV) for _ in range(2))

    def distortion(grad):
        assert L.voxe_distortion_fwd_bwd(ctypes.byref(g), ctypes.byref(c), ro.data_ptr(), rd.data_ptr(), R, None, 1.0,
                                         loss.data_ptr(), ray_loss.data_ptr(), d_d.data_ptr() if grad else None, 0, sc.data_ptr(),
                                         sc.numel(), st) == 0

    def normals():
        assert L.voxe_render_normals(ctypes.byref(g), ctypes.byref(c), ro.data_ptr(), rd.data_ptr(), R, None, nrm.data_ptr(),
                                     depth.data_ptr(), acc.data_ptr(), st) == 0

    params = ops.RenderParams(num_samples=S, near=workload.NEAR, far=workload.FAR, perturb=True, white_bkgd=True, sh_degree=0,
                              image_width=width)
    outs = [torch.empty((R, n), dtype=torch.float32, device=DEV) for n in (3, 1, 1, 1)]
    g_colour = torch.randn((R, 3), generator=torch.Generator().manual_seed(43)).to(DEV)
    r_dens, r_feat = torch.zeros_like(dens), torch.zeros_like(feat)
    ws = ops.Workspace()

    def render(repack):
        if repack:
            ws.invalidate()
        ops.render_fwd_into(spec, params, dens, feat, ro, rd, None, *outs, ws, RNG)
        ops.render_bwd_into(spec, params, dens, feat, ro, rd, None, outs[0], outs[1], outs[2], g_colour, None, None, r_dens, r_feat,
                            ws, RNG)

    t_loss = _median_ms(lambda: distortion(False), iters)
    t_grad = _median_ms(lambda: distortion(True), iters)
    by_lanes = {}
    for lanes in (1, 2, 4, 8):
        assert L.voxe_distortion_debug_lanes(lanes) == 0
        by_lanes[str(lanes)] = round(_median_ms(lambda: distortion(True), iters), 4)
    assert L.voxe_distortion_debug_lanes(0) == 0
    t_render = _median_ms(lambda: render(False), iters)
    t_render_step = _median_ms(lambda: render(True), iters)
    t_n = _median_ms(normals, iters)
    return {"rays": R, "distortion_loss_ms": round(t_loss, 4), "distortion_loss_grad_ms": round(t_grad, 4),
            "loss_grad_ms_by_lanes": by_lanes, "render_fwd_bwd_ms": round(t_render, 4),
            "render_fwd_bwd_repacked_ms": round(t_render_step, 4), "normals_ms": round(t_n, 4),
            "loss_grad_over_render": round(t_grad / t_render, 3), "loss_grad_over_render_repacked": round(t_grad / t_render_step, 3),
            "loss_over_normals": round(t_loss / t_n, 3), "loss": round(float(loss), 6),
            "voxels_with_gradient": int((d_d != 0).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distortion_bench.txt"))
    a = ap.parse_args()
    spec = ops.GridSpec(aabb=((-1.5, 1.5),) * 3, density_scale=100.0 / 3.0, density_pre_act=abi.ACT_IDENTITY,
                        density_post_act=abi.ACT_SOFTPLUS)
    d, f = workload.random_grid(160)
    dens, feat = d.to(DEV).contiguous(), f.to(DEV).contiguous()
    lines = []
    ro, rd = _rays(400, [3])
    lines.append({"case": "random160_400x400_S256_image", **case_times(spec, dens, feat, ro, rd, 256, 400, a.iters)})
    print(json.dumps(lines[-1]), flush=True)
    ro, rd = _rays(400, [3 + 12 * j for j in range(8)])
    pick = torch.randperm(ro.shape[0], generator=torch.Generator().manual_seed(11))[:32768].to(DEV)
    ro, rd = ro[pick].contiguous(), rd[pick].contiguous()
    lines.append({"case": "random160_batch32768_of_8cams_S256_linear", **case_times(spec, dens, feat, ro, rd, 256, 0, a.iters)})
    print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
