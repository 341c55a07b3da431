#!/usr/bin/env python3
"""Normals timings: device time (HIP events, median of --iters calls after warm-up, outputs pre-allocated)
of voxe_render_normals against an inference voxe_render_fwd (ray_state_valid = -1) of the same rays, cfg and jitter stream, on
the bench's 160^3 SH-0 grids (random, and the sphere as an opaque scene) and cameras (synth_pose_angles over the 100-view set):
400x400 with S = 256 over the headline's 20 cameras (3, 8, ..., 98: the oblique 38 / 83 / 88 included), 800x800 with S = 512
(the render tool's defaults) over cameras 3 / 38 / 83 / 88; and voxe_query_normals on 10^6 points.  One JSON line per case.

    python tools/normals_bench.py [--iters 20]
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
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(iters):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return sorted(times)[len(times) // 2]


def view_times(spec, dens, feat, hw, S, cam, iters):
    pose = pose_spherical(*workload.synth_pose_angles(cam, 100), workload.RADIUS)
    ro, rd = ops.cast_rays(hw, hw, workload.focal_for(hw), pose.rotation, pose.translation, DEV)
    R = ro.shape[0]
    params = ops.RenderParams(num_samples=S, near=workload.NEAR, far=workload.FAR, perturb=True, white_bkgd=True, image_width=hw)
    outs = [torch.empty((R, n), dtype=torch.float32, device=DEV) for n in (3, 1, 1, 1)]
    ws = ops.Workspace()

    def fwd():
        ops.render_fwd_into(spec, params, dens, feat, ro, rd, None, *outs, ws, RNG, keep_for_backward=False)

    L = ops.lib()
    g = make_grid_desc(dens.data_ptr(), 0, (dens.shape[0], dens.shape[1], dens.shape[2]), 0, spec.aabb, spec.density_scale,
                       spec.density_pre_act, spec.density_post_act)
    c = make_render_cfg(S, workload.NEAR, workload.FAR, True, seed=RNG[0], rng_offset=RNG[1], image_width=hw)
    nrm = torch.empty((R, 3), dtype=torch.float32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    def normals():
        assert L.voxe_render_normals(ctypes.byref(g), ctypes.byref(c), ro.data_ptr(), rd.data_ptr(), R, None, nrm.data_ptr(),
                                     outs[1].data_ptr(), outs[2].data_ptr(), st) == 0

    return _median_ms(fwd, iters), _median_ms(normals, iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    spec = ops.GridSpec(aabb=((-1.5, 1.5),) * 3, density_scale=100.0 / 3.0, density_pre_act=abi.ACT_IDENTITY,
                        density_post_act=abi.ACT_SOFTPLUS)
    scenes = {"random": workload.random_grid(160), "sphere": workload.sphere_grid(160)}
    for scene, (d, f) in scenes.items():
        dens, feat = d.to(DEV).contiguous(), f.to(DEV).contiguous()
        for hw, S, cams in ((400, 256, [3 + 5 * j for j in range(20)]), (800, 512, [3, 38, 83, 88])):
            per = {cam: view_times(spec, dens, feat, hw, S, cam, a.iters) for cam in cams}
            fwd = sum(t[0] for t in per.values()) / len(per)
            nrm = sum(t[1] for t in per.values()) / len(per)
            print(json.dumps({"case": f"{scene}160_{hw}x{hw}_S{S}", "views": len(per), "fwd_view_mean_ms": round(fwd, 4),
                              "normals_view_mean_ms": round(nrm, 4), "ratio": round(nrm / fwd, 3),
                              "oblique": {cam: [round(per[cam][0], 4), round(per[cam][1], 4)] for cam in (38, 83, 88)}}),
                  flush=True)
        pts = (torch.rand((1000000, 3), generator=torch.Generator().manual_seed(3)) * 3.0 - 1.5).to(DEV)
        out = torch.empty((1000000, 3), dtype=torch.float32, device=DEV)
        L = ops.lib()
        g = make_grid_desc(dens.data_ptr(), 0, (160, 160, 160), 0, spec.aabb, spec.density_scale, spec.density_pre_act,
                           spec.density_post_act)
        st = torch.cuda.current_stream().cuda_stream
        ms = _median_ms(lambda: L.voxe_query_normals(ctypes.byref(g), pts.data_ptr(), 1000000, out.data_ptr(), st), a.iters)
        print(json.dumps({"case": f"{scene}160_query_1e6", "device_ms": round(ms, 4)}), flush=True)


if __name__ == "__main__":
    main()
