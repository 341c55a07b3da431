#!/usr/bin/env python3
"""Visibility timings: device time (HIP events, median of --iters calls after warm-up) of
voxe_visibility_accumulate next to voxe_render_normals on the same rays, cfg and jitter stream, on the bench's 160^3 grids
(random, and the sphere as an opaque scene) at 400x400 with S = 256: one camera, and the headline's 20 cameras (3, 8, ..., 98 of
the 100-view set) as one multi-view launch.  Two accumulate figures per case: "cold" clears both grids before every call (the
clears are outside the timed span), so every first touch of a voxel is an atomic; "steady" accumulates onto the grids the same
rays already filled, so the plain load in front of each atomic skips all of them.  The mask pass (dilate 1) is timed on the
result.  One JSON line per case.

    python tools/visibility_bench.py [--iters 20]
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


def _median_ms(fn, iters, before=None):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for i in range(iters + 3):
        if before is not None:
            before()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i >= 3:
            times.append(e0.elapsed_time(e1))
    return sorted(times)[len(times) // 2]


def case_times(spec, dens, hw, S, cams, iters):
    rays = [ops.cast_rays(hw, hw, workload.focal_for(hw), *pose_spherical(*workload.synth_pose_angles(cam, 100), workload.RADIUS), DEV)
            for cam in cams]
    ro, rd = torch.cat([r[0] for r in rays]).contiguous(), torch.cat([r[1] for r in rays]).contiguous()
    R = ro.shape[0]
    dims = tuple(int(n) for n in dens.shape[:3])
    L = ops.lib()
    g = make_grid_desc(dens.data_ptr(), 0, dims, 0, spec.aabb, spec.density_scale, spec.density_pre_act, spec.density_post_act)
    c = make_render_cfg(S, workload.NEAR, workload.FAR, True, seed=RNG[0], rng_offset=RNG[1], image_width=hw,
                        image_height=hw if len(cams) > 1 else None)
    nrm = torch.empty((R, 3), dtype=torch.float32, device=DEV)
    depth, acc = (torch.empty((R, 1), dtype=torch.float32, device=DEV) for _ in range(2))
    mw, mt = (torch.zeros(dims, dtype=torch.float32, device=DEV) for _ in range(2))
    mask = torch.empty(dims, dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    def normals():
        assert L.voxe_render_normals(ctypes.byref(g), ctypes.byref(c), ro.data_ptr(), rd.data_ptr(), R, None, nrm.data_ptr(),
                                     depth.data_ptr(), acc.data_ptr(), st) == 0

    def accumulate():
        assert L.voxe_visibility_accumulate(ctypes.byref(g), ctypes.byref(c), ro.data_ptr(), rd.data_ptr(), R, None,
                                            mw.data_ptr(), mt.data_ptr(), st) == 0

    def clear():
        mw.zero_()
        mt.zero_()

    t_n = _median_ms(normals, iters)
    t_cold = _median_ms(accumulate, iters, before=clear)
    t_steady = _median_ms(accumulate, iters)
    t_mask = _median_ms(lambda: L.voxe_visibility_mask(mw.data_ptr(), *dims, 0.0, 1, mask.data_ptr(), st), iters)
    return {"views": len(cams), "rays": R, "normals_ms": round(t_n, 4), "visibility_cold_ms": round(t_cold, 4),
            "visibility_steady_ms": round(t_steady, 4), "cold_over_normals": round(t_cold / t_n, 3),
            "steady_over_normals": round(t_steady / t_n, 3), "mask_dilate1_ms": round(t_mask, 4),
            "voxels_weighed": int((mw > 0).sum()), "voxels_reached": int((mt > 0).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    spec = ops.GridSpec(aabb=((-1.5, 1.5),) * 3, density_scale=100.0 / 3.0, density_pre_act=abi.ACT_IDENTITY,
                        density_post_act=abi.ACT_SOFTPLUS)
    scenes = {"random": workload.random_grid(160), "sphere": workload.sphere_grid(160)}
    for scene, (d, _) in scenes.items():
        dens = d.to(DEV).contiguous()
        for cams in ([3], [3 + 5 * j for j in range(20)]):
            out = case_times(spec, dens, 400, 256, cams, a.iters)
            print(json.dumps({"case": f"{scene}160_400x400_S256_{len(cams)}cam", **out}), flush=True)


if __name__ == "__main__":
    main()
