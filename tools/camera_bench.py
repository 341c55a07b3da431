#!/usr/bin/env python3
"""Device time of voxe_cast_rays_camera (without / with lens distortion) and voxe_cast_rays_camera_bwd against
voxe_cast_rays_indexed / voxe_cast_rays_bwd of the same library, in one process, runs alternating (A B A B ...), for one
400 x 400 image and the trainer's 32 768-ray batch over 8 cameras.

    python tools/camera_bench.py [--rounds 20] [--inner 50] > profiles/camera_bench.txt

Each figure is the median over `rounds` of (event time of `inner` back-to-back calls) / inner, after a warm-up."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vox-e_amd"))

from thre3d_atom.utils.imaging_utils import PinholeCamera, pose_spherical  # noqa: E402
from voxe_hip import ops, workload  # noqa: E402

DEV = torch.device("cuda:0")
DIST = (-0.12, 0.03, 0.002, -0.001, 0.0)


def timed(fn, inner):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / inner   # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--inner", type=int, default=50)
    args = ap.parse_args()
    hw = 400
    focal = workload.focal_for(hw)
    plain = PinholeCamera(hw, hw, focal, focal * 0.97, hw * 0.5 + 3.3, hw * 0.5 - 2.1)
    lens = PinholeCamera(hw, hw, focal, focal * 0.97, hw * 0.5 + 3.3, hw * 0.5 - 2.1, DIST).validate()
    poses = torch.stack([torch.cat(pose_spherical(*workload.synth_pose_angles(i + 1, 8), workload.RADIUS), dim=1) for i in range(8)]).to(DEV)
    print(f"# {torch.cuda.get_device_name(0)}; us per call, median of {args.rounds} rounds of {args.inner} calls, alternating")
    for tag, p, idx in (("one 400 x 400 image", poses[:1].contiguous(), torch.arange(hw * hw, device=DEV)),
                        ("32768-ray batch over 8 cameras", poses, ops.random_subset(8 * hw * hw, 32768, DEV, rng=(1, 2)))):
        B = int(idx.shape[0])
        g_o, g_d = torch.randn((B, 3), device=DEV), torch.randn((B, 3), device=DEV)
        calls = {
            "cast_rays_indexed": lambda: ops.cast_rays_indexed(hw, hw, focal, p, idx),
            "cast_rays_camera": lambda: ops.cast_rays_camera(plain, p, idx),
            "cast_rays_camera + lens": lambda: ops.cast_rays_camera(lens, p, idx),
            "cast_rays_bwd (poses, focal)": lambda: ops.cast_rays_bwd(hw, hw, focal, p, idx, g_o, g_d, want_focal=True),
            "cast_rays_camera_bwd (poses, intrinsics)": lambda: ops.cast_rays_camera_bwd(plain, p, idx, g_o, g_d, want_intrinsics=True),
            "cast_rays_camera_bwd + lens (all)": lambda: ops.cast_rays_camera_bwd(lens, p, idx, g_o, g_d, want_intrinsics=True,
                                                                                  want_distortion=True),
        }
        for fn in calls.values():
            timed(fn, 10)
        times = {k: [] for k in calls}
        for _ in range(args.rounds):
            for k, fn in calls.items():
                times[k].append(timed(fn, args.inner))
        print(f"{tag} (B = {B})")
        base_f, base_b = statistics.median(times["cast_rays_indexed"]), statistics.median(times["cast_rays_bwd (poses, focal)"])
        for k, v in times.items():
            m = statistics.median(v)
            print(f"  {k:44s} {m:8.2f} us  ({m / (base_b if 'bwd' in k else base_f):.2f} x legacy; min {min(v):.2f} max {max(v):.2f})")


if __name__ == "__main__":
    main()
