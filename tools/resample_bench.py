#!/usr/bin/env python3
"""Grid-transform timings: device time (HIP events, median of --iters calls after warm-up) of
voxe_grid_resample under a generic rotation onto the source's own lattice, on 160^3 SH-0, 160^3 SH-2 and 200^3 SH-3 grids, next to

  (a) the streaming bound of the shapes: (1 + C) * 4 bytes read and as many written per voxel, at 8 TB/s;
  (b) a PyTorch restatement on the same GPU in the same process: permute to channels-first -> F.grid_sample (trilinear, zero
      padding, the sampling grid precomputed outside the timed span) -> permute back -> one einsum per SH band.  The two are
      timed alternately, call by call.

One JSON line per case, written to --out as well.  Exit status 1 when the kernel is slower than (b) on any case: (b) makes at
least three more passes over the grid, so no margin is asked for.

    python tools/resample_bench.py [--iters 20] [--out profiles/resample_bench.txt]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "vox-e_amd")]

from thre3d_atom.thre3d_reprs.transform import sh_rotation_matrices  # noqa: E402
from voxe_hip import abi, ops  # noqa: E402

DEV = torch.device("cuda:0")
HBM_BYTES_PER_S = 8.0e12
CASES = [("160^3 SH-0", 160, 0), ("160^3 SH-2", 160, 2), ("200^3 SH-3", 200, 3)]


def _rotation():
    def about(a, deg):
        i, j, c, s = (a + 1) % 3, (a + 2) % 3, np.cos(np.radians(deg)), np.sin(np.radians(deg))
        R = np.eye(3)
        R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
        return R
    return about(2, 31.0) @ about(0, -17.0) @ about(1, 52.0)


def _timed(fn, e0, e1):
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def run_case(name, side, degree, iters):
    C = 3 * (degree + 1) ** 2
    g = torch.Generator().manual_seed(side + degree)
    dens = torch.rand((side, side, side, 1), generator=g).to(DEV)
    feat = torch.randn((side, side, side, C), generator=g).to(DEV)
    R = _rotation()
    # the source's own lattice, rotated about the grid centre: u = R^T (i - c) + c
    centre = (side - 1) / 2.0
    A, b = R.T, centre - R.T @ np.full(3, centre)
    blocks = sh_rotation_matrices(R, degree)
    xf = ops.make_resample(A, b, blocks, degree, abi.ACT_IDENTITY, 0.0, abi.RESAMPLE_REPLACE)
    out_d, out_f = torch.empty_like(dens), torch.empty_like(feat)
    L, st = ops.lib(), torch.cuda.current_stream().cuda_stream

    def kernel():
        assert L.voxe_grid_resample(dens.data_ptr(), feat.data_ptr(), side, side, side, C, out_d.data_ptr(), out_f.data_ptr(), side,
                                    side, side, ctypes.byref(xf), None, st) == 0

    # the restatement's sampling grid: u in grid_sample's (x = last axis, y, z = first axis) order, align_corners=True
    idx = torch.stack(torch.meshgrid(*(torch.arange(side, dtype=torch.float64),) * 3, indexing="ij"), dim=-1)
    u = idx @ torch.from_numpy(A).T + torch.from_numpy(b)
    grid = (2.0 * u / (side - 1) - 1.0).flip(-1).float()[None].to(DEV)
    mats = [torch.from_numpy(m).float().to(DEV) for m in blocks]
    held = {}

    def restatement():
        vol = torch.cat([dens, feat], dim=-1).permute(3, 0, 1, 2)[None]
        smp = F.grid_sample(vol, grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0].permute(1, 2, 3, 0)
        c = smp[..., 1:].reshape(side, side, side, 3, -1)
        bands = [c[..., :1]] + [torch.einsum("jk,...k->...j", mats[l], c[..., l * l:(l + 1) ** 2]) for l in range(1, degree + 1)]
        held["d"], held["f"] = smp[..., :1].contiguous(), torch.cat(bands, dim=-1).reshape(side, side, side, C)

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t_k, t_r = [], []
    for i in range(iters + 3):
        a, r = _timed(kernel, e0, e1), _timed(restatement, e0, e1)
        if i >= 3:
            t_k.append(a)
            t_r.append(r)
    t_k, t_r = sorted(t_k)[len(t_k) // 2], sorted(t_r)[len(t_r) // 2]
    # the two compute the same thing (float32 both: agreement to rounding of the index arithmetic)
    err = max(float((out_d - held["d"]).abs().max()), float((out_f - held["f"]).abs().max()))
    bound_ms = 2.0 * (1 + C) * 4 * side ** 3 / HBM_BYTES_PER_S * 1e3
    return {"case": name, "channels": C, "kernel_ms": round(t_k, 4), "torch_restatement_ms": round(t_r, 4),
            "streaming_bound_ms": round(bound_ms, 4), "kernel_over_bound": round(t_k / bound_ms, 2),
            "restatement_over_kernel": round(t_r / t_k, 2), "max_abs_difference": float(f"{err:.3e}")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_bench.txt"))
    a = ap.parse_args()
    lines, ok = [], True
    for name, side, degree in CASES:
        res = run_case(name, side, degree, a.iters)
        ok = ok and res["kernel_ms"] <= res["torch_restatement_ms"]
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    with open(a.out, "w") as fh:
        fh.write(f"# tools/resample_bench.py --iters {a.iters}: voxe_grid_resample vs streaming bound vs PyTorch restatement "
                 f"({torch.cuda.get_device_name(0)})\n" + "\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
