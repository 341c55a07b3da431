#!/usr/bin/env python3
"""Mesh export timings: device time of voxe_mesh_count + voxe_mesh_emit (HIP events, warmed, outputs
pre-allocated) and wall time of the whole ops.extract_mesh call (one host read-back, allocations included), for the sphere
and the random grid at 160^3 and 256^3.  Bytes: densities read by the count and vertex passes, per-node scratch
(case byte, vertex / triangle bases) written and read, vertices and faces written; against 8 TB/s.

    python tools/mesh_bench.py [--iters 20]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "vox-e_amd"), os.path.join(ROOT, "tests")]

from voxe_hip import abi, ops, workload  # noqa: E402
from voxe_hip.desc import make_grid_desc  # noqa: E402

PEAK = 8e12


def sphere(side):
    import mesh_ref

    return torch.from_numpy(mesh_ref.sphere_field(side, 1.2))[..., None]


def run(name, dens, spec, level, iters):
    dev = torch.device("cuda:0")
    d = dens.to(dev).contiguous()
    X, Y, Z = d.shape[:3]
    L = ops.lib()
    g = make_grid_desc(d.data_ptr(), d.data_ptr(), (X, Y, Z), 1, spec.aabb, spec.density_scale, spec.density_pre_act,
                       spec.density_post_act)
    v, f = ops.extract_mesh(spec, d, level)      # sizes + warm-up
    V, T = len(v), len(f)
    nb = L.voxe_mesh_scratch_bytes(X, Y, Z)
    sc = torch.empty(nb, dtype=torch.uint8, device=dev)
    tot = torch.empty(2, dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def once():
        assert L.voxe_mesh_count(ctypes.byref(g), level, None, tot.data_ptr(), sc.data_ptr(), nb, st) == 0
        assert L.voxe_mesh_emit(ctypes.byref(g), level, None, v.data_ptr(), V, f.data_ptr(), T, sc.data_ptr(), nb, st) == 0

    for _ in range(3):
        once()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(iters):
        e0.record()
        once()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    walls = []
    for _ in range(max(3, iters // 4)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ops.extract_mesh(spec, d, level)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    M = (X + 2) * (Y + 2) * (Z + 2)
    nbytes = 2 * X * Y * Z * 4 + M * (1 + 1 + 4 + 4 + 1 + 4 + 4) + V * 12 + T * 12
    dev_ms = sorted(times)[len(times) // 2]
    return {"case": name, "dims": [X, Y, Z], "V": V, "T": T, "device_ms": round(dev_ms, 4),
            "extract_mesh_ms": round(sorted(walls)[len(walls) // 2], 3), "bytes": nbytes,
            "frac_of_8TBps": round(nbytes / (dev_ms * 1e-3) / PEAK, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    sph = ops.GridSpec(aabb=((-1.0, 1.0),) * 3, density_post_act=abi.ACT_IDENTITY)
    rnd = ops.GridSpec(aabb=((-1.5, 1.5),) * 3, density_pre_act=abi.ACT_ABS, density_post_act=abi.ACT_IDENTITY)
    for side in (160, 256):
        print(json.dumps(run(f"sphere{side}", sphere(side), sph, 0.5, a.iters)), flush=True)
        print(json.dumps(run(f"random{side}", workload.random_grid(side, nfeat=1)[0], rnd, 0.5, a.iters)), flush=True)


if __name__ == "__main__":
    main()
