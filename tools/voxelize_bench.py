#!/usr/bin/env python3
"""Mesh import timings: median device time (HIP events, warmed, outputs and scratch pre-allocated) of 20
voxe_voxelize_mesh calls into a 160^3 lattice at a band of two voxels, for
    sphere    the marching-cubes mesh of the 160^3 sphere (about 87 k small triangles)
    box       a 12-triangle box spanning the lattice (few triangles, each cut into many work items)
    shuffled  the sphere mesh with its faces in random order (neighbouring waves no longer work on neighbouring cells)
next to voxe_mesh_count + voxe_mesh_emit on the same grid, and to the time the key grid (8 B per voxel, written by the init pass,
read by the finalise pass) and the counter grid (4 B per voxel, written, then read and written by the column pass, then read)
take to stream at 8 TB/s -- a floor for the passes that touch every voxel, not a bound on the work pass.

    python tools/voxelize_bench.py [--iters 20] [--side 160] [--out profiles/voxelize_bench.txt]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "vox-e_amd"), os.path.join(ROOT, "tests")]

from voxe_hip import abi, ops  # noqa: E402
from voxe_hip.desc import make_grid_desc  # noqa: E402

PEAK = 8e12
AABB = ((-1.0, 1.0),) * 3


def median_ms(once, iters):
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
    return sorted(times)[len(times) // 2], min(times), max(times)


def box(side):
    import voxelize_ref

    edge = 1.0 - 2.5 / side       # (the faces 2.5 voxels inside the lattice: the whole band is on it)
    return voxelize_ref.box_mesh((-edge,) * 3, (edge,) * 3, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--side", type=int, default=160)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxelize_bench.txt"))
    a = ap.parse_args()
    import mesh_ref

    dev = torch.device("cuda:0")
    n = a.side
    L = ops.lib()
    st = torch.cuda.current_stream().cuda_stream
    spec = ops.GridSpec(aabb=AABB, density_post_act=abi.ACT_IDENTITY)
    dens = torch.from_numpy(mesh_ref.sphere_field(n, 1.2))[..., None].to(dev).contiguous()
    lines = [f"mesh import into a {n}^3 lattice over [-1, 1]^3, band 2 voxels; median (min .. max) device ms of {a.iters} calls"]

    # the export on the same grid, for scale
    sv, sf = ops.extract_mesh(spec, dens, 0.5)
    g = make_grid_desc(dens.data_ptr(), dens.data_ptr(), (n, n, n), 1, AABB, 1.0, abi.ACT_IDENTITY, abi.ACT_IDENTITY)
    nb = L.voxe_mesh_scratch_bytes(n, n, n)
    msc = torch.empty(nb, dtype=torch.uint8, device=dev)
    tot = torch.empty(2, dtype=torch.int64, device=dev)

    def export_once():
        assert L.voxe_mesh_count(C.byref(g), 0.5, None, tot.data_ptr(), msc.data_ptr(), nb, st) == 0
        assert L.voxe_mesh_emit(C.byref(g), 0.5, None, sv.data_ptr(), len(sv), sf.data_ptr(), len(sf), msc.data_ptr(), nb, st) == 0

    med, lo_, hi_ = median_ms(export_once, a.iters)
    lines.append(f"voxe_mesh_count + voxe_mesh_emit (V {len(sv)}, T {len(sf)}): {med:.4f} ({lo_:.4f} .. {hi_:.4f})")

    perm = torch.from_numpy(np.random.default_rng(0).permutation(len(sf))).to(dev)
    bv, bf = box(n)
    inputs = {"sphere": (sv, sf), "box": (torch.from_numpy(bv).to(dev), torch.from_numpy(bf).to(dev)), "shuffled": (sv, sf[perm].contiguous())}
    N = n ** 3
    h = 2.0 * 2.0 / n
    lo, hi = (C.c_float * 3)(-1, -1, -1), (C.c_float * 3)(1, 1, 1)
    sdf = torch.empty(N, dtype=torch.float32, device=dev)
    nearest = torch.empty(N, dtype=torch.int32, device=dev)
    cols = torch.empty(3 * N, dtype=torch.float32, device=dev)
    inside = torch.empty(N, dtype=torch.uint8, device=dev)
    stats = torch.empty(4, dtype=torch.int64, device=dev)
    result = {}
    for name, (v, f) in inputs.items():
        v, f = v.contiguous(), f.contiguous()
        c = ((v + 1.0) / 2.0).clamp(0, 1).contiguous()
        need = L.voxe_voxelize_scratch_bytes(n, n, n, len(f))
        sc = torch.empty(need, dtype=torch.uint8, device=dev)

        def once():
            assert L.voxe_voxelize_mesh(v.data_ptr(), len(v), f.data_ptr(), len(f), c.data_ptr(), n, n, n, lo, hi, h, sdf.data_ptr(),
                                        nearest.data_ptr(), cols.data_ptr(), inside.data_ptr(), stats.data_ptr(), sc.data_ptr(), need,
                                        st) == 0

        med, lo_, hi_ = median_ms(once, a.iters)
        s = [int(x) for x in stats.cpu()]
        result[name] = (med, sdf.clone(), inside.clone())
        lines.append(f"voxe_voxelize_mesh {name:8s} (V {len(v)}, T {len(f)}; odd columns {s[0]}, malformed {s[1]}, band voxels {s[2]}, "
                     f"work items {s[3]}; scratch {need / 2 ** 20:.1f} MiB): {med:.4f} ({lo_:.4f} .. {hi_:.4f})")
    same = torch.equal(result["sphere"][1], result["shuffled"][1]) and torch.equal(result["sphere"][2], result["shuffled"][2])
    lines.append(f"sphere and shuffled: sdf and inside bit-identical: {same}")
    stream_bytes = N * 8 * 2 + N * 4 * 4
    lines.append(f"key grid written + read, counter grid written + read + written + read: {stream_bytes / 2 ** 20:.1f} MiB, "
                 f"{stream_bytes / PEAK * 1e3:.4f} ms at 8 TB/s")
    if result["box"][0] > result["sphere"][0]:
        lines.append(f"NOTE: the 12-triangle box costs more than the {len(sf)}-triangle sphere: the work split is not doing its job")
    else:
        lines.append("the 12-triangle box costs less than the sphere mesh: the work split spreads large triangles over the waves")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
