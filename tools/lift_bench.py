#!/usr/bin/env python3
"""Lifting timings: device time (HIP events, median over --iters rounds after warm-up; the variants take
turns inside every round, in one process) of voxe_lift_accumulate at C = 1 and C = 3 in both merge modes
(voxe_lift_debug_merge: one atomic per lane, corner and channel / contributions to the same cell summed inside the wave first),
next to voxe_visibility_accumulate of the same rays (the same march, atomic max in place of the adds) and to a torch restatement
(ops.sample_probe plus index_add_), on the bench's 160^3 random grid with S = 256:
  (a) one 400 x 400 camera, image order;
  (b) the trainer's 32 768 shuffled rays over 8 cameras, linear order;
  (c) the worst case for contention: 32 768 copies of one ray, every lane of every wave in the same cell at every step.
Every call accumulates into buffers that are zeroed outside the timed window.  "added_GBps" is 8 bytes per non-zero contribution
(counted from the restatement's own samples) over the per-lane variant's time: the rate of 8-byte integer global atomics as this
kernel issues them, next to the guide's chip-wide float-atomic rate of about 1300 GB/s (256 contiguous bytes per
wave-instruction; 64 lanes in 64 rows: about 80 GB/s).  One JSON line per case, also written to --out.  --pytest_log: a log of
tests/test_lift_gpu.py run with -s; its largest error / budget ratio is recorded too.  Exit status 1 when the shipped mode is
slower than the torch restatement in any case.

    python tools/lift_bench.py [--iters 15] [--out profiles/lift_bench.txt] [--pytest_log LOG]
"""
import argparse
import json
import os
import re
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "vox-e_amd")]

from thre3d_atom.utils.imaging_utils import pose_spherical  # noqa: E402
from voxe_hip import abi, ops, workload  # noqa: E402
from voxe_hip.desc import norm_constants  # noqa: E402

DEV = torch.device("cuda:0")
RNG = (42, 7)
GUIDE_FLOAT_ATOMIC_GBPS = 1300.0


def _rays(hw, cams):
    rays = [ops.cast_rays(hw, hw, workload.focal_for(hw), *pose_spherical(*workload.synth_pose_angles(cam, 100), workload.RADIUS), DEV)
            for cam in cams]
    return torch.cat([r[0] for r in rays]).contiguous(), torch.cat([r[1] for r in rays]).contiguous()


def torch_lift(spec, params, dens, feat, ro, rd, values, sum_wv, sum_w, count=False):
    """the restatement in float32 torch ops: the forward's samples from ops.sample_probe, weights by cumprod, index_add_ per
    corner.  `count`: also return the number of non-zero quantised contributions to (sum_w, sum_wv)"""
    X, Y, Z = (int(n) for n in dens.shape[:3])
    probe = ops.sample_probe(spec, params, dens, feat, ro, rd, None, rng=RNG, outputs=("z", "inside", "sigma"))
    z, inside, sigma = probe["z"], probe["inside"], probe["sigma"]
    R, S = z.shape
    dnorm = rd.norm(dim=1)
    dl = torch.cat([z[:, 1:] - z[:, :-1], torch.full((R, 1), 1e10, device=DEV)], dim=1)
    alpha = 1.0 - torch.exp(-sigma * (dl * dnorm[:, None]))
    T = torch.cumprod(torch.cat([torch.ones((R, 1), device=DEV), 1.0 - alpha[:, :-1]], dim=1), dim=1)
    keep = (inside & (alpha * T > 0)).reshape(-1).nonzero()[:, 0]          # the samples that deposit
    w = (alpha * T).reshape(-1)[keep]
    ray = keep // S
    p = ro[ray] + rd[ray] * z.reshape(-1)[keep][:, None]
    scale, bias = norm_constants(spec.aabb)
    u = torch.stack([((p[:, a] * float(scale[a]) + float(bias[a]) + 1.0) * float((X, Y, Z)[a]) - 1.0) * 0.5 for a in range(3)], dim=1)
    fl = torch.floor(u)
    i0 = fl.long()
    ax = torch.stack([(fl + 1.0) - u, u - fl], dim=-1)
    v = values[ray]
    n_w = n_wv = 0
    for dx in range(2):
        for dy in range(2):
            for dz in range(2):
                i, j, k = i0[:, 0] + dx, i0[:, 1] + dy, i0[:, 2] + dz
                ok = (i >= 0) & (i < X) & (j >= 0) & (j < Y) & (k >= 0) & (k < Z)
                a = torch.where(ok, w * ((ax[:, 0, dx] * ax[:, 1, dy]) * ax[:, 2, dz]), torch.zeros_like(w))
                flat = (i.clamp(0, X - 1) * Y + j.clamp(0, Y - 1)) * Z + k.clamp(0, Z - 1)
                sum_w.view(-1).index_add_(0, flat, a)
                sum_wv.view(-1, v.shape[1]).index_add_(0, flat, a[:, None] * v)
                if count:
                    n_w += int((torch.round(a.double() * 2.0 ** 32) != 0).sum())
                    n_wv += int((torch.round((a[:, None] * v).double() * 2.0 ** 32) != 0).sum())
    return n_w, n_wv


def case_times(spec, dens, feat, ro, rd, S, width, iters, perturb=True):
    R = ro.shape[0]
    dims = tuple(int(n) for n in dens.shape[:3])
    params = ops.RenderParams(num_samples=S, near=workload.NEAR, far=workload.FAR, perturb=perturb, image_width=width)
    out = {"rays": R}
    mw = torch.zeros(dims, device=DEV)
    variants = {"visibility_max_weight": lambda: ops.visibility_accumulate_(spec, params, dens, ro, rd, mw, None, rng=RNG)}
    clears = [mw]
    sums = {}
    for C in (1, 3):
        values = torch.empty((R, C)).uniform_(-1, 1, generator=torch.Generator().manual_seed(5 + C)).to(DEV)
        f_wv, f_w = torch.zeros((*dims, C), device=DEV), torch.zeros(dims, device=DEV)
        n_w, n_wv = torch_lift(spec, params, dens, feat, ro, rd, values, f_wv, f_w, count=True)
        out[f"C{C}_contributions"] = n_w + n_wv
        variants[f"C{C}_torch"] = (lambda values=values, f_wv=f_wv, f_w=f_w:
                                   torch_lift(spec, params, dens, feat, ro, rd, values, f_wv, f_w))
        clears += [f_wv, f_w]
        for name, mode in (("per_lane", ops.LIFT_MERGE_PER_LANE), ("wave_merge", ops.LIFT_MERGE_WAVE), ("shipped", ops.LIFT_MERGE_SHIPPED)):
            swv, sw = torch.zeros((*dims, C), dtype=torch.int64, device=DEV), torch.zeros(dims, dtype=torch.int64, device=DEV)

            def run(values=values, swv=swv, sw=sw, mode=mode):
                ops.lift_debug_merge(mode)
                ops.lift_accumulate_(spec, params, dens, ro, rd, values, swv, sw, rng=RNG)

            variants[f"C{C}_{name}"] = run
            clears += [swv, sw]
            sums[(C, name)] = (swv, sw, f_w)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {k: [] for k in variants}
    for i in range(iters + 3):           # three warm-up rounds; the variants alternate inside every round
        for t in clears:
            t.zero_()
        for name, fn in variants.items():
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= 3:
                times[name].append(e0.elapsed_time(e1))
    ops.lift_debug_merge(ops.LIFT_MERGE_SHIPPED)
    for name, ts in times.items():
        out[f"{name}_ms"] = round(sorted(ts)[len(ts) // 2], 4)
    for C in (1, 3):      # faster and different is not faster: both modes hold the same bits, and they are the restatement's sums
        a, b, s = sums[(C, "per_lane")], sums[(C, "wave_merge")], sums[(C, "shipped")]
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[0], s[0]) and torch.equal(a[1], s[1])
        out[f"C{C}_max_abs_diff_to_torch"] = float((a[1].double() / 2.0 ** 32 - a[2].double()).abs().max())   # (the last round's call)
        out[f"C{C}_max_weight"] = float(a[2].max())
        out[f"C{C}_added_GBps_per_lane"] = round(8.0 * out[f"C{C}_contributions"] / (out[f"C{C}_per_lane_ms"] * 1e-3) / 1e9, 2)
        out[f"C{C}_merge_over_per_lane"] = round(out[f"C{C}_wave_merge_ms"] / out[f"C{C}_per_lane_ms"], 3)
        out[f"C{C}_shipped_over_torch"] = round(out[f"C{C}_shipped_ms"] / out[f"C{C}_torch_ms"], 4)
    out["guide_float_atomic_GBps"] = GUIDE_FLOAT_ATOMIC_GBPS
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lift_bench.txt"))
    ap.add_argument("--pytest_log", default=None)
    a = ap.parse_args()
    spec = ops.GridSpec(aabb=((-1.5, 1.5),) * 3, density_scale=100.0 / 3.0, density_pre_act=abi.ACT_IDENTITY,
                        density_post_act=abi.ACT_SOFTPLUS)
    d, f = workload.random_grid(160)
    dens, feat = d.to(DEV).contiguous(), f.to(DEV).contiguous()
    lines = []

    def case(name, ro, rd, width, perturb=True):
        lines.append({"case": name, **case_times(spec, dens, feat, ro, rd, 256, width, a.iters, perturb)})
        print(json.dumps(lines[-1]), flush=True)

    ro, rd = _rays(400, [3])
    case("random160_400x400_S256_image", ro, rd, 400)
    centre = (ro[200 * 400 + 200][None].expand(32768, 3).contiguous(), rd[200 * 400 + 200][None].expand(32768, 3).contiguous())
    ro, rd = _rays(400, [3 + 12 * j for j in range(8)])
    pick = torch.randperm(ro.shape[0], generator=torch.Generator().manual_seed(11))[:32768].to(DEV)
    case("random160_batch32768_of_8cams_S256_shuffled", ro[pick].contiguous(), rd[pick].contiguous(), 0)
    case("random160_32768_copies_of_one_ray_S256_no_jitter", *centre, 0, perturb=False)   # (hashed jitter differs from ray to ray)
    if a.pytest_log:
        ratios = [max(float(m.group(1)), float(m.group(2))) for m in
                  re.finditer(r"LIFT_RATIO .*?sum_w ([0-9.eE+-]+)\s+sum_wv ([0-9.eE+-]+) of the budget", open(a.pytest_log).read())]
        lines.append({"case": "tests/test_lift_gpu.py agreement", "cases": len(ratios),
                      "largest_error_over_budget": max(ratios) if ratios else None})
        print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")
    lost = [(line["case"], C) for line in lines if "rays" in line for C in (1, 3) if line[f"C{C}_shipped_over_torch"] > 1.0]
    if lost:
        print(f"the shipped lift is slower than the torch restatement: {lost}", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
