"""List-scheduler model of a launch of the lean tile kernels, numpy only, seconds on a CPU.

A launch is one one-wave block per (8x8-pixel tile, 32-sample depth segment); block b goes to XCD b mod 8 and onto the first
free wave slot there (384 slots per XCD for the backward at 3 waves per SIMD, 640 for the forward at 5).  A block costs its
prologue plus one unit per wave iteration = the in-volume sample span of the tile's 64 rays inside the segment (slab test on the
bench's own cameras); a block without a sample costs `--empty`.  The model prints, per kernel, the idle share of the wave slots
in launch order (segment-major, tile-minor) and the make-span of other orders of the same blocks relative to it:

    python tools/schedule_model.py                       # the 20 bench cameras, 400x400, S = 256
    python tools/schedule_model.py --cameras 3 38 88 --prologue 2 5 10

Orders: `b<w>` buckets of w iterations, longest bucket first, launch order inside a bucket, empty blocks last (what
tile_sched_sort_kernel builds; the library ships w = 4); `lpt` fully sorted, longest first.  What the model cannot know is how
much faster the surviving waves of a draining SIMD run; profiles/*_sched.txt holds the measurement."""
import argparse
import heapq
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vox-e_amd"))
from thre3d_atom.utils.imaging_utils import pose_spherical  # noqa: E402
from voxe_hip.workload import FAR, NEAR, RADIUS, focal_for, synth_pose_angles  # noqa: E402

SEG = 32
HALF = 1.5     # the bench's AABB


def iterations(cam, hw, samples):
    """wave iterations of every (segment, tile) of camera `cam`, segment-major; mean in-volume samples per ray"""
    yaw, pitch = synth_pose_angles(cam, 100)
    p = pose_spherical(yaw, pitch, RADIUS)
    rot = np.asarray(p.rotation, dtype=np.float64)
    t = np.asarray(p.translation, dtype=np.float64).reshape(3)
    f = focal_for(hw)
    ys, xs = np.meshgrid(np.arange(hw) + 0.5, np.arange(hw) + 0.5, indexing="ij")
    d = np.stack([(xs - hw / 2) / f, -(ys - hw / 2) / f, -np.ones_like(xs)], -1) @ rot.T
    z = np.linspace(NEAR, FAR, samples)
    with np.errstate(divide="ignore"):
        t0, t1 = (-HALF - t) / d, (HALF - t) / d
    lo, hi = np.minimum(t0, t1).max(-1), np.maximum(t0, t1).min(-1)
    klo = np.searchsorted(z, lo.ravel(), "left").reshape(hw, hw)
    khi = (np.searchsorted(z, hi.ravel(), "right") - 1).reshape(hw, hw)
    hit = khi >= klo
    nt = (hw + 7) // 8
    pad = lambda v, fill: np.pad(v, ((0, nt * 8 - hw), (0, nt * 8 - hw)), constant_values=fill)
    nseg = (samples + SEG - 1) // SEG
    it = np.zeros((nseg, nt, nt), int)
    for s in range(nseg):
        a = pad(np.where(hit, np.maximum(klo, s * SEG), 10 ** 6), 10 ** 6).reshape(nt, 8, nt, 8).min((1, 3))
        b = pad(np.where(hit, np.minimum(khi, s * SEG + SEG - 1), -10 ** 6), -10 ** 6).reshape(nt, 8, nt, 8).max((1, 3))
        it[s] = np.clip(b - a + 1, 0, SEG)
    return it.reshape(-1), float((np.clip(khi - klo + 1, 0, None) * hit).mean())


def makespan(costs, slots_per_xcd):
    """block b on XCD b mod 8, greedily onto that XCD's earliest free slot"""
    end = 0.0
    for x in range(8):
        h = [0.0] * slots_per_xcd
        for c in costs[x::8]:
            heapq.heappush(h, heapq.heappop(h) + c)
        end = max(end, max(h))
    return end


def bucketed(cost, its, width):
    return cost[np.argsort(-np.ceil(its / width).astype(int), kind="stable")]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cameras", type=int, nargs="*", default=list(range(3, 100, 5)))
    ap.add_argument("--image", type=int, default=400)
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--prologue", type=float, nargs="*", default=None, help="iteration-equivalents (default: 4.4 backward, 2.2 forward: profiles/tile_plan.txt)")
    ap.add_argument("--empty", type=float, default=0.5)
    ap.add_argument("--widths", type=int, nargs="*", default=[4, 8, 16])
    args = ap.parse_args()
    its = {cam: iterations(cam, args.image, args.samples) for cam in args.cameras}
    for cam, (flat, mean_in) in its.items():
        print(f"camera {cam}: {mean_in:.1f} in-volume samples per ray, {int((flat > 0).sum())} of {flat.size} blocks with samples")
    for name, slots, pro_default in (("backward", 384, 4.4), ("forward", 640, 2.2)):
        for pro in (args.prologue or [pro_default]):
            out = {}
            for flat, _ in its.values():
                cost = np.where(flat > 0, pro + flat, args.empty).astype(float)
                now = makespan(cost, slots)
                out.setdefault("idle", []).append(1 - cost.sum() / (8 * slots) / now)
                for w in args.widths:
                    out.setdefault(f"b{w}", []).append(makespan(bucketed(cost, flat, w), slots) / now)
                out.setdefault("lpt", []).append(makespan(np.sort(cost)[::-1], slots) / now)
            print(f"{name} ({slots} slots per XCD, prologue {pro}, empty {args.empty}): " +
                  "  ".join(f"{k} {np.mean(v):.3f} ({np.min(v):.3f} - {np.max(v):.3f})" for k, v in out.items()))


if __name__ == "__main__":
    main()
