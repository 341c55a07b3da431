#!/usr/bin/env python3
"""Bit digests of calls that share the density-only sample march (voxe_ray_march.hpp lists them all):
render_normals, visibility_accumulate_, lift_accumulate_, render_bwd_rays and the three ray losses distortion_fwd_bwd,
depth_fwd_bwd and orientation_fwd_bwd on seeded inputs, one `sha256 name` line per output tensor.  Two trees whose kernels compute the same bits print the same lines, so a change of the
shared march is checked by running this file in both trees and comparing the outputs line for line.

Inputs: a 26 x 20 x 23 grid (identity / softplus, scale 2.0), three ray sets -- (a) 21 x 13 pixels x 3 views in image order with
image_height set (no side a multiple of a tile side), (b) the same rays without image fields, (c) (a)'s rays shuffled -- each at
S = 33 and S = 96 under five depth modes (plain, hash jitter, caller jitter, aabb_clip, linear disparity).  The ray losses and the
ray gradients run at every pinned lanes-per-ray split, lifting in both merge modes with C in {0, 1, 3, 8}; normals add one launch
at 400^2 / 600^2 / 800^2 / 1040^2 pixels (8 / 4 / 2 / 1 lanes per ray).  The depth loss has target depths in [NEAR, FAR] and
widths in [0.02, 0.2]; it and the orientation loss (normal_eps 0 and 1e-2) run with ray weights in [0, 2), every seventh exactly
0, and without.  Only outputs that are bit-stable are digested: a loss's gradient goes through float atomics, so it is taken from
64 single-ray calls at one lane per ray that accumulate on one stream.  The sets (a), (b), (c) are also compared with each other per ray (exit status 1 on a difference).

--fold: FILE gets one line per call and input set, `sha256 name (n tensors)`, the sha256 of that group's per-tensor lines (which
are printed either way).

    python tools/ray_march_digest.py [--out FILE] [--fold]
"""
import argparse
import hashlib
import os
import re
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "vox-e_amd")]

from thre3d_atom.utils.imaging_utils import pose_spherical  # noqa: E402
from voxe_hip import abi, ops, workload  # noqa: E402

DEV = torch.device("cuda:0")
DIMS = (26, 20, 23)
AABB = ((-1.3, 1.2), (-1.0, 1.1), (-1.4, 1.0))
W, H, VIEWS = 21, 13, 3
LANES = (1, 2, 4, 8)
# the group of a line under --fold: call, S, mode and ray set (and, for a loss that takes ray weights, whether it got them)
GROUP = re.compile(r"(.+?_S\d+(_[a-z]+_[abc](_(un)?weighted)?)?)_")
# name -> (RenderParams fields, jitter kind): caller jitter follows a ray through the shuffle, the hash stream follows the index
MODES = {
    "plain": (dict(), None),
    "hash": (dict(perturb=True), "hash"),
    "caller": (dict(perturb=True), "caller"),
    "clip": (dict(aabb_clip=True), None),
    "lindisp": (dict(linear_disparity=True), None),
}


def digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def cameras(h, w, n):
    rays = [ops.cast_rays(h, w, workload.focal_for(w), *pose_spherical(*workload.synth_pose_angles(i, 8), workload.RADIUS), DEV)
            for i in range(n)]
    return torch.cat([r[0] for r in rays]).contiguous(), torch.cat([r[1] for r in rays]).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--fold", action="store_true")
    a = ap.parse_args()
    lines, unequal = [], []

    def emit(name, t):
        lines.append(f"{digest(t)} {name}")
        print(lines[-1], flush=True)

    g = torch.Generator().manual_seed(20)
    dens = (torch.empty((*DIMS, 1)).uniform_(-1, 1, generator=g) * 1.5).to(DEV)
    feats = {deg: torch.empty((*DIMS, 3 * (deg + 1) ** 2)).uniform_(-1, 1, generator=g).to(DEV) for deg in (0, 2)}
    spec = ops.GridSpec(aabb=AABB, density_scale=2.0, density_pre_act=abi.ACT_IDENTITY, density_post_act=abi.ACT_SOFTPLUS)
    ro, rd = cameras(H, W, VIEWS)
    R = ro.shape[0]
    perm = torch.randperm(R, generator=g).to(DEV)
    values = torch.empty((R, 8)).uniform_(-1, 1, generator=g).to(DEV)
    g_col, g_dep, g_acc = (torch.randn((R, n), generator=g).to(DEV) for n in (3, 1, 1))
    # the depth and orientation losses: their per-ray inputs from a copy of the generator (the draws of the calls above stay as
    # they were), and call(params, o, d, jit, rng, target_depth, target_sigma, ray_weight, **kw) per loss
    gl = torch.Generator()
    gl.set_state(g.get_state())
    t_depth = torch.empty(R).uniform_(workload.NEAR, workload.FAR, generator=gl).to(DEV)
    t_sigma = torch.empty(R).uniform_(0.02, 0.2, generator=gl).to(DEV)
    r_weight = torch.empty(R).uniform_(0, 2, generator=gl)
    r_weight[::7] = 0.0
    r_weight = r_weight.to(DEV)
    ray_losses = {
        "depth": lambda P, o, d, jit, rng, td, ts, w, **kw: ops.depth_fwd_bwd(spec, P, dens, o, d, td, ts, w, jit, rng, **kw),
        "orientation_eps0": lambda P, o, d, jit, rng, td, ts, w, **kw: ops.orientation_fwd_bwd(spec, P, dens, o, d, w, jit, rng,
                                                                                              normal_eps=0.0, **kw),
        "orientation_eps1e-2": lambda P, o, d, jit, rng, td, ts, w, **kw: ops.orientation_fwd_bwd(spec, P, dens, o, d, w, jit, rng,
                                                                                                 normal_eps=1e-2, **kw),
    }
    # per-ray tensors of a set: (a) and (b) as they are, (c) permuted
    sets = {"a": (dict(image_width=W, image_height=H), None), "b": (dict(), None), "c": (dict(), perm)}

    def of_set(t, p):
        return t if p is None or t is None else t[p].contiguous()

    def same_per_ray(name, per_set):
        """the per-ray outputs of (a), (b), (c) agree bit for bit, (c) un-shuffled"""
        back = torch.empty_like(perm)
        back[perm] = torch.arange(R, device=DEV)
        ref = per_set["a"]
        for k in ("b", "c"):
            for x, y in zip(ref, per_set[k]):
                y = y[back] if k == "c" else y
                if not torch.equal(x, y):
                    unequal.append(f"{name}: set {k} differs from set a")

    for S in (33, 96):
        jit_rows = torch.rand((R, S), generator=g).to(DEV)
        for mode, (fields, jkind) in MODES.items():
            rng = (1234, 77) if jkind == "hash" else (0, 0)
            out = {k: {} for k in ("normals", "distortion", "rays", *ray_losses)}
            for sname, (image, p) in sets.items():
                if jkind == "hash" and sname == "c":
                    continue      # (the hash stream follows the ray's index: a shuffled ray is another ray)
                tag = f"S{S}_{mode}_{sname}"
                params = ops.RenderParams(num_samples=S, near=workload.NEAR, far=workload.FAR, white_bkgd=True, sh_degree=2,
                                          **fields, **image)
                o, d = of_set(ro, p), of_set(rd, p)
                jit = of_set(jit_rows, p) if jkind == "caller" else None
                # normals
                N, depth, acc = ops.render_normals(spec, params, dens, o, d, jitter=jit, rng=rng)
                for n, t in (("normals", N), ("depth", depth), ("acc", acc)):
                    emit(f"normals_{tag}_{n}", t)
                out["normals"][sname] = (N, depth, acc)
                # visibility
                mw, mt = torch.zeros(DIMS, device=DEV), torch.zeros(DIMS, device=DEV)
                ops.visibility_accumulate_(spec, params, dens, o, d, mw, mt, jitter=jit, rng=rng)
                emit(f"visibility_{tag}_max_weight", mw)
                emit(f"visibility_{tag}_max_trans", mt)
                # lifting
                for merge in (ops.LIFT_MERGE_PER_LANE, ops.LIFT_MERGE_WAVE):
                    ops.lift_debug_merge(merge)
                    for C in (0, 1, 3, 8):
                        sw = torch.zeros(DIMS, dtype=torch.int64, device=DEV)
                        swv = torch.zeros((*DIMS, C), dtype=torch.int64, device=DEV) if C else None
                        vals = of_set(values[:, :C].contiguous(), p) if C else None
                        ops.lift_accumulate_(spec, params, dens, o, d, vals, swv, sw, jitter=jit, rng=rng)
                        emit(f"lift_{tag}_merge{merge}_C{C}_sum_w", sw)
                        if C:
                            emit(f"lift_{tag}_merge{merge}_C{C}_sum_wv", swv)
                ops.lift_debug_merge(ops.LIFT_MERGE_SHIPPED)
                # distortion and the ray gradients, every lanes-per-ray split
                ups = [of_set(t, p) for t in (g_col, g_dep, g_acc)]
                for lanes in LANES:
                    loss, ray = ops.distortion_fwd_bwd(spec, params, dens, o, d, jit, rng, want_loss=True, want_ray_loss=True, lanes=lanes)
                    emit(f"distortion_{tag}_G{lanes}_loss", loss)
                    emit(f"distortion_{tag}_G{lanes}_ray_loss", ray)
                    d_o, d_d = ops.render_bwd_rays(spec, params, dens, feats[2], o, d, jit, rng, *ups, lanes=lanes)
                    emit(f"rays_{tag}_G{lanes}_d_rays_o", d_o)
                    emit(f"rays_{tag}_G{lanes}_d_rays_d", d_d)
                    out["distortion"].setdefault(sname, []).append(ray)
                    out["rays"].setdefault(sname, []).extend([d_o, d_d])
                # the distortion gradient where float adds cannot race: one ray per call, one lane per ray, one stream
                one = ops.RenderParams(**{**vars(params), "image_width": 0, "image_height": 0})

                def row(t, r):
                    return None if t is None else t[r:r + 1].contiguous()

                if sname == "a":
                    dd = torch.zeros_like(dens)
                    for r in range(64):      # (to the hash stream every one of them is ray 0 of its launch)
                        ops.distortion_fwd_bwd(spec, one, dens, row(o, r), row(d, r), row(jit, r), rng, want_loss=False,
                                               d_densities=dd, accumulate=True, lanes=1)
                    emit(f"distortion_{tag}_G1_d_densities_64_single_ray_calls", dd)
                # the depth and orientation losses the same way, with the ray weights and without
                td, ts, rw = (of_set(t, p) for t in (t_depth, t_sigma, r_weight))
                for lname, call in ray_losses.items():
                    for wname, w in (("weighted", rw), ("unweighted", None)):
                        for lanes in LANES:
                            loss, ray = call(params, o, d, jit, rng, td, ts, w, want_loss=True, want_ray_loss=True, lanes=lanes)
                            emit(f"{lname}_{tag}_{wname}_G{lanes}_loss", loss)
                            emit(f"{lname}_{tag}_{wname}_G{lanes}_ray_loss", ray)
                            out[lname].setdefault(sname, []).append(ray)
                        if sname == "a":
                            dd = torch.zeros_like(dens)
                            for r in range(64):
                                call(one, row(o, r), row(d, r), row(jit, r), rng, row(td, r), row(ts, r), row(w, r), want_loss=False,
                                     d_densities=dd, accumulate=True, lanes=1)
                            emit(f"{lname}_{tag}_{wname}_G1_d_densities_64_single_ray_calls", dd)
            if jkind != "hash":
                for call, per_set in out.items():
                    same_per_ray(f"{call}_S{S}_{mode}", per_set)
            else:
                for call, per_set in out.items():
                    for x, y in zip(per_set["a"], per_set["b"]):
                        if not torch.equal(x, y):
                            unequal.append(f"{call}_S{S}_{mode}: set b differs from set a")
    # normals at the sizes where the launch picks 8 / 4 / 2 / 1 lanes per ray
    for hw in (400, 600, 800, 1040):
        o, d = cameras(hw, hw, 1)
        params = ops.RenderParams(num_samples=64, near=workload.NEAR, far=workload.FAR, image_width=hw)
        for n, t in zip(("normals", "depth", "acc"), ops.render_normals(spec, params, dens, o, d, rng=(0, 0))):
            emit(f"normals_{hw}x{hw}_S64_{n}", t)
    torch.cuda.synchronize()
    if a.fold:
        groups = {}
        for line in lines:
            groups.setdefault(GROUP.match(line.split(" ", 1)[1]).group(1), []).append(line)
        lines = [f"{hashlib.sha256(chr(10).join(m).encode()).hexdigest()} {name} ({len(m)} tensors)" for name, m in groups.items()]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    for u in unequal:
        print(f"PER-RAY MISMATCH {u}", file=sys.stderr)
    sys.exit(1 if unequal else 0)


if __name__ == "__main__":
    main()
