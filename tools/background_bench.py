#!/usr/bin/env python3
"""Environment-map background timings: device time (HIP events, median of --iters calls after warm-up)
of voxe_background_fwd and of voxe_background_bwd -- texel gradient only, and all three outputs -- for both ways of depositing
the texel gradient (voxe_background_debug_merge 1 = run merge, 2 = plain), on
  (a) one 400 x 400 camera, image order;
  (b) a 32 768-ray random batch over 8 cameras, linear order: the trainer's shape,
with maps of 64 x 128 and 512 x 1024 texels.  Each group is timed ALTERNATELY, window by window (8 calls per window), with
  - the SH-0 voxe_render_fwd + voxe_render_bwd of the same rays on the bench's 160^3 random grid (S = 256, packed grid reused);
  - the float32 torch restatement of the same model (tests/background_ref.py) with autograd, forward and forward + backward.
Also the worst case of contention: every ray of the 400 x 400 image in one cell.  One JSON line per case, also written to --out.
Exit status 1 when the shipped kernels (merge mode 0) are slower than the torch restatement anywhere.

    python tools/background_bench.py [--iters 20] [--out profiles/background_bench.txt]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "vox-e_amd"), os.path.join(ROOT, "tests")]

import background_ref as BR  # noqa: E402
from thre3d_atom.utils.imaging_utils import pose_spherical  # noqa: E402
from voxe_hip import abi, ops, workload  # noqa: E402

DEV = torch.device("cuda:0")
RNG = (42, 7)


REPS = 8   # calls per timed window: the kernels take microseconds, one call per window would time the enqueue


def _alternate(fns, iters):
    """median device time in ms per call of every callable of `fns` (a dict), the callables taking turns window by window"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {k: [] for k in fns}
    for i in range(iters + 3):
        for k, fn in fns.items():
            e0.record()
            for _ in range(REPS):
                fn()
            e1.record()
            e1.synchronize()
            if i >= 3:
                times[k].append(e0.elapsed_time(e1) / REPS)
    return {k: round(sorted(v)[len(v) // 2], 4) for k, v in times.items()}


def _rays(hw, cams):
    rays = [ops.cast_rays(hw, hw, workload.focal_for(hw), *pose_spherical(*workload.synth_pose_angles(cam, 100), workload.RADIUS), DEV)
            for cam in cams]
    return torch.cat([r[0] for r in rays]).contiguous(), torch.cat([r[1] for r in rays]).contiguous()


def case_times(texels, rd, colour, acc, g, render, iters):
    """timings of one (rays, map) pair; `render` runs the SH-0 forward + backward of the same rays (None: not timed)"""
    R = rd.shape[0]
    out = torch.empty_like(colour)
    d_acc, d_tex, d_rd = torch.empty((R,), device=DEV), torch.empty_like(texels), torch.empty_like(rd)
    tex_t, rd_t, acc_t = (t.clone().requires_grad_(True) for t in (texels, rd, acc))

    def torch_fwd():
        with torch.no_grad():
            BR.composite(colour, acc, rd, texels, dtype=torch.float32)

    def torch_fwd_bwd(all_three):
        def run():
            o = BR.composite(colour, acc_t if all_three else acc, rd_t if all_three else rd, tex_t, dtype=torch.float32)
            torch.autograd.grad((o * g).sum(), (tex_t, acc_t, rd_t) if all_three else (tex_t,))
        return run

    def bwd(mode, all_three):
        return lambda: ops.background_bwd(texels, rd, acc, g, d_acc=d_acc if all_three else None, d_texels=d_tex,
                                          d_rays_d=d_rd if all_three else None, want_acc=all_three, want_rays_d=all_three, merge=mode)

    fns = {"fwd_ms": lambda: ops.background_fwd_into(texels, rd, colour, acc, out), "torch_fwd_ms": torch_fwd,
           "torch_fwd_bwd_texels_ms": torch_fwd_bwd(False), "torch_fwd_bwd_all_ms": torch_fwd_bwd(True)}
    for mode, name in ((0, "shipped"), (1, "merge"), (2, "plain")):
        fns[f"bwd_texels_{name}_ms"] = bwd(mode, False)
        fns[f"bwd_all_{name}_ms"] = bwd(mode, True)
    if render is not None:
        fns["render_fwd_bwd_ms"] = render
    t = _alternate(fns, iters)
    res = {"rays": R, "map": list(texels.shape[:2]), **t}
    if render is not None:
        res["fwd_plus_bwd_all_over_render"] = round((t["fwd_ms"] + t["bwd_all_shipped_ms"]) / t["render_fwd_bwd_ms"], 4)
    res["torch_over_kernel_fwd"] = round(t["torch_fwd_ms"] / t["fwd_ms"], 2)
    res["torch_over_kernel_fwd_bwd_all"] = round(t["torch_fwd_bwd_all_ms"] / (t["fwd_ms"] + t["bwd_all_shipped_ms"]), 2)
    res["slower_than_torch"] = bool(t["fwd_ms"] > t["torch_fwd_ms"]
                                    or t["fwd_ms"] + t["bwd_all_shipped_ms"] > t["torch_fwd_bwd_all_ms"]
                                    or t["fwd_ms"] + t["bwd_texels_shipped_ms"] > t["torch_fwd_bwd_texels_ms"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "background_bench.txt"))
    a = ap.parse_args()
    spec = ops.GridSpec(aabb=((-1.5, 1.5),) * 3, density_scale=100.0 / 3.0, density_pre_act=abi.ACT_IDENTITY,
                        density_post_act=abi.ACT_SOFTPLUS)
    d, f = workload.random_grid(160)
    dens, feat = d.to(DEV).contiguous(), f.to(DEV).contiguous()
    gen = torch.Generator().manual_seed(43)
    maps = [(torch.randn(n, 2 * n, 3, generator=gen) * 1.5).to(DEV) for n in (64, 512)]
    ro_i, rd_i = _rays(400, [3])
    ro_b, rd_b = _rays(400, [3 + 12 * j for j in range(8)])
    pick = torch.randperm(ro_b.shape[0], generator=torch.Generator().manual_seed(11))[:32768].to(DEV)
    ro_b, rd_b = ro_b[pick].contiguous(), rd_b[pick].contiguous()
    lines = []
    for name, ro, rd, width in (("400x400_image", ro_i, rd_i, 400), ("batch32768_of_8cams_linear", ro_b, rd_b, 0)):
        R = ro.shape[0]
        params = ops.RenderParams(num_samples=256, near=workload.NEAR, far=workload.FAR, perturb=True, sh_degree=0, image_width=width)
        outs = [torch.empty((R, n), dtype=torch.float32, device=DEV) for n in (3, 1, 1, 1)]
        g = torch.randn((R, 3), generator=gen).to(DEV)
        r_dens, r_feat = torch.zeros_like(dens), torch.zeros_like(feat)
        ws = ops.Workspace()

        def render():
            ops.render_fwd_into(spec, params, dens, feat, ro, rd, None, *outs, ws, RNG)
            ops.render_bwd_into(spec, params, dens, feat, ro, rd, None, outs[0], outs[1], outs[2], g, None, None, r_dens, r_feat, ws, RNG)

        render()
        colour, acc = outs[0].clone(), outs[2].reshape(-1).clone()
        # (the random grid saturates nearly every ray; the background's cost does not depend on acc unless it is exactly 1, where
        #  a ray deposits nothing: time it on rays that all deposit)
        acc = acc.clamp(max=0.9)
        for texels in maps:
            lines.append({"case": f"random160_{name}_S256", **case_times(texels, rd, colour, acc, g, render, a.iters)})
            print(json.dumps(lines[-1]), flush=True)
    # worst case: every ray of the image in one cell of the small map
    R = rd_i.shape[0]
    u = 40 + 0.05 + 0.9 * torch.rand(R, generator=gen, dtype=torch.float64)
    v = 20 + 0.05 + 0.9 * torch.rand(R, generator=gen, dtype=torch.float64)
    rd_one = BR.directions_from_uv(u, v, 64, 128).float().to(DEV).contiguous()
    colour, acc, g = torch.rand((R, 3), generator=gen).to(DEV), (torch.rand(R, generator=gen) * 0.9).to(DEV), torch.randn((R, 3), generator=gen).to(DEV)
    lines.append({"case": "one_cell_160000_rays", **case_times(maps[0], rd_one, colour, acc, g, None, a.iters)})
    print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")
    if any(line["slower_than_torch"] for line in lines):
        print("the shipped kernels are slower than the torch restatement", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
