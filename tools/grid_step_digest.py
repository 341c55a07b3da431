#!/usr/bin/env python3
"""Bit digests of the streaming passes that share voxe_grid_elem.hpp: pack, un-pack of the gradient, the
fused grid step (voxe_grid_adam_step) and the stand-alone passes whose per-element arithmetic it repeats (voxe_adam_step,
voxe_dcl_fwd_bwd, voxe_density_diff_fwd_bwd, voxe_feature_correlation_fwd_bwd) on seeded inputs, one `sha256 name` line per
output tensor.  None of these kernels has an atomic and every reduction folds in a fixed order, so two trees whose kernels compute
the same bits print the same lines: a change of the shared element functions is checked by running this file in both trees and
comparing the outputs line for line.

Grid step: texels of 2 / 4 / 13 / 28 / 49 channels, a hand-written gradient region, three steps each (both sweep directions of
the coalesced SH-0 kernel); 35 voxels per x plane, so the whole grid is chunks + a tail, slab [4, 12) or [4, 8) starts 16-byte
aligned and slab [1, 9) or [1, 5) does not; the bricked layout, a frozen tensor, extra gradients, per-tensor step counts, and
every regulariser kind inside the step with its logged value.  Pack / un-pack: the packed grid a forward leaves in the
workspace, and the gradients of a backward in deterministic mode and of single-ray launches (float atomics of one launch
order-free there), with `accumulate` 0 and 1.

    python tools/grid_step_digest.py [--out FILE]
"""
import argparse
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "vox-e_amd")]

from thre3d_atom.utils.imaging_utils import pose_spherical  # noqa: E402
from voxe_hip import abi, ops, workload  # noqa: E402
from voxe_hip.runtime import VoxeError, check, lib, ptr, stream_ptr  # noqa: E402

DEV = torch.device("cuda:0")
AABB = ((-1.5, 1.5),) * 3
LR = 3e-3
CHANNELS = (2, 4, 13, 28, 49)


def digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def spec_for(C, pre=abi.ACT_ABS):
    return ops.GridSpec(aabb=AABB, density_scale=3.0, density_pre_act=pre, density_post_act=abi.ACT_SOFTPLUS,
                        feature_kind=abi.FEAT_ATTN if C == 2 else abi.FEAT_SH)


def grid_for(C, dims, gen):
    return (torch.empty((*dims, 1)).uniform_(-1, 1, generator=gen).to(DEV),
            torch.empty((*dims, C - 1)).uniform_(-1, 1, generator=gen).to(DEV))


def workspace_for(dens, feat):
    ws = ops.Workspace()
    ws.ensure(4 * 2 * (dens.numel() + feat.numel()) * 2 + (1 << 16), DEV)
    ws.buf.zero_()
    return ws


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def emit(name, t):
        lines.append(f"{digest(t)} {name}")
        print(lines[-1], flush=True)

    L = lib()
    st = stream_ptr(DEV)

    # ---- the fused grid step -------------------------------------------------------------------------------------------
    def run_step(tag, C, dims, layout=abi.GRAD_LINEAR, x_range=None, frozen=None, extras=False, step_features=0, pre=abi.ACT_ABS, **reg):
        gen = torch.Generator().manual_seed(1000 + C)
        spec = spec_for(C, pre)
        dens, feat = grid_for(C, dims, gen)
        refs = {}
        if "dcl_weight" in reg:
            refs["dcl_reference"] = (dens * 0.8 + 0.1 * torch.empty(dens.shape).normal_(generator=gen).to(DEV)).contiguous()
            refs["dcl_loss"] = torch.zeros((), device=DEV)
        if "feat_weight" in reg:
            refs["feat_reference"] = (feat + 0.3 * torch.empty(feat.shape).normal_(generator=gen).to(DEV)).contiguous()
            refs["feat_loss"] = torch.zeros((), device=DEV)
        ws = workspace_for(dens, feat)
        m = [torch.zeros_like(dens), torch.zeros_like(feat)]
        v = [torch.zeros_like(dens), torch.zeros_like(feat)]
        for step in (1, 2, 3):
            region = ops.workspace_grad_view(spec, dens, feat, ws)
            region.copy_(torch.empty(region.numel()).normal_(generator=gen))
            ex_d = torch.empty(dens.shape).normal_(generator=gen).to(DEV) if extras else None
            ex_f = torch.empty(feat.shape).normal_(generator=gen).to(DEV) if extras else None
            ops.grid_adam_step_(spec, dens, feat, layout, ws, step, LR, None if frozen == "densities" else (m[0], v[0]),
                                None if frozen == "features" else (m[1], v[1]), ex_d, ex_f, x_range=x_range,
                                step_features=step + step_features, **reg, **refs)
            for nm in ("dcl_loss", "feat_loss"):
                if nm in refs:
                    emit(f"step_C{C}_{tag}_s{step}_{nm}", refs[nm])
        for nm, t in (("densities", dens), ("features", feat), ("exp_avg_d", m[0]), ("exp_avg_sq_d", v[0]), ("exp_avg_f", m[1]),
                      ("exp_avg_sq_f", v[1]), ("packed", ops.workspace_packed_view(spec, dens, feat, ws)),
                      ("grad_region", ops.workspace_grad_view(spec, dens, feat, ws))):
            emit(f"step_C{C}_{tag}_{nm}", t)

    for C in CHANNELS:
        dims = (16, 5, 7) if C <= 4 else (8, 5, 7)
        half = dims[0] // 2
        run_step("whole", C, dims)
        run_step("whole_identity", C, dims, pre=abi.ACT_IDENTITY)
        run_step("slab_aligned", C, dims, x_range=(4, 4 + half))
        run_step("slab_unaligned", C, dims, x_range=(1, 1 + half))
        run_step("bricked", C, dims, layout=abi.GRAD_BRICKED)
        run_step("bricked_slab", C, dims, layout=abi.GRAD_BRICKED, x_range=(2, 2 + half))
        run_step("frozen_densities", C, dims, frozen="densities")
        run_step("frozen_features", C, dims, frozen="features")
        run_step("extras", C, dims, extras=True)
        run_step("extras_bricked", C, dims, extras=True, layout=abi.GRAD_BRICKED)
        run_step("step_features", C, dims, step_features=2)
        for kind, nm, w in ((abi.DREG_CORRELATION, "correlation", 200.0), (abi.DREG_L2, "l2", 50.0), (abi.DREG_L1, "l1", 5.0)):
            run_step(f"reg_{nm}", C, dims, dcl_weight=w, density_kind=kind)
            run_step(f"reg_{nm}_bricked", C, dims, layout=abi.GRAD_BRICKED, dcl_weight=w, density_kind=kind)
        if C <= 4:      # (the feature term inside the step: texels of up to 4 channels)
            run_step("reg_featcorr", C, dims, feat_weight=0.01)
            run_step("reg_featcorr_bricked", C, dims, layout=abi.GRAD_BRICKED, feat_weight=0.01)
            run_step("reg_featcorr_extras_l2", C, dims, extras=True, feat_weight=0.01, dcl_weight=50.0, density_kind=abi.DREG_L2)
            run_step("reg_featcorr_frozen_densities", C, dims, frozen="densities", feat_weight=0.01)

    # ---- the stand-alone passes ----------------------------------------------------------------------------------------
    gen = torch.Generator().manual_seed(77)
    n = 16 * 5 * 7 * 3 + 1          # (odd: the last block is partial)
    p, m, v = (torch.empty(n).uniform_(-1, 1, generator=gen).to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV))
    for step in (1, 2, 3):
        ops.adam_step_(p, torch.empty(n).normal_(generator=gen).to(DEV), m, v, step, LR)
    for nm, t in (("param", p), ("exp_avg", m), ("exp_avg_sq", v)):
        emit(f"adam_step_{nm}", t)
    nvox = 16 * 5 * 7
    da = torch.empty(nvox).uniform_(-1, 1, generator=gen).to(DEV)
    db = (da * 0.8 + 0.1 * torch.empty(nvox).normal_(generator=gen).to(DEV)).contiguous()
    db[::7] = da[::7]
    sc = torch.empty(L.voxe_dcl_scratch_bytes(nvox), dtype=torch.uint8, device=DEV)
    loss = torch.zeros((), device=DEV)
    for acc in (0, 1):
        seed = torch.empty(nvox).normal_(generator=gen).to(DEV)
        g = seed.clone()
        check(L.voxe_dcl_fwd_bwd(ptr(da), ptr(db), nvox, 200.0, ptr(loss), ptr(g), acc, ptr(sc), sc.numel(), st), "voxe_dcl_fwd_bwd")
        emit(f"dcl_acc{acc}_loss", loss)
        emit(f"dcl_acc{acc}_grad", g)
        for kind, nm, w in ((abi.DREG_L2, "l2", 50.0), (abi.DREG_L1, "l1", 5.0)):
            g = seed.clone()
            check(L.voxe_density_diff_fwd_bwd(ptr(da), ptr(db), nvox, kind, w, ptr(loss), ptr(g), acc, ptr(sc), sc.numel(), st),
                  "voxe_density_diff_fwd_bwd")
            emit(f"density_diff_{nm}_acc{acc}_loss", loss)
            emit(f"density_diff_{nm}_acc{acc}_grad", g)
        for F in (1, 3, 12):
            f = torch.empty(nvox * F).uniform_(-1, 1, generator=gen).to(DEV)
            r = (f + 0.3 * torch.empty(nvox * F).normal_(generator=gen).to(DEV)).contiguous()
            g = torch.empty(nvox * F).normal_(generator=gen).to(DEV)
            check(L.voxe_feature_correlation_fwd_bwd(ptr(f), ptr(r), nvox, F, 0.01, ptr(loss), ptr(g), acc, ptr(sc), sc.numel(), st),
                  "voxe_feature_correlation_fwd_bwd")
            emit(f"feature_correlation_F{F}_acc{acc}_loss", loss)
            emit(f"feature_correlation_F{F}_acc{acc}_grad", g)

    # ---- pack (the grid a forward leaves in the workspace) and un-pack (the gradients of a backward) ------------------------
    W = 16
    ro, rd = ops.cast_rays(W, W, workload.focal_for(W), *pose_spherical(*workload.synth_pose_angles(3, 100), workload.RADIUS), DEV)
    R = ro.shape[0]
    for C in CHANNELS:
        gen = torch.Generator().manual_seed(2000 + C)
        dims = (16, 5, 7) if C <= 4 else (8, 5, 7)
        cout = 1 if C == 2 else 3
        deg = {2: 0, 4: 0, 13: 1, 28: 2, 49: 3}[C]
        dens, feat = grid_for(C, dims, gen)
        dens = dens * 0.5 + 0.5
        g_col, g_dep, g_acc = (torch.empty((R, k)).normal_(generator=gen).to(DEV) for k in (cout, 1, 1))
        for pre, pname in ((abi.ACT_ABS, "abs"), (abi.ACT_IDENTITY, "identity")):
            spec = spec_for(C, pre)
            # (a) deterministic mode, image order; (b) one ray per launch, accumulated: both free of atomics' order
            for mode in ("deterministic", "single_rays"):
                det = mode == "deterministic"
                params = ops.RenderParams(num_samples=16, near=workload.NEAR, far=workload.FAR, white_bkgd=C != 2, sh_degree=deg,
                                          image_width=W if det else 0, deterministic=det)
                rays = [(ro, rd, g_col, g_dep, g_acc)] if det else \
                    [tuple(t[i:i + 1].contiguous() for t in (ro, rd, g_col, g_dep, g_acc)) for i in range(100, 124)]
                d_d, d_f = (torch.empty(dens.shape).normal_(generator=gen).to(DEV), torch.empty(feat.shape).normal_(generator=gen).to(DEV))
                ws = ops.Workspace()
                try:
                    for k, (o, d, gc, gdp, ga) in enumerate(rays):
                        out = [torch.empty((o.shape[0], c), device=DEV) for c in (cout, 1, 1, 1)]
                        ops.render_fwd_into(spec, params, dens, feat, o, d, None, *out, ws, (5, 9))
                        if k == 0:
                            emit(f"pack_C{C}_{pname}_{mode}_packed", ops.workspace_packed_view(spec, dens, feat, ws))
                        ops.render_bwd_into(spec, params, dens, feat, o, d, None, out[0], out[1], out[2], gc, gdp, ga, d_d, d_f, ws,
                                            (5, 9), accumulate=not det or pre == abi.ACT_IDENTITY)
                except VoxeError as e:
                    print(f"# unpack_C{C}_{pname}_{mode}: not offered ({e})", flush=True)
                    continue
                emit(f"unpack_C{C}_{pname}_{mode}_d_densities", d_d)
                emit(f"unpack_C{C}_{pname}_{mode}_d_features", d_f)
    torch.cuda.synchronize()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
