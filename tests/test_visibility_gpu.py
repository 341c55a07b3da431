"""GPU checks of the per-voxel visibility grids (voxe_visibility_accumulate / voxe_visibility_mask, thre3d_reprs.visibility,
prune_voxel_grid.py, export_mesh.py --visible_only): agreement with the float64 restatement tests/visibility_ref.py, the
contract's bit-level properties, an opaque analytic ball, lossless threshold-0 pruning, the mask kernel, edge cases, no
interference with a forward / backward, and the entry points on the golden checkpoint.  The inputs come from
tests/test_visibility_host.py, which checks on the host that they are not vacuous."""
import importlib.util
import os
import re

import pytest
import torch
import torch.nn.functional as F

import test_visibility_host as H
import visibility_ref
from conftest import GOLDEN, ROOT
from test_mesh_host import parse_ply
from voxe_hip import abi, ops, workload
from voxe_hip.runtime import VoxeError

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _accumulate(spec, params, dens, ro, rd, jitter=None, rng=(0, 0), weight=True, trans=True, out=None):
    mw, mt = out if out is not None else (torch.zeros(dens.shape[:3], device=DEV) for _ in range(2))
    ops.visibility_accumulate_(spec, params, dens, ro, rd, mw if weight else None, mt if trans else None, jitter=jitter, rng=rng)
    return mw, mt


# ---- 1: agreement with the restatement --------------------------------------------------------------------------------
@pytest.mark.parametrize("pre,post", H.ACTS)
@pytest.mark.parametrize("case", H.agreement_cases(), ids=lambda c: c[0])
def test_visibility_matches_the_restatement(case, pre, post):
    spec, params, dens, feat, ro, rd, jitter, rng = H.agreement_inputs(case, pre, post, DEV)
    mw, mt = _accumulate(spec, params, dens, ro, rd, jitter, rng)
    rw, rt = visibility_ref.visibility(spec, params, dens, feat, ro, rd, jitter, rng)
    H.assert_agreement_not_vacuous(rw, rt)
    err_w, err_t = float((mw.double() - rw).abs().max()), float((mt.double() - rt).abs().max())
    print(f"max|max_weight - ref| {err_w:.3e}  max|max_trans - ref| {err_t:.3e}")
    assert err_w <= 1e-5 and err_t <= 1e-5
    assert bool((mw[rw == 0] == 0).all()) and bool((mt[rt == 0] == 0).all())
    assert float(mt.max()) == 1.0                       # the first inside sample arrives with T = 1
    assert bool(torch.isfinite(mw).all()) and float(mw.min()) >= 0 and float(mw.max()) <= 1


# ---- 2: contract properties, all bit for bit --------------------------------------------------------------------------
def test_order_launch_split_and_accumulation_do_not_change_a_bit():
    hw, K, S = 24, 3, 64
    g = torch.Generator().manual_seed(3)
    dens = (torch.empty((*H.DIMS, 1)).uniform_(-1, 1, generator=g) * 1.5).to(DEV)
    spec = ops.GridSpec(aabb=H.AABB, density_scale=2.0)
    ro, rd = H.cameras(hw, K, DEV)
    R, per = ro.shape[0], hw * hw
    jitter = torch.rand((R, S), generator=g).to(DEV)
    kw = dict(num_samples=S, near=workload.NEAR, far=workload.FAR, perturb=True)
    multi = ops.RenderParams(image_width=hw, image_height=hw, **kw)
    base = _accumulate(spec, multi, dens, ro, rd, jitter)
    assert float(base[0].max()) > 0.01 and float(base[1].max()) == 1.0
    # the same call twice
    again = _accumulate(spec, multi, dens, ro, rd, jitter)
    assert torch.equal(base[0], again[0]) and torch.equal(base[1], again[1])
    # K launches into the same buffers
    one = ops.RenderParams(image_width=hw, **kw)
    split = None
    for k in range(K):
        s = slice(k * per, (k + 1) * per)
        split = _accumulate(spec, one, dens, ro[s].contiguous(), rd[s].contiguous(), jitter[s].contiguous(), out=split)
    assert torch.equal(base[0], split[0]) and torch.equal(base[1], split[1])
    # no image fields: linear order
    linear = _accumulate(spec, ops.RenderParams(**kw), dens, ro, rd, jitter)
    assert torch.equal(base[0], linear[0]) and torch.equal(base[1], linear[1])
    # shuffled rays, the jitter rows permuted along
    perm = torch.randperm(R, generator=g).to(DEV)
    shuf = _accumulate(spec, ops.RenderParams(**kw), dens, ro[perm].contiguous(), rd[perm].contiguous(), jitter[perm].contiguous())
    assert torch.equal(base[0], shuf[0]) and torch.equal(base[1], shuf[1])
    # no jitter at all (perturb off): the same properties without a caller stream
    off = dict(kw, perturb=False)
    a = _accumulate(spec, ops.RenderParams(image_width=hw, image_height=hw, **off), dens, ro, rd)
    b = _accumulate(spec, ops.RenderParams(**off), dens, ro[perm].contiguous(), rd[perm].contiguous())
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[0], base[0])
    # accumulation onto a pre-filled non-negative buffer
    pre = [(torch.rand(H.DIMS, generator=g) * s).to(DEV) for s in (0.05, 1.0)]
    onto = _accumulate(spec, multi, dens, ro, rd, jitter, out=(pre[0].clone(), pre[1].clone()))
    assert torch.equal(onto[0], torch.maximum(pre[0], base[0])) and torch.equal(onto[1], torch.maximum(pre[1], base[1]))
    # one NULL output leaves the other as it is with both
    only_w = _accumulate(spec, multi, dens, ro, rd, jitter, trans=False)
    only_t = _accumulate(spec, multi, dens, ro, rd, jitter, weight=False)
    assert torch.equal(only_w[0], base[0]) and int(only_w[1].count_nonzero()) == 0
    assert torch.equal(only_t[1], base[1]) and int(only_t[0].count_nonzero()) == 0


# ---- 3: opaque analytic ball ------------------------------------------------------------------------------------------
def test_opaque_ball_is_occluded_inside_and_open_outside():
    dens, dist, _ = H.ball_field()
    spec, params = H.ball_setup()
    dens, dist = dens.to(DEV), dist.to(DEV)
    out = None
    for yaw, pitch in H.BALL_ANGLES:
        ro, rd = H.cast(H.BALL_HW, yaw, pitch, H.BALL_RADIUS, DEV)
        out = _accumulate(spec, params, dens, ro, rd, out=out)
    mw, mt = out
    r0 = H.BALL_R0
    inner = dist < 0.1
    # any ray reaching radius rho crosses at least the radial optical depth 20 (r0 - rho)^2: T <= exp(-7.2)
    print(f"inner: max_trans {float(mt[inner].max()):.3e} max_weight {float(mw[inner].max()):.3e}")
    assert int(inner.sum()) > 50 and float(mt[inner].max()) < 0.01 and float(mw[inner].max()) < 1e-3
    # some camera lies within 90 degrees of every direction and sees the shell through (almost) empty space
    shell = (dist > r0 + 0.15) & (dist < r0 + 0.3)
    print(f"shell: min max_trans {float(mt[shell].min()):.6f}")
    assert int(shell.sum()) > 10000 and float(mt[shell].min()) >= 0.95
    # where the weight peaks: the skin of the ball.  H.BALL_WEIGHT_LEVEL replaces the 0.05 first written down for this test,
    # which no sample reaches (see its comment)
    big = mw > H.BALL_WEIGHT_LEVEL
    print(f"max_weight > {H.BALL_WEIGHT_LEVEL}: {int(big.sum())} voxels, dist {float(dist[big].min()):.3f} .. {float(dist[big].max()):.3f}; "
          f"max {float(mw.max()):.4f}")
    assert int(big.sum()) > 1000
    assert float(dist[big].min()) > r0 - 0.4 and float(dist[big].max()) < r0 + 0.1


# ---- 4: threshold-0 pruning is lossless for the cameras it came from --------------------------------------------------
def test_pruning_at_threshold_zero_keeps_the_renders():
    from thre3d_atom.thre3d_reprs.visibility import prune_voxel_grid_
    from thre3d_atom.thre3d_reprs.voxels import VoxelGrid, VoxelSize

    spec, params, dens, feat, ro, rd, jitter = H.prune_inputs(DEV)
    with torch.no_grad():
        before = ops.render(spec, params, dens, feat, ro, rd, jitter=jitter)
    mw, _ = _accumulate(spec, params, dens, ro, rd, jitter)
    keep = ops.visibility_mask(mw, 0.0, 0)
    assert torch.equal(keep.bool(), mw > 0)
    H.assert_prune_not_vacuous(keep)
    vg = VoxelGrid(dens.clone(), feat.clone(), VoxelSize(*(3.0 / 40,) * 3), density_preactivation=torch.nn.Identity(),
                   density_postactivation=torch.nn.ReLU(), expected_density_scale=3.0)
    changed = prune_voxel_grid_(vg, keep)
    assert 0 < changed <= int((keep == 0).sum())
    assert torch.equal(vg.densities[keep.bool()], dens[keep.bool()]) and torch.equal(vg.features, feat)
    assert float(vg.densities[~keep.bool()].max()) <= 0.0
    with torch.no_grad():
        after = ops.render(spec, params, vg.densities, vg.features, ro, rd, jitter=jitter)
    for name, a, b in zip(("colour", "depth", "acc"), before, after):
        err = float((a - b).abs().max())
        print(f"{name}: max|pruned - original| {err:.3e}")
        assert err <= 2e-6, name
    assert float(before[2].max()) > 0.5


# ---- 5: mask kernel ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(19, 11, 14), (1, 7, 5)])
def test_mask_kernel_is_a_strict_threshold_and_a_box_dilation(dims):
    g = torch.Generator().manual_seed(sum(dims))
    vis = torch.rand(dims, generator=g)
    vis[torch.rand(dims, generator=g) < 0.9] = 0.0       # sparse: a dilation has something to do
    thr = 0.37
    vis[0, 3, 2] = thr                                    # exactly at the threshold: dropped
    vis[0, 5, 4] = float("nan")                           # never kept
    vis = vis.to(DEV)
    above = (vis > thr).float()[None, None]
    assert not bool(above[0, 0, 0, 3, 2]) and not bool(above[0, 0, 0, 5, 4])
    for dilate in (0, 1, 2, 3):
        want = F.max_pool3d(above, 2 * dilate + 1, stride=1, padding=dilate)[0, 0].to(torch.uint8)
        got = ops.visibility_mask(vis, thr, dilate)
        assert got.dtype == torch.uint8 and got.shape == vis.shape and torch.equal(got, want), dilate
        assert torch.equal(got, ops.visibility_mask(vis[..., None], thr, dilate))
    assert 0 < int(ops.visibility_mask(vis, thr, 0).sum()) < vis.numel() // 2
    zero = ops.visibility_mask(vis, 0.0, 0)
    assert torch.equal(zero.bool(), vis > 0)
    with pytest.raises(VoxeError, match=str(abi.ERR_BAD_SHAPE)):
        ops.visibility_mask(vis, thr, 4)


# ---- 6: edges and non-interference ------------------------------------------------------------------------------------
def _in_unit_range(*grids):
    return all(bool(torch.isfinite(t).all()) and float(t.min()) >= 0.0 and float(t.max()) <= 1.0 for t in grids)


def test_edge_cases():
    g = torch.Generator().manual_seed(5)
    dens = torch.empty((32, 24, 28, 1)).uniform_(-1, 1, generator=g).to(DEV)
    spec = ops.GridSpec(aabb=H.AABB, density_scale=2.0)
    ro, rd = H.cameras(64, 1, DEV)
    # R = 0: nothing is touched
    e = torch.zeros((0, 3), device=DEV)
    params = ops.RenderParams(num_samples=128, near=workload.NEAR, far=workload.FAR, image_width=64)
    mw, mt = _accumulate(spec, params, dens, e, e)
    assert int(mw.count_nonzero()) == 0 and int(mt.count_nonzero()) == 0
    # S = 2048 on 3000 rays
    p2 = ops.RenderParams(num_samples=2048, near=workload.NEAR, far=workload.FAR, perturb=True)
    mw, mt = _accumulate(spec, p2, dens, ro[:3000].contiguous(), rd[:3000].contiguous(), rng=(1, 2))
    assert _in_unit_range(mw, mt) and float(mt.max()) == 1.0 and float(mw.max()) > 0
    # shape / dtype errors are raised, not launched
    with pytest.raises(VoxeError):
        ops.visibility_accumulate_(spec, params, dens, ro, rd, torch.zeros((32, 24, 27), device=DEV))
    with pytest.raises(VoxeError):
        ops.visibility_accumulate_(spec, params, dens, ro, rd, torch.zeros((32, 24, 28), device=DEV, dtype=torch.float64))


def test_large_grid_and_image():
    # 256^3 at 800 x 800, S = 512
    d256, _ = workload.random_grid(256, nfeat=1, seed=2)
    big = ops.GridSpec(aabb=((-1.5, 1.5),) * 3, density_scale=2.0)
    o8, r8 = H.cameras(800, 1, DEV, first=3)
    p8 = ops.RenderParams(num_samples=512, near=workload.NEAR, far=workload.FAR, perturb=True, image_width=800)
    mw, mt = _accumulate(big, p8, d256.to(DEV), o8, r8, rng=(7, 8))
    assert _in_unit_range(mw, mt) and float(mt.max()) == 1.0 and float(mw.max()) > 0.01
    assert int((mt > 0).sum()) > 256 ** 3 // 4


def test_no_interference_with_a_forward_and_its_deterministic_backward():
    g = torch.Generator().manual_seed(8)
    dens0 = torch.empty((40, 40, 40, 1)).uniform_(-1, 1, generator=g).to(DEV)
    feat0 = torch.empty((40, 40, 40, 3)).uniform_(-1, 1, generator=g).to(DEV)
    spec = ops.GridSpec(aabb=((-1.5, 1.5),) * 3, density_scale=3.0)
    ro, rd = H.cameras(64, 1, DEV)
    # (the fixed-point backward: two backward passes of the same forward give the same bits)
    params = ops.RenderParams(num_samples=64, near=workload.NEAR, far=workload.FAR, perturb=True, white_bkgd=True, image_width=64,
                              deterministic=True)
    g_col = torch.rand((ro.shape[0], 3), generator=torch.Generator().manual_seed(2)).to(DEV)
    grads = []
    for with_visibility in (False, True):
        d, f = dens0.clone().requires_grad_(True), feat0.clone().requires_grad_(True)
        ws = ops.Workspace()
        col = ops.render(spec, params, d, f, ro, rd, workspace=ws, rng=(3, 4))[0]
        if with_visibility:
            mw, mt = _accumulate(spec, params, d, ro, rd, rng=(3, 4))
            ops.visibility_mask(mw, 0.0, 1)
        (col * g_col).sum().backward()
        grads.append((d.grad.clone(), f.grad.clone()))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    assert float(grads[0][0].abs().max()) > 0


# ---- 7: entry points on the golden checkpoint -------------------------------------------------------------------------
def _load_cli(name):
    spec = importlib.util.spec_from_file_location(name[:-3] + "_vis_gpu_cli", os.path.join(ROOT, name))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _load_model(path):
    from thre3d_atom.modules.volumetric_model import create_volumetric_model_from_saved_model
    from thre3d_atom.thre3d_reprs.voxels import create_voxel_grid_from_saved_info_dict

    return create_volumetric_model_from_saved_model(path, create_voxel_grid_from_saved_info_dict, device=DEV)


def test_prune_cli_on_the_checkpoint(tmp_path):
    from click.testing import CliRunner

    from thre3d_atom.utils.constants import CAMERA_INTRINSICS, EXTRA_ACCUMULATED_WEIGHTS, HEMISPHERICAL_RADIUS
    from thre3d_atom.utils.imaging_utils import get_thre360_animation_poses

    ckpt = os.path.join(GOLDEN, "ref_checkpoint.pth")
    mod = _load_cli("prune_voxel_grid.py")
    base = ["-i", ckpt, "--num_views", "6", "--overridden_num_samples_per_ray", "64"]
    orig, extra = _load_model(ckpt)
    # the defaults (threshold 0, one voxel of dilation): the output loads and carries the input's features.  On this 6^3 grid of
    # dense Softplus blobs every voxel weighs at least 2.5e-3 in some pixel (the float64 restatement over the oracle's samples,
    # 5 poses, S = 64), so nothing falls to the default threshold here; the counts are checked on the next run
    res = CliRunner().invoke(mod.main, base + ["-o", str(tmp_path / "default.pth")])
    assert res.exit_code == 0, (res.output, res.exception)
    kept, pruned = (int(v) for v in re.search(r"kept (\d+)\s+pruned (\d+)", res.output).groups())
    assert kept > 0 and kept + pruned == orig.thre3d_repr.densities.numel()
    dflt, _ = _load_model(tmp_path / "default.pth")
    assert torch.equal(dflt.thre3d_repr.features, orig.thre3d_repr.features)
    # threshold 0.1 without dilation (the restatement keeps 119 of the 216 voxels): something is pruned, something is kept
    res = CliRunner().invoke(mod.main, base + ["-o", str(tmp_path / "pruned.pth"), "--weight_threshold", "0.1", "--dilate", "0"])
    assert res.exit_code == 0, (res.output, res.exception)
    kept, pruned = (int(v) for v in re.search(r"kept (\d+)\s+pruned (\d+)", res.output).groups())
    assert kept > 0 and pruned > 0 and kept + pruned == orig.thre3d_repr.densities.numel()
    assert re.search(r"visibility [\d.]+ ms", res.output)
    new, extra2 = _load_model(tmp_path / "pruned.pth")
    assert torch.equal(new.thre3d_repr.features, orig.thre3d_repr.features) and extra2.keys() == extra.keys()
    d0, d1 = orig.thre3d_repr.densities.detach(), new.thre3d_repr.densities.detach()
    assert bool((d1 <= d0).all()) and 0 < int((d1 != d0).sum()) <= pruned
    # threshold 0, no dilation: the renders of those poses stay
    res = CliRunner().invoke(mod.main, base + ["-o", str(tmp_path / "lossless.pth"), "--weight_threshold", "0", "--dilate", "0"])
    assert res.exit_code == 0, (res.output, res.exception)
    same, _ = _load_model(tmp_path / "lossless.pth")
    assert torch.equal(same.thre3d_repr.features, orig.thre3d_repr.features)
    for pose in get_thre360_animation_poses(extra[HEMISPHERICAL_RADIUS], 60.0, 6):
        kw = dict(num_samples_per_ray=64, perturb_sampled_points=False)
        a, b = orig.render(pose, extra[CAMERA_INTRINSICS], **kw), same.render(pose, extra[CAMERA_INTRINSICS], **kw)
        for x, y in ((a.colour, b.colour), (a.depth, b.depth),
                     (a.extra[EXTRA_ACCUMULATED_WEIGHTS], b.extra[EXTRA_ACCUMULATED_WEIGHTS])):
            assert float((x - y).abs().max()) <= 2e-6


def test_export_mesh_visible_only_on_the_checkpoint(tmp_path):
    from click.testing import CliRunner

    from thre3d_atom.modules.volumetric_model import create_volumetric_model_from_saved_model_attn
    from thre3d_atom.thre3d_reprs.mesh import default_level, extract_mesh, save_ply
    from thre3d_atom.thre3d_reprs.voxels import create_voxel_grid_from_saved_info_dict_attn

    ckpt = os.path.join(GOLDEN, "ref_checkpoint.pth")
    exp = _load_cli("export_mesh.py")
    res = CliRunner().invoke(exp.main, ["-i", ckpt, "-o", str(tmp_path / "all.ply")])
    assert res.exit_code == 0, (res.output, res.exception)
    res = CliRunner().invoke(exp.main, ["-i", ckpt, "-o", str(tmp_path / "seen.ply"), "--visible_only", "--num_views", "6",
                                        "--visibility_threshold", "0.02"])
    assert res.exit_code == 0, (res.output, res.exception)
    t_all, t_seen = len(parse_ply(tmp_path / "all.ply")[2]), len(parse_ply(tmp_path / "seen.ply")[2])
    assert 0 < t_seen <= t_all
    res = CliRunner().invoke(exp.main, ["-i", ckpt, "-o", str(tmp_path / "seen0.ply"), "--visible_only", "--num_views", "6"])
    assert res.exit_code == 0, (res.output, res.exception)
    assert 0 < len(parse_ply(tmp_path / "seen0.ply")[2]) <= t_all
    # without the flag: the bytes of the script's logic before the option existed
    vol_mod, _ = create_volumetric_model_from_saved_model_attn(ckpt, create_voxel_grid_from_saved_info_dict_attn, device=DEV,
                                                               load_attn=False)
    grid = vol_mod.thre3d_repr
    save_ply(extract_mesh(grid, level=default_level(grid), mask=None), tmp_path / "direct.ply")
    assert (tmp_path / "all.ply").read_bytes() == (tmp_path / "direct.ply").read_bytes()
