"""GPU checks of the mask lifting (voxe_lift_accumulate / voxe_lift_debug_merge, thre3d_reprs.lifting, lift_masks_to_grid.py,
prune_voxel_grid_by_region.py, export_mesh.py --region): agreement with the float64 restatement tests/lift_ref.py within a
per-voxel budget, the contract's bit-level properties in both merge modes, exact identities of the fixed-point sums, the bounds
the shipped visibility kernel gives on the same inputs, no interference with a forward / backward, edge cases, the two-ball scene
and the entry points on the golden checkpoint.  The inputs come from tests/test_lift_host.py, which checks on the host that they
are not vacuous and that the budget catches broken restatements."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import lift_ref
import test_lift_host as H
from conftest import GOLDEN, ROOT
from test_mesh_host import parse_ply
from voxe_hip import abi, ops, workload
from voxe_hip.runtime import VoxeError

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ONE = float(1 << 32)


def _lift(spec, params, dens, ro, rd, values, jitter=None, rng=(0, 0), wv=True, w=True, out=None):
    """(sum_wv, sum_w) int64 of one call; values None = coverage only; `out` = a pair to accumulate into"""
    if out is None:
        C = 1 if values is None else values.shape[1]
        out = (torch.zeros((*dens.shape[:3], C), dtype=torch.int64, device=DEV),
               torch.zeros(dens.shape[:3], dtype=torch.int64, device=DEV))
    give = values is not None and wv
    ops.lift_accumulate_(spec, params, dens, ro, rd, values if give else None, out[0] if give else None, out[1] if w else None,
                         jitter=jitter, rng=rng)
    return out


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.fixture(autouse=True)
def _shipped_merge_mode():
    yield
    ops.lift_debug_merge(ops.LIFT_MERGE_SHIPPED)


# ---- 1: agreement with the restatement --------------------------------------------------------------------------------
_REF = {}


def _reference(case, pre, post):
    """the case's inputs, its probe-based restatement at C = 3 and the visibility grid, computed once; channel 0 of the values
    serves the C = 1 runs (a channel's sums do not depend on the others)"""
    key = (case[0], pre, post)
    if key not in _REF:
        spec, params, dens, feat, ro, rd, jitter, rng = H.lift_inputs(case, pre, post, DEV)
        values = H.lift_values(case, 3, ro.shape[0], DEV)
        ref = lift_ref.lift(spec, params, dens, feat, ro, rd, values, jitter, rng)
        _REF[key] = ((spec, params, dens, ro, rd, jitter, rng), values, ref)
    return _REF[key]


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("pre,post", H.ACTS)
@pytest.mark.parametrize("case", H.lift_cases(), ids=lambda c: c[0])
def test_lift_matches_the_restatement(case, pre, post, channels):
    """|kernel - restatement| <= n_c (1e-5 max|v| + 2^-33) per voxel and channel (lift_ref.budget).  Largest error / budget
    ratio seen on an MI355X over all cases: see profiles/lift_bench.txt."""
    (spec, params, dens, ro, rd, jitter, rng), values, (rwv, rw, nc) = _reference(case, pre, post)
    values = values[:, :channels].contiguous()
    rwv = rwv[..., :channels]
    H.assert_lift_not_vacuous(rw)
    swv, sw = _lift(spec, params, dens, ro, rd, values, jitter, rng)
    got_wv, got_w = swv.double() / ONE, sw.double() / ONE
    vmax = float(values.abs().max())
    ratio_w, ratio_wv = lift_ref.worst_ratio(got_w, rw, nc, 1.0), lift_ref.worst_ratio(got_wv, rwv, nc, vmax)
    print(f"LIFT_RATIO {case[0]} acts=({pre},{post}) C={channels}: sum_w {ratio_w:.4f}  sum_wv {ratio_wv:.4f} of the budget; "
          f"max n_c {int(nc.max())}  max weight {float(rw.max()):.4f}")
    assert bool(((got_w - rw).abs() <= lift_ref.budget(nc, 1.0)).all())
    assert bool(((got_wv - rwv).abs() <= lift_ref.budget(nc, vmax)[..., None]).all())
    assert bool((sw[rw == 0] == 0).all()) and bool((swv[rwv == 0] == 0).all())
    assert int(sw.min()) >= 0 and bool((swv.abs() <= sw[..., None]).all())


# ---- 2: contract properties, all bit for bit --------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [ops.LIFT_MERGE_SHIPPED, ops.LIFT_MERGE_PER_LANE, ops.LIFT_MERGE_WAVE])
def test_order_launch_split_and_accumulation_do_not_change_a_bit(mode):
    ops.lift_debug_merge(mode)
    hw, K, S = 24, 3, 64
    g = torch.Generator().manual_seed(3)
    dens = (torch.empty((*H.DIMS, 1)).uniform_(-1, 1, generator=g) * 1.5).to(DEV)
    spec = ops.GridSpec(aabb=H.AABB, density_scale=2.0)
    ro, rd = H.cameras(hw, K, DEV)
    R, per = ro.shape[0], hw * hw
    jitter = torch.rand((R, S), generator=g).to(DEV)
    values = torch.empty((R, 3)).uniform_(-1, 1, generator=g).to(DEV)
    kw = dict(num_samples=S, near=workload.NEAR, far=workload.FAR, perturb=True)
    multi = ops.RenderParams(image_width=hw, image_height=hw, **kw)
    base = _lift(spec, multi, dens, ro, rd, values, jitter)
    assert int(base[1].max()) > 0.01 * ONE and int(base[0].abs().max()) > 0.01 * ONE
    # the same call twice
    assert _same(base, _lift(spec, multi, dens, ro, rd, values, jitter))
    # K launches into the same buffers
    one = ops.RenderParams(image_width=hw, **kw)
    split = None
    for k in range(K):
        s = slice(k * per, (k + 1) * per)
        split = _lift(spec, one, dens, ro[s].contiguous(), rd[s].contiguous(), values[s].contiguous(), jitter[s].contiguous(),
                      out=split)
    assert _same(base, split)
    # no image fields: linear order
    assert _same(base, _lift(spec, ops.RenderParams(**kw), dens, ro, rd, values, jitter))
    # shuffled rays, the value and jitter rows permuted along
    perm = torch.randperm(R, generator=g).to(DEV)
    shuf = _lift(spec, ops.RenderParams(**kw), dens, ro[perm].contiguous(), rd[perm].contiguous(), values[perm].contiguous(),
                 jitter[perm].contiguous())
    assert _same(base, shuf)
    # no jitter at all (perturb off): the same properties without a caller stream
    off = dict(kw, perturb=False)
    a = _lift(spec, ops.RenderParams(image_width=hw, image_height=hw, **off), dens, ro, rd, values)
    b = _lift(spec, ops.RenderParams(**off), dens, ro[perm].contiguous(), rd[perm].contiguous(), values[perm].contiguous())
    assert _same(a, b) and not torch.equal(a[1], base[1])
    # accumulation onto pre-filled buffers
    pre = (torch.randint(-10 ** 12, 10 ** 12, (*H.DIMS, 3), generator=g).to(DEV), torch.randint(0, 10 ** 12, H.DIMS, generator=g).to(DEV))
    onto = _lift(spec, multi, dens, ro, rd, values, jitter, out=(pre[0].clone(), pre[1].clone()))
    assert torch.equal(onto[0], pre[0] + base[0]) and torch.equal(onto[1], pre[1] + base[1])
    # one NULL output leaves the other as it is with both; coverage only
    only_wv = _lift(spec, multi, dens, ro, rd, values, jitter, w=False)
    only_w = _lift(spec, multi, dens, ro, rd, values, jitter, wv=False)
    cover = _lift(spec, multi, dens, ro, rd, None, jitter)
    assert torch.equal(only_wv[0], base[0]) and int(only_wv[1].count_nonzero()) == 0
    assert torch.equal(only_w[1], base[1]) and int(only_w[0].count_nonzero()) == 0
    assert torch.equal(cover[1], base[1]) and int(cover[0].count_nonzero()) == 0


def test_merge_modes_return_identical_bits():
    """per lane == wave merge == shipped, in image order (lanes of a wave share cells), in linear order, with every ray through
    one cell, and for C = 1, 3 and 8"""
    hw, S = 40, 96                     # 40 px: partial 16-px tiles
    g = torch.Generator().manual_seed(11)
    dens = (torch.empty((*H.DIMS, 1)).uniform_(-1, 1, generator=g) * 1.5).to(DEV)
    spec = ops.GridSpec(aabb=H.AABB, density_scale=2.0)
    ro, rd = H.cameras(hw, 1, DEV)
    same = (ro[:1].expand(700, 3).contiguous(), rd[hw * hw // 2 + hw // 2][None].expand(700, 3).contiguous())
    for name, (o, d), width in (("image", (ro, rd), hw), ("linear", (ro, rd), 0), ("one_ray", same, 0)):
        for C in (1, 3, 8):
            values = torch.empty((o.shape[0], C)).uniform_(-1, 1, generator=g).to(DEV)
            params = ops.RenderParams(num_samples=S, near=workload.NEAR, far=workload.FAR, image_width=width)
            got = []
            for mode in (ops.LIFT_MERGE_PER_LANE, ops.LIFT_MERGE_WAVE, ops.LIFT_MERGE_SHIPPED):
                ops.lift_debug_merge(mode)
                got.append(_lift(spec, params, dens, o, d, values))
            assert int(got[0][1].max()) > 0, (name, C)
            assert _same(got[0], got[1]) and _same(got[0], got[2]), (name, C)
    for bad in (3, -1):
        with pytest.raises(VoxeError, match=str(abi.ERR_BAD_SHAPE)):
            ops.lift_debug_merge(bad)


# ---- 3: exact identities of the fixed-point sums ------------------------------------------------------------------------
def test_exact_identities():
    case = H.lift_cases()[1]
    spec, params, dens, _, ro, rd, jitter, rng = H.lift_inputs(case, *H.ACTS[0], DEV)
    R = ro.shape[0]

    def run(values):
        return _lift(spec, params, dens, ro, rd, values.to(DEV), jitter, rng)

    ones = run(torch.ones(R, 3))
    assert int(ones[1].max()) > 0.01 * ONE
    for ch in range(3):
        assert torch.equal(ones[0][..., ch], ones[1])                       # q(a * 1) == q(a)
    zeros = run(torch.zeros(R, 2))
    assert int(zeros[0].count_nonzero()) == 0 and torch.equal(zeros[1], ones[1])
    g = torch.Generator().manual_seed(4)
    hot = torch.nn.functional.one_hot(torch.randint(0, 8, (R,), generator=g), 8).float()
    lab = run(hot)
    assert torch.equal(lab[0].sum(-1), lab[1]) and int(lab[0].min()) >= 0 and int((lab[0] > 0).any(dim=-1).sum()) > 100
    v = torch.empty((R, 3)).uniform_(-1, 1, generator=g)
    pos, neg = run(v), run(-v)
    assert torch.equal(neg[0], -pos[0]) and torch.equal(neg[1], pos[1]) and int(pos[0].abs().max()) > 0


# ---- 4: against the shipped visibility kernel on the same inputs ----------------------------------------------------------
@pytest.mark.parametrize("case", [H.lift_cases()[0], H.lift_cases()[4]], ids=lambda c: c[0])
def test_sums_are_bounded_by_the_visibility_grid(case):
    pre, post = H.ACTS[1]
    (spec, params, dens, ro, rd, jitter, rng), _, (_, _, nc) = _reference(case, pre, post)
    mw = torch.zeros(dens.shape[:3], device=DEV)
    ops.visibility_accumulate_(spec, params, dens, ro, rd, mw, None, jitter=jitter, rng=rng)
    _, sw = _lift(spec, params, dens, ro, rd, None, jitter, rng)
    qmax = torch.round(mw.double() * ONE).to(torch.int64)      # (a float32 times 2^32 is exact in float64: q of the largest term)
    assert int((mw == 0).sum()) > 100 and float(mw.max()) >= 0.01
    assert bool((sw[mw == 0] == 0).all())
    assert bool((sw >= qmax).all())
    assert bool((sw <= nc * qmax).all())


# ---- 5: non-interference ------------------------------------------------------------------------------------------------
def test_no_interference_with_a_forward_and_its_deterministic_backward():
    g = torch.Generator().manual_seed(8)
    dens0 = torch.empty((40, 40, 40, 1)).uniform_(-1, 1, generator=g).to(DEV)
    feat0 = torch.empty((40, 40, 40, 3)).uniform_(-1, 1, generator=g).to(DEV)
    spec = ops.GridSpec(aabb=((-1.5, 1.5),) * 3, density_scale=3.0)
    ro, rd = H.cameras(64, 1, DEV)
    params = ops.RenderParams(num_samples=64, near=workload.NEAR, far=workload.FAR, perturb=True, white_bkgd=True, image_width=64,
                              deterministic=True)
    g_col = torch.rand((ro.shape[0], 3), generator=torch.Generator().manual_seed(2)).to(DEV)
    values = torch.rand((ro.shape[0], 3), generator=torch.Generator().manual_seed(3)).to(DEV)
    runs = []
    for with_lift in (False, True):
        d, f = dens0.clone().requires_grad_(True), feat0.clone().requires_grad_(True)
        ws = ops.Workspace()
        col = ops.render(spec, params, d, f, ro, rd, workspace=ws, rng=(3, 4))[0]
        if with_lift:
            swv, sw = _lift(spec, params, d, ro, rd, values, rng=(3, 4))
            assert int(sw.max()) > 0
        (col * g_col).sum().backward()
        runs.append((col.detach().clone(), d.grad.clone(), f.grad.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert float(runs[0][1].abs().max()) > 0


# ---- 6: edge cases ------------------------------------------------------------------------------------------------------
def test_edge_cases():
    g = torch.Generator().manual_seed(5)
    dens = torch.empty((*H.DIMS, 1)).uniform_(-1, 1, generator=g).to(DEV)
    spec = ops.GridSpec(aabb=H.AABB, density_scale=2.0)
    ro, rd = H.cameras(24, 1, DEV)
    params = ops.RenderParams(num_samples=64, near=workload.NEAR, far=workload.FAR, image_width=24)
    values = torch.ones((ro.shape[0], 2), device=DEV)
    # R = 0: nothing is touched
    e = torch.zeros((0, 3), device=DEV)
    swv, sw = _lift(spec, params, dens, e, e, torch.zeros((0, 2), device=DEV))
    assert int(swv.count_nonzero()) == 0 and int(sw.count_nonzero()) == 0
    # rays that miss the box
    swv, sw = _lift(spec, params, dens, ro + torch.tensor([50.0, 0.0, 0.0], device=DEV), rd, values)
    assert int(swv.count_nonzero()) == 0 and int(sw.count_nonzero()) == 0
    # a NaN density voxel: no crash, outputs finite (integers) and within a ray's total weight per contribution
    base = _lift(spec, params, dens, ro, rd, values)
    bad = dens.clone()
    bad[13, 10, 11, 0] = float("nan")
    swv, sw = _lift(spec, params, bad, ro, rd, values)
    torch.cuda.synchronize()
    assert int(sw.min()) >= 0 and int(sw.max()) <= int(base[1].max()) * 2 + int(ONE) and torch.equal(swv[..., 0], sw)
    assert int(sw.count_nonzero()) > 0 and not torch.equal(sw, base[1])
    # shape / dtype / pairing errors are raised, not launched
    X, Y, Z = H.DIMS
    i64 = dict(dtype=torch.int64, device=DEV)
    with pytest.raises(VoxeError):
        ops.lift_accumulate_(spec, params, dens, ro, rd, values, torch.zeros((X, Y, Z, 3), **i64), torch.zeros((X, Y, Z), **i64))
    with pytest.raises(VoxeError):
        ops.lift_accumulate_(spec, params, dens, ro, rd, values, torch.zeros((X, Y, Z, 2), **i64), torch.zeros((X, Y, Z), device=DEV))
    with pytest.raises(VoxeError):
        ops.lift_accumulate_(spec, params, dens, ro, rd, values, None, torch.zeros((X, Y, Z), **i64))
    with pytest.raises(VoxeError):
        ops.lift_accumulate_(spec, params, dens, ro, rd, values[:5], torch.zeros((X, Y, Z, 2), **i64), None)
    with pytest.raises(VoxeError):
        ops.lift_accumulate_(spec, params, dens, ro, rd, torch.ones((ro.shape[0], 9), device=DEV), torch.zeros((X, Y, Z, 9), **i64), None)
    with pytest.raises(VoxeError):
        ops.lift_accumulate_(spec, params, dens, ro, rd, values, torch.zeros((X, Y, Z, 2), dtype=torch.int64), None)   # host tensor


# ---- 7: the two-ball scene ----------------------------------------------------------------------------------------------
def test_two_ball_labels_on_the_device():
    from thre3d_atom.thre3d_reprs.lifting import Lifted, region_labels, remove_mask

    spec, params, dens, views = H.two_ball_setup(DEV)
    out = None
    for ro, rd, mask in views:
        out = _lift(spec, params, dens, ro, rd, mask, out=out)
    lifted = Lifted(*out)
    labels = region_labels(lifted)
    H.assert_two_ball_labels(labels)
    # ... and what would be removed: skin of B, nothing of A's band, no unseen voxel
    rm = remove_mask(labels, 1)
    _, da, db = H.two_ball_field()
    band_a = ((da > H.TB_R0 - H.TB_BAND[1]) & (da < H.TB_R0 - H.TB_BAND[0])).to(DEV)
    band_b = ((db > H.TB_R0 - H.TB_BAND[1]) & (db < H.TB_R0 - H.TB_BAND[0])).to(DEV)
    assert rm.dtype == torch.uint8 and int(rm[band_a].sum()) == 0 and int(rm[labels == 0].sum()) == 0
    assert int(rm[band_b].sum()) >= 0.9 * int(band_b.sum())
    assert torch.equal(remove_mask(labels, 0), (labels == 1).to(torch.uint8)) and int(rm.sum()) < int((labels == 1).sum())


# ---- 8: entry points on the golden checkpoint ---------------------------------------------------------------------------
def _load_cli(name):
    spec = importlib.util.spec_from_file_location(name[:-3] + "_lift_gpu_cli", os.path.join(ROOT, name))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _load_model(path):
    from thre3d_atom.modules.volumetric_model import create_volumetric_model_from_saved_model
    from thre3d_atom.thre3d_reprs.voxels import create_voxel_grid_from_saved_info_dict

    return create_volumetric_model_from_saved_model(path, create_voxel_grid_from_saved_info_dict, device=DEV)


def test_lift_prune_and_mesh_clis_on_the_checkpoint(tmp_path):
    from click.testing import CliRunner
    from PIL import Image

    from thre3d_atom.data.datasets import InMemoryPosedImages
    from thre3d_atom.thre3d_reprs.lifting import load_region
    from thre3d_atom.thre3d_reprs.poses import write_camera_params
    from thre3d_atom.thre3d_reprs.visibility import prune_voxel_grid_
    from thre3d_atom.utils.constants import CAMERA_INTRINSICS, EXTRA_ACCUMULATED_WEIGHTS, HEMISPHERICAL_RADIUS
    from thre3d_atom.utils.imaging_utils import CameraBounds, get_thre360_animation_poses

    ckpt = os.path.join(GOLDEN, "ref_checkpoint.pth")
    orig, extra = _load_model(ckpt)
    half, _ = _load_model(ckpt)
    grid = orig.thre3d_repr
    X = grid.densities.shape[0]
    keep = torch.zeros(grid.densities.shape[:3], dtype=torch.bool, device=DEV)
    keep[: X // 2] = True
    prune_voxel_grid_(half.thre3d_repr, keep)                          # half the object: x below the middle
    intr = extra[CAMERA_INTRINSICS]
    poses = get_thre360_animation_poses(extra[HEMISPHERICAL_RADIUS], 60.0, 6)
    (tmp_path / "data" / "train").mkdir(parents=True)
    (tmp_path / "masks").mkdir()
    kw = dict(num_samples_per_ray=64, perturb_sampled_points=False)
    fractions = []
    for i, pose in enumerate(poses):
        acc = half.render(pose, intr, **kw).extra[EXTRA_ACCUMULATED_WEIGHTS].detach().reshape(int(intr.height), int(intr.width)).cpu()
        mask = acc > 0.5 * float(acc.max())
        fractions.append(float(mask.float().mean()))
        Image.fromarray(np.zeros((int(intr.height), int(intr.width), 3), dtype=np.uint8)).save(tmp_path / "data" / "train" / f"{i:04d}.png")
        if i % 2:       # greyscale and RGBA (alpha) masks, mixed
            Image.fromarray((mask.numpy() * 255).astype(np.uint8)).save(tmp_path / "masks" / f"{i:04d}.png")
        else:
            rgba = np.zeros((int(intr.height), int(intr.width), 4), dtype=np.uint8)
            rgba[..., 3] = mask.numpy() * 255
            Image.fromarray(rgba).save(tmp_path / "masks" / f"{i:04d}.png")
    assert 0.01 < min(fractions) and max(fractions) < 0.9, fractions
    pose34 = torch.stack([torch.cat([torch.as_tensor(p.rotation).reshape(3, 3), torch.as_tensor(p.translation).reshape(3, 1)], dim=1)
                          for p in poses]).float()
    near, far = orig.render_config.camera_bounds
    data = InMemoryPosedImages(torch.zeros(len(poses), 3, int(intr.height), int(intr.width)), pose34, intr,
                               CameraBounds(float(near), float(far)))
    write_camera_params(tmp_path / "data" / "train_camera_params.json", data, pose34)

    lift = _load_cli("lift_masks_to_grid.py")
    base = ["-i", ckpt, "-d", str(tmp_path / "data"), "-m", str(tmp_path / "masks"), "--overridden_num_samples_per_ray", "64"]
    res = CliRunner().invoke(lift.main, base + ["-o", str(tmp_path / "first.pth")])
    assert res.exit_code == 0, (res.output, res.exception)
    first = load_region(tmp_path / "first.pth", grid)
    assert first["num_views"] == len(poses) and first["threshold"] == 0.5 and first["min_weight"] == 1e-3
    # every voxel of this small dense grid weighs more than the default min_weight in some view: the second run takes the median
    # weight of the first as its min_weight, which leaves half the voxels unseen
    level = float(first["weight"].median())
    res = CliRunner().invoke(lift.main, base + ["-o", str(tmp_path / "region.pth"), "--min_weight", repr(level)])
    assert res.exit_code == 0, (res.output, res.exception)
    print(res.output.strip())
    n0, n1, n2 = (int(v) for v in re.search(r"unseen (\d+)\s+voted out (\d+)\s+voted in (\d+)", res.output).groups())
    assert re.search(rf"{len(poses)} views", res.output) and re.search(r"lift [\d.]+ ms", res.output)
    region = load_region(tmp_path / "region.pth", grid)
    labels = region["labels"]
    assert (n0, n1, n2) == tuple(int((labels == v).sum()) for v in (0, 1, 2)) and min(n0, n1, n2) > 0
    assert torch.equal(region["weight"], first["weight"])                               # the same bits, run after run
    assert torch.equal(labels == 0, region["weight"] <= level)
    seen = labels != 0
    assert torch.equal(labels[seen] == 2, region["mean"][..., 0][seen] >= 0.5)
    assert bool(torch.isnan(region["mean"][~seen]).all())
    # the masks show the half below the middle: most voted-in voxels lie there, most voted-out ones beyond
    xs = torch.arange(X)[:, None, None].expand_as(labels)
    assert float((xs[labels == 2] < X // 2).float().mean()) > 0.5 and float((xs[labels == 1] >= X // 2).float().mean()) > 0.5
    # a missing mask names the file
    os.remove(tmp_path / "masks" / "0003.png")
    res = CliRunner().invoke(lift.main, base + ["-o", str(tmp_path / "none.pth")])
    assert res.exit_code != 0 and "0003.png" in res.output and not (tmp_path / "none.pth").exists()

    # pruning by the region lowers label-1 voxels only, and the output loads
    prune = _load_cli("prune_voxel_grid_by_region.py")
    d0 = grid.densities.detach()[..., 0].cpu()
    changed = {}
    for dilate in (0, 1):
        out = tmp_path / f"pruned{dilate}.pth"
        res = CliRunner().invoke(prune.main, ["-i", ckpt, "--region", str(tmp_path / "region.pth"), "-o", str(out),
                                              "--region_dilate", str(dilate)])
        assert res.exit_code == 0, (res.output, res.exception)
        new, extra2 = _load_model(out)
        d1 = new.thre3d_repr.densities.detach()[..., 0].cpu()
        assert torch.equal(new.thre3d_repr.features, grid.features) and extra2.keys() == extra.keys()
        assert bool((d1 <= d0).all()) and bool((d1[labels != 1] == d0[labels != 1]).all())
        changed[dilate] = int((d1 != d0).sum())
    assert 0 < changed[0] <= n1 and changed[1] <= changed[0]
    res = CliRunner().invoke(prune.main, ["-i", ckpt, "--region", str(tmp_path / "region.pth"), "-o", str(tmp_path / "x.pth"),
                                          "--region_dilate", "4"])
    assert res.exit_code != 0

    # the mesh without the voted-out voxels
    exp = _load_cli("export_mesh.py")
    res = CliRunner().invoke(exp.main, ["-i", ckpt, "-o", str(tmp_path / "all.ply")])
    assert res.exit_code == 0, (res.output, res.exception)
    res = CliRunner().invoke(exp.main, ["-i", ckpt, "-o", str(tmp_path / "in.ply"), "--region", str(tmp_path / "region.pth")])
    assert res.exit_code == 0, (res.output, res.exception)
    t_all, t_in = len(parse_ply(tmp_path / "all.ply")[2]), len(parse_ply(tmp_path / "in.ply")[2])
    print(f"triangles: {t_all} without --region, {t_in} with")
    assert 0 < t_in < t_all
