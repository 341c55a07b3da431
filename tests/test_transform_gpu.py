"""GPU checks of the grid transform (voxe_grid_resample, thre3d_reprs.transform, transform_voxel_grid.py): the kernel against the
float64 restatement tests/transform_ref.py with that restatement in float32 as the yardstick, exact lattice-preserving maps,
the UNION mode, render equivalence through the public API, the command-line tool on the golden checkpoint and no interference
with a forward / backward.  The inputs come from tests/test_transform_host.py, which checks on the host that the conventions
hold on the CPU oracle."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import test_transform_host as H
import transform_ref as T
from conftest import GOLDEN, ROOT
from voxe_hip import abi, ops, workload

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SKIP_CAP = 0.01       # share of voxels whose `taken` may go unchecked (u within 1e-4 of a hull boundary, ties of the UNION)


def _grid(dims, channels, seed):
    g = torch.Generator().manual_seed(seed)
    dens = torch.randn((*dims, 1), generator=g) * 2.0
    feat = torch.randn((*dims, channels), generator=g)
    return dens, feat


def _maps(dims_s, dims_d):
    """(name, A, b, R) of the two maps of check 6 between lattices of anisotropic voxels: a generic rotation / translation /
    scale, and the identity onto a shifted, finer lattice (which runs past the source: whole rows of fill)"""
    v_s = (0.21, 0.33, 0.17)
    lo_s = tuple(-(n * e) / 2 for n, e in zip(dims_s, v_s))
    out = []
    # generic: the destination covers about the source's extent, scaled by 1.3
    v_d = tuple(1.3 * (n * e) / m for n, e, m in zip(dims_s, v_s, dims_d))
    lo_d = tuple(-(m * e) / 2 + c for m, e, c in zip(dims_d, v_d, (0.03, -0.02, 0.04)))
    out.append(("generic",) + T.index_map(dims_s, lo_s, v_s, dims_d, lo_d, v_d, H.GENERIC_R, (0.05, -0.04, 0.02), 1.3)
               + (H.GENERIC_R,))
    v_f = tuple(0.45 * e for e in v_s)
    lo_f = tuple(l + 0.37 * e for l, e in zip(lo_s, v_s))
    out.append(("finer",) + T.index_map(dims_s, lo_s, v_s, dims_d, lo_f, v_f, np.eye(3), (0.0, 0.0, 0.0), 1.0) + (np.eye(3),))
    return out


def _run(dens, feat, xf, dims_d, **kw):
    d, f, taken = ops.grid_resample(None if dens is None else dens.to(DEV), None if feat is None else feat.to(DEV), xf,
                                    dst_dims=dims_d, want_taken=True, **kw)
    torch.cuda.synchronize()
    return (None if d is None else d.cpu()), (None if f is None else f.cpu()), taken.cpu()


def _assert_close(name, got, ref64, yard32):
    """the kernel's max abs error against float64 is at most 4x the float32 restatement's, floor 1e-6 * max|value|"""
    err, yard = float((got.double() - ref64).abs().max()), float((yard32.double() - ref64).abs().max())
    bound = max(4.0 * yard, 1e-6 * float(ref64.abs().max()))
    print(f"  {name}: kernel {err:.3e}  float32 restatement {yard:.3e}  bound {bound:.3e}")
    assert err <= bound, name


# ---- 6: kernel vs restatement -------------------------------------------------------------------------------------------------
SHAPES = [((1, 5, 7), (3, 4, 65)), ((13, 9, 17), (11, 15, 10)), ((13, 9, 17), (11, 15, 1)), ((13, 9, 17), (6, 5, 63))]
CHANNELS = [(-1, 1), (-1, 5), (0, 3), (1, 12), (2, 27), (3, 48)]


@pytest.mark.parametrize("degree,channels", CHANNELS, ids=lambda v: str(v))
@pytest.mark.parametrize("dims_s,dims_d", SHAPES, ids=lambda v: "x".join(str(n) for n in v))
def test_kernel_matches_the_restatement(dims_s, dims_d, degree, channels):
    from thre3d_atom.thre3d_reprs.transform import sh_rotation_matrices

    dens, feat = _grid(dims_s, channels, seed=sum(dims_s) + channels)
    fill = -1.25
    taken_total = 0
    for name, A, b, R in _maps(dims_s, dims_d):
        blocks = sh_rotation_matrices(R, degree)
        A32, b32 = T.as_kernel_args(A, b)
        blocks32 = [np.asarray(m, np.float32).astype(np.float64) for m in blocks]
        for pre in (abi.ACT_IDENTITY, abi.ACT_ABS):
            xf = ops.make_resample(A, b, blocks, degree, pre, fill, abi.RESAMPLE_REPLACE)
            got_d, got_f, got_t = _run(dens, feat, xf, dims_d)
            kw = dict(blocks=blocks32, sh_degree=degree, pre_abs=pre == abi.ACT_ABS, fill=fill)
            ref = T.resample(dens, feat, dims_d, A32, b32, **kw)
            yard = T.resample(dens, feat, dims_d, A32, b32, dtype=torch.float32, **kw)
            print(f"{name} pre {pre}: taken {int(ref['taken'].sum())}/{ref['taken'].numel()}")
            _assert_close("densities", got_d, ref["densities"], yard["densities"])
            _assert_close("features", got_f, ref["features"], yard["features"])
            skip = T.near_hull(ref["u"], dims_s)
            assert float(skip.float().mean()) <= SKIP_CAP
            assert torch.equal(got_t.bool()[~skip], ref["taken"][~skip])
            taken_total += int(ref["taken"].sum())
            if name == "finer":   # rows of the destination past the source: exactly the fill values
                outside = (ref["u"] < -1).any(dim=-1) | torch.stack([ref["u"][..., a] > dims_s[a] for a in range(3)]).any(dim=0)
                assert int(outside.sum()) > 0 or dims_d[2] < 63
                assert bool((got_d[outside] == fill).all()) and bool((got_f[outside] == 0).all()) and not bool(got_t[outside].any())
    assert taken_total > 0
    # one pair alone: the other tensors are not needed
    name, A, b, R = _maps(dims_s, dims_d)[1]
    xf = ops.make_resample(A, b, sh_rotation_matrices(R, degree), degree, abi.ACT_IDENTITY, fill, abi.RESAMPLE_REPLACE)
    both = _run(dens, feat, xf, dims_d)
    only_d, only_f = _run(dens, None, xf, dims_d), _run(None, feat, xf, dims_d)
    assert only_d[1] is None and torch.equal(only_d[0], both[0]) and torch.equal(only_d[2], both[2])
    assert only_f[0] is None and torch.equal(only_f[1], both[1]) and torch.equal(only_f[2], both[2])


# ---- 7: exact cases -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", [0, 1, 2, 3])
@pytest.mark.parametrize("case", T.lattice_cases(), ids=lambda c: c[0])
def test_lattice_preserving_maps_are_exact_on_the_device(case, degree):
    from thre3d_atom.thre3d_reprs.transform import sh_rotation_matrices

    _, R, shift = case
    dens, feat = H.lattice_inputs(degree)
    dims_d, _, _, A, b = T.lattice_setup(H.LATTICE_DIMS, H.LATTICE_EDGES, R, shift)
    blocks = sh_rotation_matrices(R, degree)
    fill = -1.5
    xf = ops.make_resample(A, b, blocks, degree, abi.ACT_IDENTITY, fill, abi.RESAMPLE_REPLACE)
    got_d, got_f, got_t = _run(dens, feat, xf, dims_d)
    want_d = torch.from_numpy(T.permute_by(dens.numpy(), R, shift, fill))
    want_f = torch.from_numpy(T.permute_by(feat.numpy(), R, shift, 0.0))
    want_t = torch.from_numpy(T.permute_by(np.ones((*H.LATTICE_DIMS, 1), np.uint8), R, shift, 0)[..., 0])
    assert torch.equal(got_d, want_d) and torch.equal(got_t, want_t)
    if degree == 0:
        assert torch.equal(got_f, want_f)
    else:
        rotated = T.rotate_coefficients(want_f.double(), blocks, degree)
        err = float((got_f.double() - rotated).abs().max())
        print(f"degree {degree}: max |features - rotated permutation| {err:.2e}")
        assert err <= 1e-6
        assert float((rotated - want_f.double()).abs().max()) > 0.1      # (the rotation does something)


# ---- 8: UNION -----------------------------------------------------------------------------------------------------------------
def _union_inputs(pre):
    """a carved ball (source, 16^3, SH-1) and a carved box (destination, 20 x 18 x 22) of the same field type"""
    g = torch.Generator().manual_seed(31 + pre)
    dims_s, dims_d = (16, 16, 16), (20, 18, 22)
    c = [2 * (torch.arange(n) + 0.5) / n - 1 for n in dims_s]
    r = torch.sqrt(c[0][:, None, None] ** 2 + c[1][None, :, None] ** 2 + c[2][None, None, :] ** 2)
    src_d = torch.where(r < 0.8, 3.0 * (1.0 - r) + 0.2, torch.zeros(())).float()[..., None]
    box = torch.ones(dims_d, dtype=torch.bool)
    for a, n in enumerate(dims_d):
        inside = (2 * (torch.arange(n) + 0.5) / n - 1).abs() < 0.6
        box &= inside.reshape([-1 if k == a else 1 for k in range(3)])
    # (outside the box a thin haze, not 0: a source sample of exactly 0 against a destination of exactly 0 would be a tie)
    dst_d = torch.where(box, torch.empty(dims_d).uniform_(0.5, 2.0, generator=g), torch.full((), 0.05))[..., None]
    if pre == abi.ACT_ABS:    # the sign of a raw value does not matter under abs
        src_d = src_d * torch.where(torch.rand(src_d.shape, generator=g) < 0.5, -1.0, 1.0)
        dst_d = dst_d * torch.where(torch.rand(dst_d.shape, generator=g) < 0.5, -1.0, 1.0)
    src_f, dst_f = torch.randn((*dims_s, 12), generator=g), torch.randn((*dims_d, 12), generator=g)
    v_s, v_d = (0.11, 0.12, 0.10), (0.15, 0.16, 0.13)
    lo_s = tuple(-(n * e) / 2 for n, e in zip(dims_s, v_s))
    lo_d = tuple(-(n * e) / 2 for n, e in zip(dims_d, v_d))
    A, b = T.index_map(dims_s, lo_s, v_s, dims_d, lo_d, v_d, H.GENERIC_R, (0.3, -0.2, 0.25), 1.2)
    return src_d, src_f, dst_d, dst_f, A, b


@pytest.mark.parametrize("pre", [abi.ACT_IDENTITY, abi.ACT_ABS])
def test_union_composes_a_ball_into_a_box(pre):
    from thre3d_atom.thre3d_reprs.transform import sh_rotation_matrices

    src_d, src_f, dst_d, dst_f, A, b = _union_inputs(pre)
    blocks = sh_rotation_matrices(H.GENERIC_R, 1)
    xf = ops.make_resample(A, b, blocks, 1, pre, 0.0, abi.RESAMPLE_UNION)
    out_d, out_f = dst_d.to(DEV).clone(), dst_f.to(DEV).clone()
    ret_d, ret_f, taken = ops.grid_resample(src_d.to(DEV), src_f.to(DEV), xf, dst_densities=out_d, dst_features=out_f, want_taken=True)
    torch.cuda.synchronize()
    assert ret_d is out_d and ret_f is out_f
    out_d, out_f, taken = out_d.cpu(), out_f.cpu(), taken.cpu().bool()
    A32, b32 = T.as_kernel_args(A, b)
    kw = dict(blocks=[np.asarray(m, np.float32).astype(np.float64) for m in blocks], sh_degree=1, pre_abs=pre == abi.ACT_ABS,
              mode=T.UNION, dst_d=dst_d, dst_f=dst_f)
    ref = T.resample(src_d, src_f, dst_d.shape[:3], A32, b32, **kw)
    yard = T.resample(src_d, src_f, dst_d.shape[:3], A32, b32, dtype=torch.float32, **kw)
    old = dst_d[..., 0].double().abs() if pre == abi.ACT_ABS else dst_d[..., 0].double()
    skip = T.near_hull(ref["u"], src_d.shape[:3]) | ((ref["new_density"] - old).abs() < 1e-5)
    print(f"taken {int(taken.sum())} of {taken.numel()}  (restatement {int(ref['taken'].sum())}), unchecked {int(skip.sum())}")
    assert float(skip.float().mean()) <= SKIP_CAP
    assert torch.equal(taken[~skip], ref["taken"][~skip])
    assert 100 < int(taken.sum()) < taken.numel()
    # every voxel the source did not take keeps its bits
    assert torch.equal(out_d[~taken], dst_d[~taken]) and torch.equal(out_f[~taken], dst_f[~taken])
    both = taken & ref["taken"] & yard["taken"]
    assert int(both.sum()) > 100
    _assert_close("densities", out_d[both], ref["densities"][both], yard["densities"][both])
    _assert_close("features", out_f[both], ref["features"][both], yard["features"][both])
    with pytest.raises(ops.VoxeError):   # aliasing / missing destination
        ops.grid_resample(out_d.to(DEV), None, xf)


def test_compose_voxel_grids_blends_attention_and_checks_the_fields():
    from thre3d_atom.thre3d_reprs.transform import compose_voxel_grids_
    from thre3d_atom.thre3d_reprs.voxels import VoxelGrid, VoxelSize

    src_d, src_f, dst_d, dst_f, _, _ = _union_inputs(abi.ACT_IDENTITY)
    relu = dict(density_preactivation=torch.nn.Identity(), density_postactivation=torch.nn.ReLU())
    src = VoxelGrid(src_d.to(DEV), src_f.to(DEV), VoxelSize(0.11, 0.12, 0.10), attn=torch.full_like(src_d, 2.0).to(DEV), **relu)
    dst = VoxelGrid(dst_d.to(DEV), dst_f.to(DEV), VoxelSize(0.15, 0.16, 0.13), attn=torch.full_like(dst_d, -1.0).to(DEV), **relu)
    versions = (dst.densities._version, dst.features._version)
    taken = compose_voxel_grids_(dst, src, H.GENERIC_R, (0.3, -0.2, 0.25), 1.2).bool().cpu()
    assert 100 < int(taken.sum()) < taken.numel()
    assert dst.densities._version > versions[0] and dst.features._version > versions[1]
    assert torch.equal(dst.densities.cpu()[~taken], dst_d[~taken]) and torch.equal(dst.features.cpu()[~taken], dst_f[~taken])
    attn = dst.attn.cpu()[..., 0]
    assert bool((attn[~taken] == -1.0).all()) and float((attn[taken] - 2.0).abs().max()) <= 1e-5   # (valid samples: no fill mixed in)
    other = VoxelGrid(src_d.to(DEV), src_f.to(DEV), VoxelSize(0.1, 0.1, 0.1), density_preactivation=torch.nn.Identity(),
                      density_postactivation=torch.nn.Softplus())
    with pytest.raises(ValueError):
        compose_voxel_grids_(dst, other, np.eye(3))
    with pytest.raises(ValueError):
        compose_voxel_grids_(dst, VoxelGrid(src_d.to(DEV), src_f[..., :3].contiguous().to(DEV), VoxelSize(0.1, 0.1, 0.1), **relu),
                             np.eye(3))
    with pytest.raises(ValueError):
        compose_voxel_grids_(dst, VoxelGrid(src_d.to(DEV), src_f.to(DEV), VoxelSize(0.1, 0.1, 0.1), expected_density_scale=2.0,
                                            **relu), np.eye(3))


# ---- 9: render equivalence through the public API -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", H.ORACLE_CASES, ids=lambda c: c[0])
def test_transformed_grid_renders_the_same_image_from_moved_rays(case):
    from thre3d_atom.rendering.volumetric.render_interface import Rays
    from thre3d_atom.thre3d_reprs.renderers import SHVoxGridRenderConfig, render_sh_voxel_grid
    from thre3d_atom.thre3d_reprs.transform import transform_voxel_grid
    from thre3d_atom.thre3d_reprs.voxels import VoxelGrid, VoxelSize
    from thre3d_atom.utils.constants import EXTRA_ACCUMULATED_WEIGHTS
    from thre3d_atom.utils.imaging_utils import CameraBounds

    _, R, shift = case
    degree = 2
    dens, feat = H.oracle_grid(degree)
    grid = VoxelGrid(dens.to(DEV), feat.to(DEV), VoxelSize(*(H.ORACLE_EDGE,) * 3), density_preactivation=torch.nn.Identity(),
                     density_postactivation=torch.nn.ReLU(), attn=torch.randn(dens.shape, generator=torch.Generator().manual_seed(1)).to(DEV))
    dims_d, v_d, t, _, _ = T.lattice_setup(H.ORACLE_DIMS, (H.ORACLE_EDGE,) * 3, R, shift)
    moved = transform_voxel_grid(grid, R, translation=t)
    assert moved.grid_dims == dims_d and tuple(moved.voxel_size) == tuple(v_d) and moved.attn.shape == (*dims_d, 1)
    assert torch.equal(moved.densities.cpu(), torch.from_numpy(T.permute_by(dens.numpy(), R, shift, 0.0)))
    assert torch.equal(moved.attn.cpu(), torch.from_numpy(T.permute_by(grid.attn.cpu().numpy(), R, shift, 0.0)))
    o, d = H.oracle_rays()
    o2, d2 = H.moved_rays(o, d, R, t)
    config = SHVoxGridRenderConfig(num_samples_per_ray=H.ORACLE_S, camera_bounds=CameraBounds(workload.NEAR, workload.FAR),
                                   perturb_sampled_points=False)
    shape = (H.ORACLE_HW, H.ORACLE_HW)
    with torch.no_grad():
        a = render_sh_voxel_grid(grid, Rays(torch.from_numpy(o).to(DEV), torch.from_numpy(d).to(DEV), shape), config)
        b = render_sh_voxel_grid(moved, Rays(torch.from_numpy(o2).to(DEV), torch.from_numpy(d2).to(DEV), shape), config)
    err_c = float((a.colour - b.colour).abs().max())
    err_a = float((a.extra[EXTRA_ACCUMULATED_WEIGHTS] - b.extra[EXTRA_ACCUMULATED_WEIGHTS]).abs().max())
    print(f"{case[0]}: colour {err_c:.2e} acc {err_a:.2e}")
    assert float(a.extra[EXTRA_ACCUMULATED_WEIGHTS].mean()) >= 0.05 and float(a.colour.std()) >= 0.05
    # each GPU render is within 5e-6 of the oracle, the oracle's pair within 2e-6 of each other (test_transform_host.py)
    assert err_c <= 1.2e-5 and err_a <= 1.2e-5


# ---- 10: the command-line tool on the golden checkpoint -----------------------------------------------------------------------
def _load_cli(name):
    spec = importlib.util.spec_from_file_location(name[:-3] + "_xf_gpu_cli", os.path.join(ROOT, name))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _load_model(path):
    from thre3d_atom.modules.volumetric_model import create_volumetric_model_from_saved_model
    from thre3d_atom.thre3d_reprs.voxels import create_voxel_grid_from_saved_info_dict

    return create_volumetric_model_from_saved_model(path, create_voxel_grid_from_saved_info_dict, device=DEV)


def test_cli_round_trip_on_the_checkpoint(tmp_path):
    from click.testing import CliRunner

    ckpt = os.path.join(GOLDEN, "ref_checkpoint.pth")
    mod = _load_cli("transform_voxel_grid.py")
    assert np.array_equal(mod.rotation_from_options(quarter_turns=("z", 1)), T.quarter_turn("z", 1))
    assert np.array_equal(mod.rotation_from_options(quarter_turns=("x", 3)), T.quarter_turn("x", 3))
    assert np.array_equal(mod.rotation_from_options(mirror="y"), T.mirror("y"))
    assert np.abs(mod.rotation_from_options("y", 30.0) - T.rotation_about("y", 30.0)).max() < 1e-15
    orig, extra = _load_model(ckpt)
    d0, f0 = orig.thre3d_repr.densities.detach().cpu(), orig.thre3d_repr.features.detach().cpu()
    path = ckpt
    for turn in range(4):
        out = tmp_path / f"turn{turn + 1}.pth"
        res = CliRunner().invoke(mod.main, ["-i", str(path), "-o", str(out), "--quarter_turns", "z", "1"])
        assert res.exit_code == 0, (res.output, res.exception)
        path = out
        if turn == 0:
            new, extra2 = _load_model(out)           # the existing loader reads it
            assert extra2.keys() == extra.keys()
            d1 = new.thre3d_repr.densities.detach().cpu()
            assert torch.equal(d1, torch.from_numpy(T.permute_by(d0.numpy(), T.quarter_turn("z", 1), (0, 0, 0), 0.0)))
            assert torch.equal(d1, torch.from_numpy(np.ascontiguousarray(np.rot90(d0.numpy(), 1, axes=(0, 1)))))
            assert not torch.equal(d1, d0)
    back, _ = _load_model(path)
    assert torch.equal(back.thre3d_repr.densities.detach().cpu(), d0)
    assert float((back.thre3d_repr.features.detach().cpu() - f0).abs().max()) <= 1e-6
    # re-gridding keeps the world extent; composing a checkpoint into itself moved changes something and still loads
    res = CliRunner().invoke(mod.main, ["-i", ckpt, "-o", str(tmp_path / "fine.pth"), "--output_dims", "9", "8", "7",
                                        "--rotate_axis", "y", "--rotate_degrees", "20", "--translate", "0.1", "0", "-0.1"])
    assert res.exit_code == 0, (res.output, res.exception)
    fine, _ = _load_model(tmp_path / "fine.pth")
    assert fine.thre3d_repr.grid_dims == (9, 8, 7)
    assert np.allclose([hi - lo for lo, hi in fine.thre3d_repr.aabb], [hi - lo for lo, hi in orig.thre3d_repr.aabb])
    res = CliRunner().invoke(mod.main, ["-i", ckpt, "-o", str(tmp_path / "both.pth"), "--into", ckpt, "--mirror", "x"])
    assert res.exit_code == 0, (res.output, res.exception)
    both, _ = _load_model(tmp_path / "both.pth")
    db = both.thre3d_repr.densities.detach().cpu()
    assert bool((db >= d0).all()) and 0 < int((db != d0).sum()) < d0.numel()
    res = CliRunner().invoke(mod.main, ["-i", ckpt, "-o", str(tmp_path / "bad.pth"), "--mirror", "x", "--quarter_turns", "z", "1"])
    assert res.exit_code != 0


# ---- 11: no interference ------------------------------------------------------------------------------------------------------
def test_no_interference_with_a_forward_and_its_deterministic_backward():
    from test_visibility_host import cameras

    g = torch.Generator().manual_seed(8)
    dens0 = torch.empty((40, 40, 40, 1)).uniform_(-1, 1, generator=g).to(DEV)
    feat0 = torch.empty((40, 40, 40, 3)).uniform_(-1, 1, generator=g).to(DEV)
    spec = ops.GridSpec(aabb=((-1.5, 1.5),) * 3, density_scale=3.0)
    ro, rd = cameras(64, 1, DEV)
    params = ops.RenderParams(num_samples=64, near=workload.NEAR, far=workload.FAR, perturb=True, white_bkgd=True, image_width=64,
                              deterministic=True)
    g_col = torch.rand((ro.shape[0], 3), generator=torch.Generator().manual_seed(2)).to(DEV)
    xf = ops.make_resample(H.GENERIC_R * 1.1, [3.0, 2.0, 1.0], [np.eye(1)], 0)
    grads = []
    for with_resample in (False, True):
        d, f = dens0.clone().requires_grad_(True), feat0.clone().requires_grad_(True)
        ws = ops.Workspace()
        col = ops.render(spec, params, d, f, ro, rd, workspace=ws, rng=(3, 4))[0]
        if with_resample:
            out = ops.grid_resample(d, f, xf, dst_dims=(33, 35, 37), want_taken=True)
            assert int(out[2].sum()) > 1000
        (col * g_col).sum().backward()
        grads.append((d.grad.clone(), f.grad.clone()))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    assert float(grads[0][0].abs().max()) > 0
