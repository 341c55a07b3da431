"""CPU checks of the mask-lifting feature: the C ABI's declarations and argument validation (no device work), the region helpers on
host tensors, the entry points' options and unchanged paths, and -- with the oracle's sample probe feeding the float64 restatement
tests/lift_ref.py -- that the inputs of the GPU tests (tests/test_lift_gpu.py builds them with the functions below) are not
vacuous, that the error budget held there catches three broken restatements, and that the two-ball scene's labels are right in
the restatement alone."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import lift_ref
from conftest import ROOT
from test_visibility_host import ACTS, AABB, BALL_ANGLES, DIMS, agreement_cases, agreement_inputs, cameras, cast  # noqa: F401
from voxe_hip import abi, ops, workload
from voxe_hip.desc import make_grid_desc, make_render_cfg

CPU = torch.device("cpu")
# the frusta overfill this box in y and z (rays cross those faces: footprint corners fall outside the grid) and miss its far end in x
OVERFILL_AABB = ((-0.5, 2.6), (-0.6, 0.5), (-0.5, 0.55))


# ---- inputs shared with the GPU tests ---------------------------------------------------------------------------------
def lift_cases():
    """test_visibility_host.agreement_cases() plus a box the frusta overfill and 1000 shuffled rays (no multiple of 256)"""
    return agreement_cases() + [
        ("overfill", 40, 1, True, None, False, False, "image"),
        ("shuffled1000", 32, 1, True, "caller", False, False, "shuffled"),
    ]


def lift_inputs(case, pre, post, device):
    """(spec, params, densities, features, rays_o, rays_d, jitter, rng) of one case"""
    spec, params, dens, feat, ro, rd, jitter, rng = agreement_inputs(case, pre, post, device)
    if case[0] == "overfill":
        spec = ops.GridSpec(aabb=OVERFILL_AABB, density_scale=2.0, density_pre_act=pre, density_post_act=post)
    if case[0] == "shuffled1000":
        ro, rd, jitter = ro[:1000].contiguous(), rd[:1000].contiguous(), jitter[:1000].contiguous()
    return spec, params, dens, feat, ro, rd, jitter, rng


def lift_values(case, channels, num_rays, device):
    """[R,C] float32 in [-1, 1], a few of them exactly 0, 1 and -1"""
    g = torch.Generator().manual_seed(1000 + 7 * len(case[0]) + channels)
    v = torch.empty((num_rays, channels)).uniform_(-1, 1, generator=g)
    pick = torch.randint(0, 10, (num_rays, channels), generator=g)
    v[pick == 0], v[pick == 1], v[pick == 2] = 0.0, 1.0, -1.0
    return v.to(device)


def assert_lift_not_vacuous(weight):
    assert int((weight == 0).sum()) > 100 and float(weight.max()) >= 0.01


# two opaque balls side by side on a DIMS grid of 0.1 voxels; 8 cameras around them
TB_AABB = ((-1.3, 1.3), (-1.0, 1.0), (-1.15, 1.15))
TB_R0 = 0.45
TB_A, TB_B = (-0.55, 0.05, 0.0), (0.6, -0.1, 0.05)
TB_HW, TB_RADIUS, TB_NEAR, TB_FAR, TB_S = 48, 5.0, 3.0, 7.0, 96
# the skin of a ball: voxel centres this far below its surface.  Shallower voxels share their footprint cells with empty space
# next to the other ball's rays, deeper ones carry little weight
TB_BAND = (0.03, 0.2)
TB_EXEMPT = 0.02


def two_ball_field():
    """(densities [X,Y,Z,1] float32, dist to A's centre, dist to B's centre [X,Y,Z] float64)"""
    axes = [torch.tensor([TB_AABB[a][0] + (i + 0.5) * (TB_AABB[a][1] - TB_AABB[a][0]) / DIMS[a] for i in range(DIMS[a])],
                         dtype=torch.float64) for a in range(3)]
    x, y, z = torch.meshgrid(*axes, indexing="ij")
    da, db = (torch.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) for c in (TB_A, TB_B))
    dens = 40.0 * torch.relu(TB_R0 - da) + 40.0 * torch.relu(TB_R0 - db)
    return dens.to(torch.float32)[..., None], da, db


def _first_hit(ro, rd, centre):
    """depth (in units of |d|) at which each ray enters the ball, +inf for a miss"""
    o = ro.double() - torch.tensor(centre, dtype=torch.float64, device=ro.device)
    d = rd.double()
    a, b, c = (d * d).sum(-1), (o * d).sum(-1), (o * o).sum(-1) - TB_R0 ** 2
    disc = b * b - a * c
    t = (-b - torch.sqrt(disc.clamp_min(0.0))) / a
    return torch.where((disc > 0) & (t > 0), t, torch.full_like(t, float("inf")))


def two_ball_setup(device):
    """(spec, params, densities, [(rays_o, rays_d, mask [R,1])] per camera): the mask is 1 where the ray hits ball A first"""
    spec = ops.GridSpec(aabb=TB_AABB, density_scale=1.0, density_pre_act=abi.ACT_IDENTITY, density_post_act=abi.ACT_RELU)
    params = ops.RenderParams(num_samples=TB_S, near=TB_NEAR, far=TB_FAR, image_width=TB_HW)
    views = []
    for yaw, pitch in BALL_ANGLES:
        ro, rd = cast(TB_HW, yaw, pitch, TB_RADIUS, device)
        ta, tb = _first_hit(ro, rd, TB_A), _first_hit(ro, rd, TB_B)
        views.append((ro, rd, (torch.isfinite(ta) & (ta < tb)).to(torch.float32)[:, None]))
    return spec, params, two_ball_field()[0].to(device), views


def assert_two_ball_labels(labels):
    """skin voxels of A are voted in, skin voxels of B voted out, up to TB_EXEMPT of each band"""
    _, da, db = two_ball_field()
    labels = labels.cpu()
    for name, dist, want in (("A", da, 2), ("B", db, 1)):
        band = (dist > TB_R0 - TB_BAND[1]) & (dist < TB_R0 - TB_BAND[0])
        wrong = int((labels[band] != want).sum())
        print(f"ball {name}: {int(band.sum())} skin voxels, {wrong} not labelled {want}")
        assert int(band.sum()) >= 100 and wrong <= TB_EXEMPT * int(band.sum()), name
    assert int((labels == 0).sum()) > 0     # the corners of the box and the hearts of the balls are unseen


def labels_from_sums(sum_wv, sum_w, threshold=0.5, min_weight=1e-3):
    """region_labels over real-valued sums (the restatement's)"""
    from thre3d_atom.thre3d_reprs.lifting import Lifted, region_labels

    one = float(1 << 32)
    return region_labels(Lifted(torch.round(sum_wv * one).to(torch.int64), torch.round(sum_w * one).to(torch.int64)), threshold,
                         min_weight)


# ---- the inputs are not vacuous; the budget has teeth (oracle probe -> restatement, no device) -------------------------
@pytest.mark.parametrize("pre,post", ACTS)
@pytest.mark.parametrize("case", lift_cases(), ids=lambda c: c[0])
def test_inputs_are_not_vacuous_and_mutants_break_the_budget(case, pre, post):
    spec, params, dens, feat, ro, rd, jitter, rng = lift_inputs(case, pre, post, CPU)
    values = lift_values(case, 3, ro.shape[0], CPU)
    probe = lift_ref.host_probe(spec, params, dens, feat, ro, rd, jitter, rng)
    swv, sw, nc = lift_ref.lift_host(spec, params, dens, feat, ro, rd, values, probe=probe)
    assert_lift_not_vacuous(sw)
    assert bool((nc[sw > 0] > 0).all()) and int(nc[sw == 0].sum()) == 0
    assert float(swv.abs().max()) > 0.01 and bool((swv.abs() <= sw[..., None] + 1e-12).all())
    if case[0] == "overfill":     # corners outside the grid: some sample's footprint leaves it
        z, inside, _ = probe
        p = ro[:, None, :] + rd[:, None, :] * z[:, :, None]
        _, i0, _, _ = lift_ref.normals_ref.index_coords(p.reshape(-1, 3), DIMS, spec.aabb)
        out = ((i0 < 0) | (i0 + 1 >= torch.tensor(DIMS))).any(dim=1) & inside.reshape(-1).bool()
        assert int(out.sum()) > 100
    vmax = float(values.abs().max())
    for mutant in lift_ref.MUTANTS:
        mwv, mw, _ = lift_ref.lift_host(spec, params, dens, feat, ro, rd, values, probe=probe, mutant=mutant)
        ratio = max(lift_ref.worst_ratio(mw, sw, nc, 1.0), lift_ref.worst_ratio(mwv, swv, nc, vmax))
        print(f"{mutant}: worst error / budget {ratio:.3g}")
        assert ratio > 1.0, mutant


def test_two_ball_labels_in_the_restatement():
    spec, params, dens, views = two_ball_setup(CPU)
    feat = torch.zeros((*DIMS, 3))
    out = None
    for ro, rd, mask in views:
        out = lift_ref.lift_host(spec, params, dens, feat, ro, rd, mask, out=out)
        assert 0.02 < float(mask.mean()) < 0.5
    assert_two_ball_labels(labels_from_sums(out[0], out[1]))


# ---- C ABI ------------------------------------------------------------------------------------------------------------
def _lib():
    from voxe_hip import build

    return abi.declare(ctypes.CDLL(build.build()), "voxe_")


def _proto_names(text, start):
    proto = re.search(re.escape(start) + r"\((.*?)\);", text, re.S).group(1)
    proto = re.sub(r"/\*.*?\*/", "", proto, flags=re.S)
    return [re.split(r"[\s*]+", a.strip())[-1] for a in proto.split(",")]


def test_lift_symbols_are_declared_with_no_cpu_twin_and_abi_13():
    text = open(os.path.join(ROOT, "include", "voxe.h")).read()
    L = _lib()
    for name in ("voxe_lift_accumulate", "voxe_lift_debug_merge"):
        assert re.search(rf"\b{name}\s*\(", text) and name in abi.hip_symbols() and hasattr(L, name)
    assert not re.search(r"\bvoxe_cpu_\w*lift", text)
    assert not any("lift" in s for s in abi.cpu_symbols())
    assert "lift" not in open(os.path.join(ROOT, "oracle", "voxe_cpu.c")).read()
    assert abi.ABI_VERSION == 13 and "#define VOXE_ABI_VERSION 13" in text and L.voxe_abi_version() == 13
    assert "voxe_lift.hip" in __import__("voxe_hip.build", fromlist=["SOURCES"]).SOURCES
    assert _proto_names(text, "int voxe_lift_accumulate") == ["grid", "cfg", "rays_o", "rays_d", "R", "jitter", "values", "C",
                                                              "sum_wv", "sum_w", "stream"]
    assert len(abi.HIP_ONLY["lift_accumulate"][1]) == 11
    src = open(os.path.join(ROOT, "vox-e_amd", "csrc", "voxe_lift.hip")).read()
    assert "__hip_atomic_fetch_add" in src and "__HIP_MEMORY_SCOPE_AGENT" in src and "asm" not in src and "getenv" not in src
    assert ops.lift_accumulate_ is not None and ops.lift_debug_merge is not None and ops.LIFT_ONE == 1 << 32


def test_validation_without_a_device():
    L = _lib()
    P = ctypes.c_void_p(16)
    g = make_grid_desc(16, 0, (8, 6, 5), 3, AABB, 1.0, abi.ACT_IDENTITY, abi.ACT_SOFTPLUS)   # features NULL: not read
    c = make_render_cfg(32, 1.0, 4.0)

    def acc(g_=g, c_=c, ro=P, rd=P, R=4, values=P, C=3, swv=P, sw=P):
        return L.voxe_lift_accumulate(ctypes.byref(g_) if g_ else None, ctypes.byref(c_) if c_ else None, ro, rd, R, None, values,
                                      C, swv, sw, None)

    assert acc(g_=None) == abi.ERR_NULL_POINTER and acc(c_=None) == abi.ERR_NULL_POINTER
    assert acc(ro=None) == abi.ERR_NULL_POINTER and acc(rd=None) == abi.ERR_NULL_POINTER
    g.densities = 0
    assert acc(g) == abi.ERR_NULL_POINTER
    g.densities = 16
    assert acc(R=-1) == abi.ERR_BAD_SHAPE and acc(R=1 << 31) == abi.ERR_BAD_SHAPE
    for dims in ((0, 6, 5), (8, -1, 5), (1300, 1300, 1300), (1 << 12, 1 << 12, 2), (2, 2, 1 << 24)):
        g.X, g.Y, g.Z = dims
        assert acc(g) == abi.ERR_BAD_SHAPE, dims
    g.X, g.Y, g.Z = 8, 6, 5
    c.num_samples = 0
    assert acc(c_=c) == abi.ERR_BAD_SHAPE
    c.num_samples = 32
    g.density_post_act = 9
    assert acc(g) == abi.ERR_UNSUPPORTED
    g.density_post_act, g.density_pre_act = abi.ACT_RELU, 5
    assert acc(g) == abi.ERR_UNSUPPORTED
    g.density_pre_act = abi.ACT_ABS
    # exactly one of values / sum_wv NULL; C outside 1..8
    assert acc(values=None) == abi.ERR_NULL_POINTER and acc(swv=None) == abi.ERR_NULL_POINTER
    assert acc(values=None, sw=None) == abi.ERR_NULL_POINTER and acc(swv=None, sw=None) == abi.ERR_NULL_POINTER
    assert acc(C=0) == abi.ERR_BAD_SHAPE and acc(C=9) == abi.ERR_BAD_SHAPE and acc(C=-1) == abi.ERR_BAD_SHAPE
    assert acc(values=None, C=9) == abi.ERR_BAD_SHAPE and acc(swv=None, C=0) == abi.ERR_BAD_SHAPE
    # R == 0 reads nothing: an empty values tensor has no address
    assert acc(ro=None, rd=None, R=0, values=None) == abi.OK and acc(ro=None, rd=None, R=0, values=None, C=9) == abi.ERR_BAD_SHAPE
    # no launch: R == 0 (NULL rays allowed), or both outputs NULL (coverage only without its output)
    for C in (1, 8):
        assert acc(ro=None, rd=None, R=0, C=C) == abi.OK
    assert acc(ro=None, rd=None, R=0, values=None, swv=None, sw=None) == abi.OK
    assert acc(values=None, swv=None, sw=None) == abi.OK and acc(values=None, swv=None, sw=None, C=0) == abi.OK
    # feature kind / F are not read
    g.feature_kind, g.F = 7, 0
    assert acc(values=None, swv=None, sw=None) == abi.OK
    # the merge pin: 0, 1, 2 and nothing else
    for mode in (1, 2, 0):
        assert L.voxe_lift_debug_merge(mode) == abi.OK
    assert L.voxe_lift_debug_merge(3) == abi.ERR_BAD_SHAPE and L.voxe_lift_debug_merge(-1) == abi.ERR_BAD_SHAPE


def test_operators_refuse_host_tensors():
    from thre3d_atom.thre3d_reprs.lifting import remove_mask
    from voxe_hip.runtime import VoxeError

    spec = ops.GridSpec(aabb=AABB)
    params = ops.RenderParams(num_samples=8, near=1.0, far=4.0)
    z = torch.zeros(4, 4, 4, 1)
    with pytest.raises(VoxeError):
        ops.lift_accumulate_(spec, params, z, torch.zeros(2, 3), torch.zeros(2, 3), torch.zeros(2, 1),
                             torch.zeros(4, 4, 4, 1, dtype=torch.int64), torch.zeros(4, 4, 4, dtype=torch.int64))
    with pytest.raises(VoxeError):      # the dilation is a device pass
        remove_mask(torch.ones(4, 4, 4, dtype=torch.uint8), 1)


# ---- region helpers on host tensors -------------------------------------------------------------------------------------
def _host_lifted():
    one = 1 << 32
    sum_w = torch.tensor([0, one // 2000, one // 500, one, 3 * one, one // 100], dtype=torch.int64).view(6, 1, 1)
    vote = torch.tensor([0.0, 1.0, 0.25, 0.5, 0.75, 0.499]).view(6, 1, 1)
    sum_wv = torch.stack([torch.round(sum_w.double() * vote.double()).to(torch.int64), -sum_w], dim=-1)
    return sum_wv, sum_w


def test_lifted_weight_mean_and_region_labels():
    from thre3d_atom.thre3d_reprs.lifting import Lifted, region_labels, remove_mask

    lifted = Lifted(*_host_lifted())
    w = lifted.weight()
    assert w.dtype == torch.float32 and w.shape == (6, 1, 1)
    assert torch.equal(w.flatten(), (lifted.sum_w.double() / 2.0 ** 32).float().flatten()) and float(w[3]) == 1.0
    m = lifted.mean(1e-3)
    assert m.dtype == torch.float32 and m.shape == (6, 1, 1, 2)
    assert bool(torch.isnan(m[0]).all()) and bool(torch.isnan(m[1]).all())          # weight 0 and 0.0005 <= 1e-3
    assert torch.allclose(m[2:, 0, 0, 0], torch.tensor([0.25, 0.5, 0.75, 0.499]), atol=1e-6)
    assert bool((m[2:, 0, 0, 1] == -1.0).all())
    assert not bool(torch.isnan(lifted.mean(0.0)[1]).any()) and bool(torch.isnan(lifted.mean(0.0)[0]).all())
    labels = region_labels(lifted)
    assert labels.dtype == torch.uint8 and labels.flatten().tolist() == [0, 0, 1, 2, 2, 1]
    assert region_labels(lifted, threshold=0.8).flatten().tolist() == [0, 0, 1, 1, 1, 1]
    assert region_labels(lifted, threshold=0.2, min_weight=0.0).flatten().tolist() == [0, 2, 2, 2, 2, 2]
    assert region_labels(lifted, min_weight=2.0).flatten().tolist() == [0, 0, 0, 0, 2, 0]
    rm = remove_mask(labels, 0)
    assert rm.dtype == torch.uint8 and rm.flatten().tolist() == [0, 0, 1, 0, 0, 1]


def test_save_and_load_region(tmp_path):
    from thre3d_atom.thre3d_reprs.lifting import Lifted, load_region, region_labels, save_region
    from thre3d_atom.thre3d_reprs.voxels import VoxelGrid, VoxelSize

    def grid(dims, size=0.1):
        return VoxelGrid(torch.zeros((*dims, 1)), torch.zeros((*dims, 3)), VoxelSize(size, size, size),
                         density_preactivation=torch.nn.Identity(), density_postactivation=torch.nn.ReLU())

    lifted = Lifted(*_host_lifted())
    labels = region_labels(lifted, 0.5, 1e-3)
    g = grid((6, 1, 1))
    path = tmp_path / "region.pth"
    save_region(path, labels, lifted, {"grid": g, "threshold": 0.5, "min_weight": 1e-3, "num_views": 7})
    raw = torch.load(path, weights_only=False)
    assert set(raw) == {"labels", "weight", "mean", "dims", "aabb", "threshold", "min_weight", "num_views"}
    region = load_region(path, g)
    assert torch.equal(region["labels"], labels) and region["labels"].dtype == torch.uint8
    assert torch.equal(region["weight"], lifted.weight()) and region["mean"].shape == (6, 1, 1, 2)
    assert tuple(region["dims"]) == (6, 1, 1) and region["num_views"] == 7
    assert region["threshold"] == 0.5 and region["min_weight"] == 1e-3
    assert np.allclose(np.array(region["aabb"]), np.array([[-0.3, 0.3], [-0.05, 0.05], [-0.05, 0.05]]))
    with pytest.raises(ValueError, match="dims"):
        load_region(path, grid((5, 1, 1)))
    with pytest.raises(ValueError, match="AABB"):
        load_region(path, grid((6, 1, 1), size=0.2))
    with pytest.raises(ValueError):
        save_region(tmp_path / "bad.pth", labels[:3], lifted, {"grid": g, "threshold": 0.5, "min_weight": 1e-3, "num_views": 1})


def test_lift_images_checks_its_images():
    from thre3d_atom.thre3d_reprs.lifting import lift_images

    vol_mod = type("V", (), {"thre3d_repr": None})()
    with pytest.raises(ValueError, match="N,C,H,W"):
        lift_images(vol_mod, [None, None], None, torch.zeros(3, 1, 4, 4))
    with pytest.raises(ValueError, match="N,C,H,W"):
        lift_images(vol_mod, [None], None, torch.zeros(1, 9, 4, 4))
    for bad in (1.5, float("nan")):
        with pytest.raises(ValueError, match="<= 1"):
            lift_images(vol_mod, [None], None, torch.full((1, 1, 4, 4), bad))


# ---- entry points -----------------------------------------------------------------------------------------------------
def _cli(name):
    spec = importlib.util.spec_from_file_location(name[:-3] + "_lift_cli", os.path.join(ROOT, name))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_entry_point_options():
    lift = {p.name: p for p in _cli("lift_masks_to_grid.py").main.params}
    assert set(lift) == {"model_path", "data_path", "masks_path", "output_path", "split", "threshold", "min_weight",
                         "overridden_num_samples_per_ray"}
    for name, short in (("model_path", "-i"), ("data_path", "-d"), ("masks_path", "-m"), ("output_path", "-o")):
        assert lift[name].required and short in lift[name].opts
    assert lift["split"].default == "train" and lift["threshold"].default == 0.5 and lift["min_weight"].default == 1e-3
    assert lift["overridden_num_samples_per_ray"].default is None
    exp = {p.name: p for p in _cli("export_mesh.py").main.params}
    assert exp["region"].default is None and not exp["region"].required
    byr = {p.name: p for p in _cli("prune_voxel_grid_by_region.py").main.params}
    assert set(byr) == {"model_path", "output_path", "region", "region_dilate"}
    assert byr["region"].required and byr["region_dilate"].default == 1
    # prune_voxel_grid.py is as it was: the region rule has an entry point of its own
    prune = {p.name for p in _cli("prune_voxel_grid.py").main.params}
    assert prune == {"model_path", "output_path", "data_path", "num_views", "weight_threshold", "dilate",
                     "overridden_num_samples_per_ray"}
    assert "region" not in open(os.path.join(ROOT, "prune_voxel_grid.py")).read()
    for doc in ("README.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "lift_masks_to_grid.py" in text and "prune_voxel_grid_by_region.py" in text and "--region" in text, doc
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "4.16" in design and "voxe_lift_debug_merge" in design
    assert "lift_bench.py" in open(os.path.join(ROOT, "tools", "README.md")).read()


def test_missing_mask_is_an_error_that_names_the_file(tmp_path):
    import click
    from PIL import Image

    mod = _cli("lift_masks_to_grid.py")
    (tmp_path / "train").mkdir()
    (tmp_path / "masks").mkdir()
    for name in ("a.png", "b.png"):
        Image.fromarray(np.zeros((4, 4, 3), dtype=np.uint8)).save(tmp_path / "train" / name)
    Image.fromarray(np.full((4, 4), 255, dtype=np.uint8)).save(tmp_path / "masks" / "a.png")
    with pytest.raises(click.UsageError, match="b.png"):
        mod.read_masks(tmp_path / "masks", tmp_path / "train", {"a.png": {}, "b.png": {}})
    rgba = np.zeros((4, 4, 4), dtype=np.uint8)
    rgba[..., 0], rgba[:2, :, 3] = 200, 51
    Image.fromarray(rgba).save(tmp_path / "masks" / "b.png")
    masks = mod.read_masks(tmp_path / "masks", tmp_path / "train", {"a.png": {}, "b.png": {}})
    assert masks.shape == (2, 1, 4, 4) and masks.dtype == torch.float32
    assert bool((masks[0] == 1.0).all()) and bool((masks[1, 0, :2] == 0.2).all()) and bool((masks[1, 0, 2:] == 0.0).all())


@pytest.mark.parametrize("flags,calls", [([], 0), (["--region", "region.pth"], 1)])
def test_export_mesh_takes_the_region_path_only_when_asked(flags, calls, tmp_path, monkeypatch):
    """without --region export_mesh.py makes exactly the calls it made before: extract_mesh(grid, level, mask=None)"""
    from click.testing import CliRunner

    from thre3d_atom.thre3d_reprs.constants import STATE_DICT, THRE3D_REPR
    from thre3d_atom.thre3d_reprs.mesh import Mesh

    mod = _cli("export_mesh.py")
    seen = {"region": [], "visible": [], "extract": []}
    grid = type("G", (), {"voxel_size": (0.1, 0.1, 0.1), "attn": None})()
    vol_mod = type("V", (), {"thre3d_repr": grid})()
    monkeypatch.setattr(mod.torch, "load", lambda *a, **k: {THRE3D_REPR: {STATE_DICT: {}}})
    monkeypatch.setattr(mod.torch.cuda, "synchronize", lambda *a: None)
    monkeypatch.setattr(mod, "create_volumetric_model_from_saved_model_attn", lambda *a, **k: (vol_mod, {"extra": 1}))
    monkeypatch.setattr(mod, "visible_mask", lambda *a: seen["visible"].append(a))

    def fake_region(g, path, mask):
        seen["region"].append((g, path, mask))
        return "REGION"

    def fake_extract(g, level=None, mask=None):
        seen["extract"].append((g, level, mask))
        return Mesh(torch.zeros(3, 3), torch.tensor([[0, 1, 2]], dtype=torch.int32), torch.zeros(3, 3))

    monkeypatch.setattr(mod, "region_mask", fake_region)
    monkeypatch.setattr(mod, "extract_mesh", fake_extract)
    res = CliRunner().invoke(mod.main, ["-i", "model.pth", "-o", str(tmp_path / "m.ply")] + flags)
    assert res.exit_code == 0, (res.output, res.exception)
    assert len(seen["region"]) == calls and not seen["visible"]
    (g, level, mask), = seen["extract"]
    assert g is grid and abs(level - np.log(2.0) / 0.1) < 1e-12
    if calls:
        assert mask == "REGION" and seen["region"][0] == (grid, "region.pth", None)
    else:
        assert mask is None
    assert (tmp_path / "m.ply").exists()


def test_mesh_mask_is_labels_not_one_and_the_given_mask():
    from thre3d_atom.thre3d_reprs.lifting import mesh_mask

    labels = torch.tensor([0, 1, 2, 1, 2, 0], dtype=torch.uint8).view(6, 1, 1)
    assert mesh_mask(labels).flatten().tolist() == [1, 0, 1, 0, 1, 1]
    other = torch.tensor([1, 1, 0, 0, 1, 0], dtype=torch.bool).view(6, 1, 1)
    assert mesh_mask(labels, other).flatten().tolist() == [1, 0, 0, 0, 1, 0]
