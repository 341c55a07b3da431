"""CPU checks of the per-voxel visibility feature: the C ABI's declarations and argument validation (no device work), the pruning
rule per activation pair, the entry points' options, export_mesh.py's unchanged path without --visible_only, and -- with the
oracle's sample probe feeding the float64 restatement tests/visibility_ref.py -- that the inputs of the GPU tests
(tests/test_visibility_gpu.py builds them with the functions below) are not vacuous."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import visibility_ref
from conftest import ROOT
from voxe_hip import abi, ops, workload
from voxe_hip.desc import make_grid_desc, make_render_cfg

CPU = torch.device("cpu")
AABB = ((-1.9, 1.7), (-1.4, 1.6), (-2.0, 1.5))       # unequal voxel sizes with the non-cubic dims below; wider than the frusta
DIMS = (26, 20, 23)
ACTS = [(abi.ACT_IDENTITY, abi.ACT_SOFTPLUS), (abi.ACT_ABS, abi.ACT_RELU)]


# ---- inputs shared with the GPU tests ---------------------------------------------------------------------------------
def cast(hw, yaw, pitch, radius, device):
    """rays of one hw x hw camera on `device`: the kernel's ray casting there, the oracle's on the host"""
    from thre3d_atom.utils.imaging_utils import pose_spherical

    pose = pose_spherical(yaw, pitch, radius)
    if torch.device(device).type == "cpu":
        from oracle import voxe_oracle as vo

        o, d = vo.cast_rays(hw, hw, workload.focal_for(hw), pose.rotation.numpy(), pose.translation.numpy())
        return torch.from_numpy(o), torch.from_numpy(d)
    return ops.cast_rays(hw, hw, workload.focal_for(hw), pose.rotation, pose.translation, device)


def cameras(hw, n, device, first=0):
    """test_normals_gpu._cameras: n cameras of the synthetic workload, one after the other"""
    rays = [cast(hw, *workload.synth_pose_angles(i, 8), workload.RADIUS, device) for i in range(first, first + n)]
    return torch.cat([r[0] for r in rays]), torch.cat([r[1] for r in rays])


def agreement_cases():
    # (name, hw, views, perturb, jitter kind, aabb_clip, lindisp, order)
    return [
        ("plain", 48, 1, False, None, False, False, "image"),
        ("hash_clip", 40, 1, True, None, True, False, "image"),
        ("multiview_lindisp", 24, 3, True, None, False, True, "multiview"),
        ("jitter_shuffled", 32, 1, True, "caller", False, False, "shuffled"),
    ]


def agreement_inputs(case, pre, post, device):
    """(spec, params, densities, features, rays_o, rays_d, jitter, rng) of one agreement case"""
    name, hw, views, perturb, jkind, clip, lindisp, order = case
    g = torch.Generator().manual_seed(len(name) + 10 * pre + post)
    dens = torch.empty((*DIMS, 1)).uniform_(-1, 1, generator=g) * 1.5
    feat = torch.empty((*DIMS, 3)).uniform_(-1, 1, generator=g)
    spec = ops.GridSpec(aabb=AABB, density_scale=2.0, density_pre_act=pre, density_post_act=post)
    ro, rd = cameras(hw, views, device)
    R, S = ro.shape[0], 96
    width = height = 0
    if order in ("image", "multiview"):
        width = hw
        height = hw if order == "multiview" else 0
    elif order == "shuffled":
        perm = torch.randperm(R, generator=g).to(device)
        ro, rd = ro[perm].contiguous(), rd[perm].contiguous()
    params = ops.RenderParams(num_samples=S, near=workload.NEAR, far=workload.FAR, perturb=perturb, linear_disparity=lindisp,
                              aabb_clip=clip, image_width=width, image_height=height)
    jitter = torch.rand((R, S), generator=g).to(device) if jkind == "caller" else None
    rng = (1234, 77) if perturb and jitter is None else (0, 0)
    return spec, params, dens.to(device), feat.to(device), ro, rd, jitter, rng


def assert_agreement_not_vacuous(mw, mt):
    assert float(mw.max()) > 0.01
    assert int((mw == 0).sum()) > 100
    assert int((mt > 0.5).sum()) > 1000


def prune_inputs(device):
    """(spec, params, densities, features, rays_o, rays_d, jitter) of the lossless-pruning test: a ReLU field, empty in most
    places, 4 cameras at 64 x 64, S = 128, fixed caller jitter"""
    g = torch.Generator().manual_seed(17)
    dens = torch.empty((40, 40, 40, 1)).uniform_(-1, 1, generator=g) - 0.8     # 10 % of the voxels above 0: a faint haze
    ax = (torch.arange(40, dtype=torch.float32) + 0.5) / 40 * 3.0 - 1.5
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    dens[torch.sqrt(x * x + y * y + z * z) < 0.6] = 1.0                          # and a solid ball the central rays stop in
    feat = torch.empty((40, 40, 40, 3)).uniform_(-1, 1, generator=g)
    spec = ops.GridSpec(aabb=((-1.5, 1.5),) * 3, density_scale=3.0, density_pre_act=abi.ACT_IDENTITY,
                        density_post_act=abi.ACT_RELU)
    hw, S = 64, 128
    ro, rd = cameras(hw, 4, device)
    params = ops.RenderParams(num_samples=S, near=workload.NEAR, far=workload.FAR, perturb=True, white_bkgd=True, image_width=hw,
                              image_height=hw)
    jitter = torch.rand((ro.shape[0], S), generator=g).to(device)
    return spec, params, dens.to(device), feat.to(device), ro, rd, jitter


def assert_prune_not_vacuous(keep):
    frac = float((keep != 0).double().mean())
    assert 0.05 <= frac <= 0.95, frac


BALL_R0 = 0.7
BALL_CENTRE = (0.15, -0.1, 0.05)
BALL_AABB = ((-1.2, 1.3), (-1.0, 1.1), (-1.1, 1.2))
BALL_HW, BALL_RADIUS, BALL_NEAR, BALL_FAR = 96, 5.0, 3.0, 7.0
# azimuth {0, 90, 180, 270} x elevation +-35 degrees (pose_spherical's pitch is measured from the +z axis)
BALL_ANGLES = [(yaw, 90.0 - elev) for elev in (35.0, -35.0) for yaw in (0.0, 90.0, 180.0, 270.0)]


# The level above which the GPU test looks for the skin of the ball.  A ray that enters the ball head on meets, at radial depth x,
# sigma = 40 x and T = exp(-20 x^2), so one sample of length delta = (far - near) / (S - 1) = 4 / 383 weighs
# 40 x delta exp(-20 x^2) <= delta sqrt(40 / e) = 0.040 (at x = 0.16; an oblique ray peaks lower, by sqrt(cos)), and a corner gets
# t_c <= 1 of it: the 0.05 first written down for this test is out of reach -- the float64 restatement peaks at 0.0353 and has no
# voxel above 0.04.  Half the analytic peak is used instead; the restatement has 3971 voxels above it, at dist 0.42 .. 0.65.
BALL_WEIGHT_LEVEL = 0.02


def ball_field():
    """(densities [X,Y,Z,1] float32, dist [X,Y,Z] float64) of test_analytic_sphere_normals_are_radial: 40 (r0 - dist) under a
    Softplus, an opaque ball of radius r0"""
    dims = (70, 58, 64)
    axes = [torch.tensor([BALL_AABB[a][0] + (i + 0.5) * (BALL_AABB[a][1] - BALL_AABB[a][0]) / dims[a] for i in range(dims[a])],
                         dtype=torch.float64) for a in range(3)]
    x, y, z = torch.meshgrid(*axes, indexing="ij")
    dist = torch.sqrt((x - BALL_CENTRE[0]) ** 2 + (y - BALL_CENTRE[1]) ** 2 + (z - BALL_CENTRE[2]) ** 2)
    return (40.0 * (BALL_R0 - dist)).to(torch.float32)[..., None], dist, torch.stack([x, y, z], dim=-1)


def ball_setup():
    spec = ops.GridSpec(aabb=BALL_AABB, density_scale=1.0, density_pre_act=abi.ACT_IDENTITY, density_post_act=abi.ACT_SOFTPLUS)
    params = ops.RenderParams(num_samples=384, near=BALL_NEAR, far=BALL_FAR, image_width=BALL_HW)
    return spec, params


def test_ball_shell_projects_inside_every_frustum():
    """every voxel centre of the shell r0 + 0.15 < dist < r0 + 0.3 lands inside the image of each of the 8 cameras, between
    near and far: the shell's visibility is not a matter of the field of view"""
    from thre3d_atom.utils.imaging_utils import pose_spherical

    _, dist, xyz = ball_field()
    shell = xyz[(dist > BALL_R0 + 0.15) & (dist < BALL_R0 + 0.3)]
    assert len(shell) > 10000
    focal = workload.focal_for(BALL_HW)
    for yaw, pitch in BALL_ANGLES:
        pose = pose_spherical(yaw, pitch, BALL_RADIUS)
        rot, t = pose.rotation.double(), pose.translation.double()[:, 0]
        cam = (shell - t) @ rot                       # R^T (p - t): the camera looks down -z
        depth = -cam[:, 2]
        px, py = focal * cam[:, 0] / depth + BALL_HW / 2, -focal * cam[:, 1] / depth + BALL_HW / 2
        assert float(depth.min()) > BALL_NEAR + 0.1 and float(depth.max()) < BALL_FAR - 0.1
        assert float(min(px.min(), py.min())) > 1.0 and float(max(px.max(), py.max())) < BALL_HW - 1.0
        assert abs(float(t.norm()) - BALL_RADIUS) < 1e-5 and abs(abs(float(t[2])) - BALL_RADIUS * np.sin(np.radians(35.0))) < 1e-5


# ---- the inputs are not vacuous (oracle probe -> restatement, no device) ----------------------------------------------
@pytest.mark.parametrize("pre,post", ACTS)
@pytest.mark.parametrize("case", agreement_cases(), ids=lambda c: c[0])
def test_agreement_inputs_are_not_vacuous(case, pre, post):
    spec, params, dens, feat, ro, rd, jitter, rng = agreement_inputs(case, pre, post, CPU)
    mw, mt = visibility_ref.visibility_host(spec, params, dens, feat, ro, rd, jitter, rng)
    assert_agreement_not_vacuous(mw, mt)
    assert float(mt.max()) == 1.0


def test_prune_inputs_are_not_vacuous():
    spec, params, dens, feat, ro, rd, jitter = prune_inputs(CPU)
    mw, _ = visibility_ref.visibility_host(spec, params, dens, feat, ro, rd, jitter)
    assert_prune_not_vacuous(mw > 0)
    # ... and the renders the pruned grid is compared on are not empty images
    from oracle import voxe_oracle as vo

    grid = vo.Grid(dens.numpy(), feat.numpy(), spec.aabb, spec.density_scale, spec.density_pre_act, spec.density_post_act)
    cfg = make_render_cfg(params.num_samples, params.near, params.far, params.perturb, white_bkgd=params.white_bkgd)
    acc = vo.render_fwd(grid, cfg, ro.numpy(), rd.numpy(), jitter.numpy())["acc"]
    assert float(acc.max()) > 0.5 and float((acc > 0.5).mean()) > 0.02


# ---- C ABI ------------------------------------------------------------------------------------------------------------
def _lib():
    from voxe_hip import build

    return abi.declare(ctypes.CDLL(build.build()), "voxe_")


def test_visibility_symbols_are_declared_with_no_cpu_twin_and_abi_13():
    text = open(os.path.join(ROOT, "include", "voxe.h")).read()
    for name in ("voxe_visibility_accumulate", "voxe_visibility_mask"):
        assert re.search(rf"\b{name}\s*\(", text) and name in abi.hip_symbols()
    assert not re.search(r"\bvoxe_cpu_\w*visibility", text)
    assert not any("visibility" in s for s in abi.cpu_symbols())
    assert abi.ABI_VERSION == 13 and "#define VOXE_ABI_VERSION 13" in text
    L = _lib()
    assert L.voxe_abi_version() == 13
    assert hasattr(L, "voxe_visibility_accumulate") and hasattr(L, "voxe_visibility_mask")
    assert "voxe_visibility.hip" in __import__("voxe_hip.build", fromlist=["SOURCES"]).SOURCES


def test_validation_without_a_device():
    L = _lib()
    P = ctypes.c_void_p(16)
    g = make_grid_desc(16, 0, (8, 6, 5), 3, AABB, 1.0, abi.ACT_IDENTITY, abi.ACT_SOFTPLUS)   # features NULL: not read
    c = make_render_cfg(32, 1.0, 4.0)

    def acc(g_=g, c_=c, ro=P, rd=P, R=4, mw=P, mt=P):
        return L.voxe_visibility_accumulate(ctypes.byref(g_) if g_ else None, ctypes.byref(c_) if c_ else None, ro, rd, R, None,
                                            mw, mt, None)

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
    # no launch: R == 0 (NULL rays allowed), or both outputs NULL
    assert acc(ro=None, rd=None, R=0, mw=None, mt=None) == abi.OK and acc(ro=None, rd=None, R=0) == abi.OK
    assert acc(mw=None, mt=None) == abi.OK
    # feature kind / F are not read
    g.feature_kind, g.F = 7, 0
    assert acc(mw=None, mt=None) == abi.OK

    def mask(vis=P, dims=(4, 5, 6), thr=0.0, dilate=0, out=P):
        return L.voxe_visibility_mask(vis, *dims, thr, dilate, out, None)

    assert mask(vis=None) == abi.ERR_NULL_POINTER and mask(out=None) == abi.ERR_NULL_POINTER
    for dims in ((0, 5, 6), (4, -1, 6), (1300, 1300, 1300)):
        assert mask(dims=dims) == abi.ERR_BAD_SHAPE, dims
    assert mask(dilate=4) == abi.ERR_BAD_SHAPE and mask(dilate=-1) == abi.ERR_BAD_SHAPE


def test_operators_refuse_host_tensors():
    from voxe_hip.runtime import VoxeError

    spec = ops.GridSpec(aabb=AABB)
    params = ops.RenderParams(num_samples=8, near=1.0, far=4.0)
    z = torch.zeros(4, 4, 4, 1)
    with pytest.raises(VoxeError):
        ops.visibility_accumulate_(spec, params, z, torch.zeros(2, 3), torch.zeros(2, 3), torch.zeros(4, 4, 4))
    with pytest.raises(VoxeError):
        ops.visibility_mask(torch.zeros(4, 4, 4), 0.0)


# ---- pruning rule -----------------------------------------------------------------------------------------------------
def test_empty_value_per_activation_pair():
    from thre3d_atom.thre3d_reprs.visibility import empty_raw_density, pruned_densities

    raw = torch.tensor([-30.0, -3.0, -0.0, 0.0, 0.5, 7.0]).view(6, 1, 1, 1)
    drop = torch.zeros(6, 1, 1, dtype=torch.uint8)
    keep = torch.ones(6, 1, 1, dtype=torch.bool)
    for post in (abi.ACT_IDENTITY, abi.ACT_RELU):
        assert empty_raw_density(abi.ACT_IDENTITY, post, 2.5) == 0.0 and empty_raw_density(abi.ACT_ABS, post, 2.5) == 0.0
        out = pruned_densities(raw, drop, abi.ACT_IDENTITY, post, 2.5)
        assert torch.equal(out, torch.minimum(raw, torch.zeros_like(raw)))            # lowered to 0, never raised
        assert torch.equal(pruned_densities(raw, drop, abi.ACT_ABS, post, 2.5), torch.zeros_like(raw))
        assert torch.equal(pruned_densities(raw, keep, abi.ACT_ABS, post, 2.5), raw)
    assert empty_raw_density(abi.ACT_IDENTITY, abi.ACT_SOFTPLUS, 2.5) == -8.0
    out = pruned_densities(raw, drop, abi.ACT_IDENTITY, abi.ACT_SOFTPLUS, 2.5)
    assert torch.equal(out.flatten(), torch.tensor([-30.0, -8.0, -8.0, -8.0, -8.0, -8.0]))
    with pytest.raises(ValueError):
        empty_raw_density(abi.ACT_ABS, abi.ACT_SOFTPLUS, 1.0)
    with pytest.raises(ValueError):
        pruned_densities(raw, drop, abi.ACT_ABS, abi.ACT_SOFTPLUS, 1.0)
    # a mixed mask ([X,Y,Z,1] accepted): kept voxels are bit-identical, pre(scale * raw') <= pre(scale * raw) everywhere
    g = torch.Generator().manual_seed(0)
    raw = torch.randn((5, 4, 3, 1), generator=g)
    m = torch.rand((5, 4, 3, 1), generator=g) > 0.5
    for pre, post in ((abi.ACT_IDENTITY, abi.ACT_SOFTPLUS), (abi.ACT_IDENTITY, abi.ACT_RELU), (abi.ACT_ABS, abi.ACT_RELU)):
        out = pruned_densities(raw, m, pre, post, 1.7)
        assert torch.equal(out[m], raw[m])
        f = (lambda x: x.abs()) if pre == abi.ACT_ABS else (lambda x: x)
        assert bool((f(1.7 * out) <= f(1.7 * raw)).all()) and bool((out[~m] != raw[~m]).any())


def test_prune_voxel_grid_on_a_host_grid():
    from thre3d_atom.thre3d_reprs.visibility import prune_voxel_grid_
    from thre3d_atom.thre3d_reprs.voxels import VoxelGrid, VoxelSize

    g = torch.Generator().manual_seed(1)
    dens, feat = torch.randn((6, 5, 4, 1), generator=g), torch.randn((6, 5, 4, 3), generator=g)
    keep = torch.rand((6, 5, 4), generator=g) > 0.4
    for tunable in (False, True):
        vg = VoxelGrid(dens.clone(), feat.clone(), VoxelSize(0.1, 0.1, 0.1), density_preactivation=torch.nn.Identity(),
                       density_postactivation=torch.nn.Softplus(), expected_density_scale=4.0, tunable=tunable)
        n = prune_voxel_grid_(vg, keep.to(torch.uint8))
        want = torch.where(keep[..., None], dens, dens.clamp(max=-5.0))
        assert torch.equal(vg.densities.detach(), want) and torch.equal(vg.features.detach(), feat)
        assert n == int((want != dens).sum()) and 0 < n <= int((~keep).sum())
        assert prune_voxel_grid_(vg, keep) == 0                        # idempotent
    vg = VoxelGrid(dens.clone(), feat.clone(), VoxelSize(0.1, 0.1, 0.1), density_preactivation=torch.abs,
                   density_postactivation=torch.nn.Softplus())
    with pytest.raises(ValueError):
        prune_voxel_grid_(vg, keep)
    with pytest.raises(ValueError):
        prune_voxel_grid_(vg, keep[:3])


# ---- entry points -----------------------------------------------------------------------------------------------------
def _cli(name):
    spec = importlib.util.spec_from_file_location(name[:-3] + "_vis_cli", os.path.join(ROOT, name))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_entry_point_options():
    import click

    prune = {p.name: p for p in _cli("prune_voxel_grid.py").main.params}
    assert set(prune) == {"model_path", "output_path", "data_path", "num_views", "weight_threshold", "dilate",
                          "overridden_num_samples_per_ray"}
    assert prune["model_path"].required and prune["output_path"].required and prune["data_path"].default is None
    assert prune["num_views"].default == 36 and prune["weight_threshold"].default == 0.0 and prune["dilate"].default == 1
    assert "-i" in prune["model_path"].opts and "-o" in prune["output_path"].opts and "-d" in prune["data_path"].opts
    ctx = click.Context(_cli("prune_voxel_grid.py").main)
    with pytest.raises(click.BadParameter):
        prune["dilate"].type.convert("4", prune["dilate"], ctx)
    exp = {p.name: p for p in _cli("export_mesh.py").main.params}
    assert exp["visible_only"].is_flag and exp["visible_only"].default is False
    assert exp["visibility_threshold"].default == 0.0 and exp["num_views"].default == 36 and exp["data_path"].default is None
    for doc in ("README.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "prune_voxel_grid.py" in text and "--visible_only" in text, doc
    assert "4.10" in open(os.path.join(ROOT, "DESIGN.md")).read()


@pytest.mark.parametrize("flags,calls", [([], 0), (["--visible_only", "--num_views", "5"], 1)])
def test_export_mesh_takes_the_visibility_path_only_when_asked(flags, calls, tmp_path, monkeypatch):
    """without --visible_only export_mesh.py makes exactly the calls it made before: extract_mesh(grid, level, mask=None)"""
    from click.testing import CliRunner

    from thre3d_atom.thre3d_reprs.constants import STATE_DICT, THRE3D_REPR
    from thre3d_atom.thre3d_reprs.mesh import Mesh

    mod = _cli("export_mesh.py")
    seen = {"visible": [], "extract": []}
    grid = type("G", (), {"voxel_size": (0.1, 0.1, 0.1), "attn": None})()
    vol_mod = type("V", (), {"thre3d_repr": grid})()
    monkeypatch.setattr(mod.torch, "load", lambda *a, **k: {THRE3D_REPR: {STATE_DICT: {}}})
    monkeypatch.setattr(mod.torch.cuda, "synchronize", lambda *a: None)
    monkeypatch.setattr(mod, "create_volumetric_model_from_saved_model_attn", lambda *a, **k: (vol_mod, {"extra": 1}))

    def fake_visible(vm, extra, cfg, mask):
        seen["visible"].append((vm, extra, cfg.num_views, cfg.visibility_threshold, mask))
        return "VISIBLE"

    def fake_extract(g, level=None, mask=None):
        seen["extract"].append((g, level, mask))
        return Mesh(torch.zeros(3, 3), torch.tensor([[0, 1, 2]], dtype=torch.int32), torch.zeros(3, 3))

    monkeypatch.setattr(mod, "visible_mask", fake_visible)
    monkeypatch.setattr(mod, "extract_mesh", fake_extract)
    res = CliRunner().invoke(mod.main, ["-i", "model.pth", "-o", str(tmp_path / "m.ply")] + flags)
    assert res.exit_code == 0, (res.output, res.exception)
    assert len(seen["visible"]) == calls
    (g, level, mask), = seen["extract"]
    assert g is grid and abs(level - np.log(2.0) / 0.1) < 1e-12
    if calls:
        assert mask == "VISIBLE" and seen["visible"][0] == (vol_mod, {"extra": 1}, 5, 0.0, None)
    else:
        assert mask is None
    assert (tmp_path / "m.ply").exists()
