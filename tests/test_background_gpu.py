"""GPU checks of the environment-map background (voxe_background_fwd / voxe_background_bwd, ops.background_composite,
thre3d_reprs.background, VolumetricModel's background, the trainer's background_resolution) against the float64 restatement
tests/background_ref.py, whose inputs tests/test_background_host.py checks on the host.

Bounds.  Forward: the restatement run in float32 torch on the same inputs is the yardstick; the kernel's max abs error against
float64 must be at most 4 x that figure, floor 1e-6 (the convention of tests/test_distortion_gpu.py).  d_texels, d_acc, d_rays_d:
rel_l2 < 1e-4 against the restatement, the project's bound for gradients.  The three merge modes lie within the bounds of one
reference, hence within twice the bounds of each other."""
import logging
import re

import numpy as np
import pytest
import torch

import background_ref as BR
from voxe_hip import abi, ops, workload

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GRAD_REL_L2 = 1e-4
MODES = (0, 1, 2)          # voxe_background_debug_merge: shipped, run merge, plain

_rel_l2 = BR.rel_l2


def _to_dev(*ts):
    return [t.to(DEV).contiguous() for t in ts]


def _forward(texels, d, colour, acc):
    out = torch.empty_like(colour)
    ops.background_fwd_into(texels, d, colour, acc, out)
    return out


def _reference(texels, d, colour, acc, g):
    """(out64, d_acc, d_texels, d_rays_d, s, forward yardstick) of one case on the host"""
    out64 = BR.composite(colour, acc, d, texels)
    out32 = BR.composite(colour, acc, d, texels, dtype=torch.float32)
    d_acc, d_tex, d_d, s = BR.analytic_gradients(acc, d, texels, g)
    return out64, d_acc, d_tex, d_d, s, float((out32.double() - out64).abs().max())


# ---- 1: agreement with the restatement, every merge mode ----------------------------------------------------------------------
@pytest.mark.parametrize("R", BR.RAY_COUNTS)
@pytest.mark.parametrize("He,We", BR.MAPS)
def test_background_matches_the_restatement(He, We, R):
    texels, d, colour, acc, g, _, _ = BR.agreement_case(He, We, R)
    out64, r_acc, r_tex, r_d, s, yard = _reference(texels, d, colour, acc, g)
    bound = max(4.0 * yard, 1e-6)
    t_, d_, c_, a_, g_ = _to_dev(texels, d, colour, acc, g)
    out = _forward(t_, d_, c_, a_).cpu()
    err_fwd = float((out.double() - out64).abs().max())
    print(f"{He}x{We} R {R}: forward err {err_fwd:.3e} (f32 torch {yard:.3e}, bound {bound:.3e})")
    results = []
    for mode in MODES:
        d_acc, d_tex, d_d = (t.cpu() for t in ops.background_bwd(t_, d_, a_, g_, merge=mode))
        errs = (_rel_l2(d_tex, r_tex), _rel_l2(d_acc, r_acc), _rel_l2(d_d, r_d))
        print(f"{He}x{We} R {R} merge {mode}: rel_l2 d_texels {errs[0]:.3e}  d_acc {errs[1]:.3e}  d_rays_d {errs[2]:.3e}")
        results.append((mode, errs, d_acc, d_tex, d_d))
    assert err_fwd <= bound, (err_fwd, bound)
    dead = (s == 0).all(dim=1)
    for mode, errs, d_acc, d_tex, d_d in results:
        assert all(e < GRAD_REL_L2 for e in errs), (mode, errs)
        assert bool((d_tex[r_tex == 0] == 0).all()) and bool((d_d[dead] == 0).all())        # zero s: exact zeros
        assert all(bool(torch.isfinite(t).all()) for t in (d_acc, d_tex, d_d))
    for _, _, d_acc, d_tex, d_d in results[1:]:
        assert _rel_l2(d_tex, results[0][3]) < 2 * GRAD_REL_L2
        assert _rel_l2(d_acc, results[0][2]) < 2 * GRAD_REL_L2 and _rel_l2(d_d, results[0][4]) < 2 * GRAD_REL_L2


# ---- 2: contention ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["one_cell", "two_cells", "camera"])
def test_texel_gradient_under_contention(name):
    case = {"one_cell": BR.one_cell_case, "two_cells": BR.two_cell_case, "camera": BR.camera_case}[name]()
    texels, d, colour, acc, g = case
    _, _, r_tex, _, _, _ = _reference(*case)
    t_, d_, a_, g_ = _to_dev(texels, d, acc, g)
    for mode in MODES:
        _, d_tex, _ = ops.background_bwd(t_, d_, a_, g_, want_acc=False, want_rays_d=False, merge=mode)
        err = _rel_l2(d_tex.cpu(), r_tex)
        print(f"{name} merge {mode}: d_texels rel_l2 {err:.3e}")
        assert err < GRAD_REL_L2, (mode, err)
        assert bool((d_tex.cpu()[r_tex == 0] == 0).all())


# ---- 3: semantics -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base():
    texels, d, colour, acc, g, _, _ = BR.agreement_case(5, 7, 4096)
    t_, d_, c_, a_, g_ = _to_dev(texels, d, colour, acc, g)
    d_acc, d_tex, d_d = ops.background_bwd(t_, d_, a_, g_)
    return dict(t=t_, d=d_, c=c_, a=a_, g=g_, d_acc=d_acc, d_tex=d_tex, d_d=d_d, out=_forward(t_, d_, c_, a_))


def test_accumulate_adds_and_overwrite_clears(base):
    gen = torch.Generator().manual_seed(1)
    pre = [torch.randn(t.shape, generator=gen).to(DEV) for t in (base["d_acc"], base["d_tex"], base["d_d"])]
    onto = [p.clone() for p in pre]
    ops.background_bwd(base["t"], base["d"], base["a"], base["g"], d_acc=onto[0], d_texels=onto[1], d_rays_d=onto[2], accumulate=True)
    for got, p, want in zip(onto, pre, (base["d_acc"], base["d_tex"], base["d_d"])):
        assert _rel_l2(got, p + want) < 1e-5
    # accumulate = 0 over buffers full of garbage: overwritten, and texels no ray deposits into hold an exact 0
    few = slice(0, 3)                                        # three rays touch at most 12 of the 35 texels
    junk = [torch.full_like(p, float("nan")) for p in pre]
    ops.background_bwd(base["t"], base["d"][few].contiguous(), base["a"][few].contiguous(), base["g"][few].contiguous(),
                       d_acc=junk[0][few], d_texels=junk[1], d_rays_d=junk[2][few])
    assert bool(torch.isfinite(junk[1]).all()) and int((junk[1] == 0).all(dim=2).sum()) >= 35 - 12
    assert bool(torch.isfinite(junk[0][few]).all()) and bool(torch.isfinite(junk[2][few]).all())
    # outputs that are not asked for are not computed
    only = ops.background_bwd(base["t"], base["d"], base["a"], base["g"], want_acc=False, want_rays_d=False)
    assert only[0] is None and only[2] is None and _rel_l2(only[1], base["d_tex"]) < 1e-5
    none_tex = ops.background_bwd(base["t"], base["d"], base["a"], base["g"], want_texels=False)
    assert none_tex[1] is None and torch.equal(none_tex[0], base["d_acc"]) and torch.equal(none_tex[2], base["d_d"])
    # no rays: the binding leaves cleared texels
    e3, e1 = torch.zeros((0, 3), device=DEV), torch.zeros((0,), device=DEV)
    buf = torch.ones_like(base["t"])
    ops.background_bwd(base["t"], e3, e1, e3, d_texels=buf)
    assert int(buf.count_nonzero()) == 0 and _forward(base["t"], e3, e3, e1).shape == (0, 3)


def test_colour_out_may_be_colour_in(base):
    buf = base["c"].clone()
    ops.background_fwd_into(base["t"], base["d"], buf, base["a"], buf)
    assert torch.equal(buf, base["out"])


def test_saturated_rays_pass_through_bit_for_bit(base):
    """acc == 1: out == colour bit for bit and every gradient that carries the factor 1 - acc (d_texels, d_rays_d) is exactly 0;
    d_acc = -sum g b is the model's derivative at acc = 1 and has no such factor"""
    ones = torch.ones_like(base["a"])
    assert torch.equal(_forward(base["t"], base["d"], base["c"], ones), base["c"])
    for mode in MODES:
        d_acc, d_tex, d_d = ops.background_bwd(base["t"], base["d"], ones, base["g"], merge=mode)
        assert int(d_tex.count_nonzero()) == 0 and int(d_d.count_nonzero()) == 0
        assert float(d_acc.abs().max()) > 0           # (d_acc = -sum g b does not depend on acc)
    d_acc, d_tex, d_d = ops.background_bwd(base["t"], base["d"], base["a"], torch.zeros_like(base["g"]))
    assert int(d_acc.count_nonzero()) == 0 and int(d_tex.count_nonzero()) == 0 and int(d_d.count_nonzero()) == 0


def test_poles_and_unusable_directions(base):
    d = torch.tensor([[0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [0.0, 0.0, 0.0], [float("nan"), 1.0, 0.0], [1.0, float("inf"), 0.0],
                      [0.3, -0.2, 0.5]])
    gen = torch.Generator().manual_seed(3)
    colour, acc, g = torch.rand(6, 3, generator=gen), torch.rand(6, generator=gen) * 0.5, torch.randn(6, 3, generator=gen)
    texels = base["t"].cpu()
    out64, r_acc, r_tex, r_d, _, _ = _reference(texels, d, colour, acc, g)
    d_, c_, a_, g_ = _to_dev(d, colour, acc, g)
    out = _forward(base["t"], d_, c_, a_).cpu()
    assert bool(torch.isfinite(out).all()) and float((out.double() - out64).abs().max()) < 1e-6
    assert torch.equal(out[2:5], colour[2:5]) and bool((out[:2] != colour[:2]).all())      # unusable: b = 0; the poles have a value
    for mode in MODES:
        d_acc, d_tex, d_d = (t.cpu() for t in ops.background_bwd(base["t"], d_, a_, g_, merge=mode))
        assert all(bool(torch.isfinite(t).all()) for t in (d_acc, d_tex, d_d))
        assert int(d_d[:5].count_nonzero()) == 0 and int(d_acc[2:5].count_nonzero()) == 0 and float(d_d[5].abs().max()) > 0
        assert _rel_l2(d_tex, r_tex) < GRAD_REL_L2 and _rel_l2(d_acc, r_acc) < GRAD_REL_L2 and _rel_l2(d_d, r_d) < GRAD_REL_L2


# ---- 4: autograd through the render -------------------------------------------------------------------------------------------
def _scene(side=16, hw=24, views=1, first=0):
    """(spec, params, densities, features, rays_o, rays_d) of a soft ball that leaves most rays unsaturated"""
    import test_visibility_host as H

    ax = (torch.arange(side, dtype=torch.float32) + 0.5) / side * 3.0 - 1.5
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    r = torch.sqrt(x * x + y * y + z * z)
    gen = torch.Generator().manual_seed(4)
    dens = (torch.where(r < 0.8, 0.3, -3.0) + 0.1 * torch.randn(side, side, side, generator=gen))[..., None].contiguous()
    feat = torch.empty(side, side, side, 3).uniform_(-1, 1, generator=gen)
    spec = ops.GridSpec(aabb=((-1.5, 1.5),) * 3, density_scale=2.0)
    ro, rd = H.cameras(hw, views, DEV, first=first)
    params = ops.RenderParams(num_samples=48, near=workload.NEAR, far=workload.FAR, image_width=hw, image_height=hw if views > 1 else 0)
    return spec, params, dens.to(DEV), feat.to(DEV), ro, rd


@pytest.fixture(scope="module")
def through():
    """the direct computation: render, the restatement's b, render_bwd_into with d_colour = G and d_acc = -sum G b"""
    spec, params, dens, feat, ro, rd = _scene()
    gen = torch.Generator().manual_seed(6)
    texels = (torch.randn(8, 16, 3, generator=gen) * 1.5).to(DEV)
    G = torch.randn(ro.shape[0], 3, generator=gen).to(DEV)
    R = ro.shape[0]
    ws = ops.Workspace()
    out = [torch.empty((R, n), dtype=torch.float32, device=DEV) for n in (3, 1, 1, 1)]
    ops.render_fwd_into(spec, params, dens, feat, ro, rd, None, *out, ws, (0, 0))
    b = BR.background(texels.cpu().double(), rd.cpu().double())
    g_acc = (-(G.cpu().double() * b).sum(dim=1, keepdim=True)).float().to(DEV)
    d_dens, d_feat = torch.empty_like(dens), torch.empty_like(feat)
    ops.render_bwd_into(spec, params, dens, feat, ro, rd, None, out[0], out[1], out[2], G, None, g_acc, d_dens, d_feat, ws, (0, 0))
    acc = out[2].cpu().double()
    assert 0.2 < float((acc < 0.9).double().mean())          # most rays leave something for the background
    composite = (out[0].cpu().double() + (1 - acc) * b)
    return dict(spec=spec, params=params, dens=dens, feat=feat, ro=ro, rd=rd, texels=texels, G=G, g_acc=g_acc, d_dens=d_dens,
                d_feat=d_feat, colour=out[0], acc=out[2], composite=composite)


def test_grid_gradient_through_the_composite(through):
    p = through
    d, f = p["dens"].clone().requires_grad_(True), p["feat"].clone().requires_grad_(True)
    tex = p["texels"].clone().requires_grad_(True)
    col, _, acc, _ = ops.render(p["spec"], p["params"], d, f, p["ro"], p["rd"], rng=(0, 0))
    out = ops.background_composite(col, acc, p["rd"], tex)
    assert float((out.detach().cpu().double() - p["composite"]).abs().max()) < 1e-6
    (out * p["G"]).sum().backward()
    errs = _rel_l2(d.grad, p["d_dens"]), _rel_l2(f.grad, p["d_feat"])
    print(f"grid gradient through the composite: rel_l2 densities {errs[0]:.3e} features {errs[1]:.3e}")
    assert errs[0] < GRAD_REL_L2 and errs[1] < GRAD_REL_L2
    _, r_tex, _, _ = BR.analytic_gradients(p["acc"].cpu(), p["rd"].cpu(), p["texels"].cpu(), p["G"].cpu())[:4]
    assert _rel_l2(tex.grad.cpu(), r_tex) < GRAD_REL_L2


def test_grid_gradient_in_the_deferred_gradient_mode(through):
    from test_hip_fused_step import _region_to_gradients
    from thre3d_atom.modules.optim import FusedGridAdam
    from thre3d_atom.thre3d_reprs.voxels import VoxelGrid, VoxelSize

    p = through
    vg = VoxelGrid(p["dens"].clone(), p["feat"].clone(), VoxelSize(*(3.0 / 16,) * 3), density_preactivation=torch.nn.Identity(),
                   density_postactivation=torch.nn.Softplus(), expected_density_scale=2.0, tunable=True).to(DEV)
    spec = vg.voxe_grid_spec()
    with FusedGridAdam(vg, lr=0.01) as opt:
        ws = vg.voxe_workspace("sh")
        col, _, acc, _ = ops.render(spec, p["params"], vg.densities, vg.features, p["ro"], p["rd"], workspace=ws, rng=(0, 0))
        out = ops.background_composite(col, acc, p["rd"], p["texels"])
        (out * p["G"]).sum().backward()
        assert vg.densities.grad is None and vg.features.grad is None and ws.deferred.dirty
        region = ops.workspace_grad_view(spec, vg.densities, vg.features, ws).clone()
        d_dens, d_feat = _region_to_gradients(region, abi.GRAD_LINEAR, vg.densities.detach(), spec, 4)
        opt.zero_grad()
    errs = _rel_l2(d_dens, p["d_dens"]), _rel_l2(d_feat, p["d_feat"])
    print(f"deferred-gradient mode: rel_l2 densities {errs[0]:.3e} features {errs[1]:.3e}")
    assert errs[0] < GRAD_REL_L2 and errs[1] < GRAD_REL_L2


def test_ray_gradient_is_the_sum_of_both_parts(through):
    p = through
    rd = p["rd"].clone().requires_grad_(True)
    col, _, acc, _ = ops.render(p["spec"], p["params"], p["dens"], p["feat"], p["ro"], rd, rng=(0, 0))
    out = ops.background_composite(col, acc, rd, p["texels"])
    (out * p["G"]).sum().backward()
    _, part_render = ops.render_bwd_rays(p["spec"], p["params"], p["dens"], p["feat"], p["ro"], p["rd"], None, (0, 0), p["G"], None,
                                         p["g_acc"], want_o=False)
    _, _, part_bg = ops.background_bwd(p["texels"], p["rd"], p["acc"].reshape(-1).contiguous(), p["G"], want_acc=False,
                                       want_texels=False)
    err = _rel_l2(rd.grad, part_render + part_bg)
    print(f"d_rays_d: rel_l2 {err:.3e}; |render part| {float(part_render.norm()):.3e} |background part| {float(part_bg.norm()):.3e}")
    assert err < GRAD_REL_L2 and float(part_bg.norm()) > 0 and float(part_render.norm()) > 0


# ---- 5: the model -------------------------------------------------------------------------------------------------------------
def _model(side=16, samples=48, white=False, background=None):
    from thre3d_atom.modules.volumetric_model import VolumetricModel
    from thre3d_atom.thre3d_reprs.renderers import SHVoxGridRenderConfig, render_sh_voxel_grid
    from thre3d_atom.thre3d_reprs.voxels import VoxelGrid, VoxelSize
    from thre3d_atom.utils.imaging_utils import CameraBounds

    _, _, dens, feat, _, _ = _scene(side)
    vg = VoxelGrid(dens, feat, VoxelSize(*(3.0 / side,) * 3), density_preactivation=torch.nn.Identity(),
                   density_postactivation=torch.nn.Softplus(), expected_density_scale=2.0, tunable=True)
    cfg = SHVoxGridRenderConfig(samples, CameraBounds(1.8, 6.6), white_bkgd=white, perturb_sampled_points=False)
    return VolumetricModel(vg, render_sh_voxel_grid, cfg, device=DEV, background=background)


def _known_background(n=8, seed=12):
    from thre3d_atom.thre3d_reprs.background import EnvMapBackground

    bg = EnvMapBackground(n, 2 * n)
    with torch.no_grad():
        bg.texels.copy_(torch.randn(n, 2 * n, 3, generator=torch.Generator().manual_seed(seed)) * 1.5)
    return bg


def _view(i, hw=24):
    from thre3d_atom.utils.imaging_utils import CameraIntrinsics, pose_spherical

    return pose_spherical(60.0 * i, 20.0 + 50.0 * ((i * 0.618) % 1.0), 4.0311), CameraIntrinsics(hw, hw, 0.5 * hw / np.tan(0.5 * 0.6911112))


def _restated_image(vm, texels, pose, intr):
    """render(with_background=False).colour + (1 - acc) b, b from the restatement: [H, W, 3] float64 on the host"""
    from thre3d_atom.rendering.volumetric.utils.misc import cast_rays, flatten_rays
    from thre3d_atom.utils.constants import EXTRA_ACCUMULATED_WEIGHTS

    plain = vm.render(pose, intr, with_background=False)
    d = flatten_rays(cast_rays(intr, pose, device=DEV)).directions.cpu().double()
    b = BR.background(texels.detach().cpu().double(), d).reshape(intr.height, intr.width, 3)
    acc = plain.extra[EXTRA_ACCUMULATED_WEIGHTS].cpu().double()
    return plain.colour.cpu().double() + (1 - acc) * b, plain


def test_model_composites_the_background(tmp_path):
    from thre3d_atom.modules.volumetric_model import create_volumetric_model_from_saved_model
    from thre3d_atom.thre3d_reprs.voxels import create_voxel_grid_from_saved_info_dict
    from thre3d_atom.utils.constants import EXTRA_ACCUMULATED_WEIGHTS

    bg = _known_background()
    vm = _model(background=bg)
    pose, intr = _view(1)
    want, plain = _restated_image(vm, bg.texels, pose, intr)
    full = vm.render(pose, intr)
    err = float((full.colour.cpu().double() - want).abs().max())
    print(f"model render with a background: max abs err {err:.3e}")
    assert err < 1e-6 and float((full.colour - plain.colour).abs().max()) > 0.1
    assert torch.equal(full.depth, plain.depth) and torch.equal(full.extra[EXTRA_ACCUMULATED_WEIGHTS], plain.extra[EXTRA_ACCUMULATED_WEIGHTS])
    assert torch.equal(_model().render(pose, intr).colour, plain.colour)              # no background: as it was
    with pytest.raises(ValueError):
        _model(white=True, background=_known_background())
    with pytest.raises(ValueError):
        vm.render(pose, intr, white_bkgd=True)
    torch.save(vm.get_save_info(), tmp_path / "m.pth")
    loaded, _ = create_volumetric_model_from_saved_model(tmp_path / "m.pth", create_voxel_grid_from_saved_info_dict, device=DEV)
    assert loaded.background is not None and loaded.background.texels.is_cuda
    assert torch.equal(loaded.render(pose, intr).colour, full.colour)


# ---- 6: the trainer -----------------------------------------------------------------------------------------------------------
class _Capture(logging.Handler):
    def __init__(self):
        super().__init__()
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


@pytest.fixture(scope="module")
def capture_data():
    """six 24 x 24 views of the soft ball in front of a known, non-constant environment: the existing render plus the
    RESTATEMENT's background"""
    from thre3d_atom.data.datasets import InMemoryPosedImages
    from thre3d_atom.utils.imaging_utils import CameraBounds

    truth = _model()
    texels = _known_background(8, seed=21).texels
    poses, images = [], []
    for i in range(6):
        pose, intr = _view(i)
        image, _ = _restated_image(truth, texels, pose, intr)
        poses.append(torch.cat([pose.rotation, pose.translation], dim=1))
        images.append(image.float().clamp(0, 1).permute(2, 0, 1))
    return InMemoryPosedImages(torch.stack(images), torch.stack(poses), intr, CameraBounds(1.8, 6.6))


@pytest.mark.parametrize("fused", [True, False], ids=["fused_grid_step", "voxe_adam"])
@pytest.mark.parametrize("pose_lr", [0.0, 1e-3], ids=["fixed_poses", "pose_refinement"])
def test_trainer_learns_a_background(tmp_path, capture_data, fused, pose_lr, monkeypatch):
    from thre3d_atom.modules import trainers
    from thre3d_atom.thre3d_reprs.poses import CameraPoseDeltas
    from thre3d_atom.utils.logging import log

    made = []

    class Recording(CameraPoseDeltas):
        def __init__(self, n):
            super().__init__(n)
            made.append(self)

    monkeypatch.setattr(trainers, "CameraPoseDeltas", Recording)
    torch.manual_seed(5)
    vm = _model()
    cap = _Capture()
    log.addHandler(cap)
    try:
        trainers.train_sh_vox_grid_vol_mod_with_posed_images(
            vm, capture_data, tmp_path, ray_batch_size=1024, num_stages=1, num_iterations_per_stage=30, summary_freq=1,
            fast_debug_mode=True, fused_grid_step=fused, background_resolution=8, pose_learning_rate=pose_lr,
            distortion_weight=0.01 if pose_lr else 0.0)
    finally:
        log.removeHandler(cap)
    losses = [float(m.group(1)) for m in (re.search(r"loss:\s*([-+0-9.eE]+)", line) for line in cap.lines) if m]
    print(f"fused {fused} pose_lr {pose_lr}: loss {losses[:3]} ... {losses[-3:]}")
    assert len(losses) == 30 and np.mean(losses[-5:]) < np.mean(losses[:5])        # the loss falls
    # (the first reason that rules the one-call iteration out is the one that is logged: distortion_weight here, when both are on)
    assert sum("background_resolution > 0" in line for line in cap.lines) == (1 if fused and not pose_lr else 0)
    assert sum("no one-call iteration" in line for line in cap.lines) == (1 if fused else 0)
    texels = vm.background.texels.detach()
    assert tuple(texels.shape) == (8, 16, 3) and bool(torch.isfinite(texels).all()) and float(texels.abs().max()) > 0.05
    saved = torch.load(tmp_path / "saved_models" / "model_final.pth", map_location="cpu", weights_only=False)
    assert torch.equal(saved["background"]["state_dict"]["texels"], texels.cpu()) and saved["background"]["config_dict"] == {"height": 8, "width": 16}
    if pose_lr:
        grad = made[0].deltas.grad
        assert grad is not None and bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0
