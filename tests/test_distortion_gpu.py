"""GPU checks of the distortion loss on rays (voxe_distortion_fwd_bwd, ops.distortion_loss, thre3d_reprs.distortion, the trainer's
distortion_weight): agreement of value and gradient with the float64 restatement tests/distortion_ref.py for every lanes-per-ray
split of the kernel, the call's semantics, no interference with a forward / backward, descent on a floater, and the trainer on
both optimiser paths.  The inputs come from tests/test_distortion_host.py, which checks on the host that they are not vacuous.

Bounds.  Gradient: rel_l2 < 1e-4 against the restatement (the project's bound for render gradients, which go through the same
float32 gather and fast_exp chain).  ray_loss / loss: the restatement's own formula run in float32 torch on the same probed
samples is the yardstick (same input rounding); the kernel's max abs error against float64 must be at most 4 x that figure
(summation order, fast_exp, the scan), floor 1e-6."""
import logging

import numpy as np
import pytest
import torch

import distortion_ref as DR
import test_distortion_host as T
import test_visibility_host as H
from voxe_hip import abi, ops, workload

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GRAD_REL_L2 = 1e-4
LANES = (0, 1, 2, 4, 8)          # 0: the dispatcher's choice by R


def _rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def _call(spec, params, dens, ro, rd, jitter=None, rng=(0, 0), lanes=0, grad=True, grad_scale=1.0, accumulate=False, out=None,
          want_loss=True):
    d = out if out is not None else (torch.empty_like(dens) if grad else None)
    loss, ray = ops.distortion_fwd_bwd(spec, params, dens, ro, rd, jitter, rng, grad_scale=grad_scale, want_loss=want_loss,
                                       want_ray_loss=True, d_densities=d, accumulate=accumulate, lanes=lanes)
    return loss, ray, d


# ---- 1: agreement with the restatement, every lanes-per-ray split -----------------------------------------------------
@pytest.mark.parametrize("pre,post", T.ACTS)
@pytest.mark.parametrize("case", T.agreement_cases(), ids=lambda c: c[0])
def test_distortion_matches_the_restatement(case, pre, post):
    spec, params, dens, feat, ro, rd, jitter, rng = T.agreement_inputs(case, pre, post, DEV)
    L64, g64 = DR.loss_and_gradient(DR.distortion, spec, params, dens, feat, ro, rd, jitter, rng)
    T.assert_agreement_not_vacuous(case, L64, g64)
    with torch.no_grad():
        L32 = DR.distortion(spec, params, dens, feat, ro, rd, jitter, rng, dtype=torch.float32)
    yard_ray = float((L32.double() - L64).abs().max())
    yard_loss = abs(float(L32.mean()) - float(L64.mean()))
    bound_ray, bound_loss = max(4.0 * yard_ray, 1e-6), max(4.0 * yard_loss, 1e-6)
    results = []
    for lanes in LANES:
        loss, ray, d = _call(spec, params, dens, ro, rd, jitter, rng, lanes=lanes)
        err_ray = float((ray.double() - L64).abs().max())
        err_loss = abs(float(loss) - float(L64.mean()))
        err_g = _rel_l2(d, g64) if float(g64.norm()) > 0 else float(d.abs().max())
        print(f"{case[0]} pre {pre} post {post} lanes {lanes}: ray_loss err {err_ray:.3e} (f32 torch {yard_ray:.3e})  "
              f"loss err {err_loss:.3e} (f32 torch {yard_loss:.3e})  grad rel_l2 {err_g:.3e}")
        results.append((lanes, err_ray, err_loss, err_g, ray, d))
    for lanes, err_ray, err_loss, err_g, ray, d in results:
        assert err_ray <= bound_ray, (lanes, err_ray, bound_ray)
        assert err_loss <= bound_loss, (lanes, err_loss, bound_loss)
        assert err_g < GRAD_REL_L2, (lanes, err_g)
        assert bool((ray[L64 == 0] == 0).all()) and bool((d[g64 == 0] == 0).all())      # empty rays / untouched voxels: exact 0
        assert bool(torch.isfinite(ray).all()) and bool(torch.isfinite(d).all())
    # (every split within the bounds of the same reference: within twice the bounds of each other)
    for _, _, _, _, ray, d in results[1:]:
        assert float((ray - results[0][4]).abs().max()) <= 2 * bound_ray
        if float(g64.norm()) > 0:
            assert _rel_l2(d, results[0][5]) < 2 * GRAD_REL_L2


# ---- 2: semantics -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base():
    spec, params, dens, feat, ro, rd, jitter, rng = T.agreement_inputs(T.agreement_cases()[1], *T.ACTS[0], DEV)   # hash jitter + clip
    loss, ray, d = _call(spec, params, dens, ro, rd, jitter, rng)
    return dict(spec=spec, params=params, dens=dens, feat=feat, ro=ro, rd=rd, jitter=jitter, rng=rng, loss=loss, ray=ray, d=d)


def _again(p, **kw):
    return _call(p["spec"], p["params"], p["dens"], p["ro"], p["rd"], p["jitter"], p["rng"], **kw)


def test_accumulate_adds_to_the_buffer_and_clear_leaves_exact_zeros(base):
    pre = torch.randn(base["dens"].shape, generator=torch.Generator().manual_seed(1)).to(DEV) * float(base["d"].abs().max())
    _, _, onto = _again(base, accumulate=True, out=pre.clone())
    assert _rel_l2(onto, pre + base["d"]) < 1e-5
    assert torch.equal(onto[base["d"] == 0], pre[base["d"] == 0])            # voxels no sample touches keep the prefill's bits
    # accumulate = 0 over a buffer full of garbage: exact 0 where no sample lands
    _, _, fresh = _again(base, out=torch.full_like(base["dens"], float("nan")))
    untouched = fresh == 0
    assert bool(torch.isfinite(fresh).all()) and int(untouched.sum()) > 1000 and int((~untouched).sum()) > 100


def test_grad_scale_scales_the_gradient_only(base):
    loss, ray, d3 = _again(base, grad_scale=3.0)
    assert _rel_l2(d3, 3.0 * base["d"]) < 1e-6
    assert torch.equal(loss, base["loss"]) and torch.equal(ray, base["ray"])


def test_null_outputs(base):
    loss, ray, d = _again(base, grad=False)
    assert d is None and torch.equal(ray, base["ray"]) and torch.equal(loss, base["loss"])
    none, ray, _ = _again(base, grad=False, want_loss=False)
    assert none is None and torch.equal(ray, base["ray"])
    # R == 0 with accumulate = 0 still zeroes the gradient
    e = torch.zeros((0, 3), device=DEV)
    buf = torch.ones_like(base["dens"])
    loss0, ray0, _ = _call(base["spec"], base["params"], base["dens"], e, e, out=buf)
    assert int(buf.count_nonzero()) == 0 and ray0.shape == (0,) and float(loss0) == 0.0


def test_an_empty_relu_grid_gives_exact_zeros(base):
    spec = ops.GridSpec(aabb=H.AABB, density_scale=2.0, density_pre_act=abi.ACT_IDENTITY, density_post_act=abi.ACT_RELU)
    dens = -torch.rand((*H.DIMS, 1), generator=torch.Generator().manual_seed(2)).to(DEV) - 0.01
    for lanes in LANES:
        loss, ray, d = _call(spec, base["params"], dens, base["ro"], base["rd"], base["jitter"], base["rng"], lanes=lanes)
        assert float(loss) == 0.0 and int(ray.count_nonzero()) == 0 and int(d.count_nonzero()) == 0


def test_autograd_op_equals_the_direct_call(base):
    d = base["dens"].clone().requires_grad_(True)
    loss, ray = ops.distortion_loss(base["spec"], base["params"], d, base["ro"], base["rd"], base["jitter"], base["rng"],
                                    return_ray_loss=True)
    assert loss.dim() == 0 and torch.equal(loss.detach(), base["loss"]) and torch.equal(ray, base["ray"]) and not ray.requires_grad
    (2.5 * loss).backward()
    assert _rel_l2(d.grad, 2.5 * base["d"]) < 1e-5
    # no gradient wanted: none is computed, the value is the same
    with torch.no_grad():
        again = ops.distortion_loss(base["spec"], base["params"], base["dens"], base["ro"], base["rd"], base["jitter"], base["rng"])
    assert torch.equal(again, base["loss"]) and not again.requires_grad


def test_gradient_through_the_volumetric_model():
    from thre3d_atom.modules.volumetric_model import VolumetricModel
    from thre3d_atom.rendering.volumetric.render_interface import Rays
    from thre3d_atom.thre3d_reprs.renderers import SHVoxGridRenderConfig, render_sh_voxel_grid
    from thre3d_atom.thre3d_reprs.voxels import VoxelGrid, VoxelSize
    from thre3d_atom.utils.imaging_utils import CameraBounds

    spec, params, dens, feat, ro, rd, ball, shell = T.floater_inputs(DEV)
    vg = VoxelGrid(dens.clone(), feat.clone(), VoxelSize(*(3.0 / 32,) * 3), density_preactivation=torch.nn.Identity(),
                   density_postactivation=torch.nn.Softplus(), expected_density_scale=2.0, tunable=True)
    vm = VolumetricModel(vg, render_sh_voxel_grid, SHVoxGridRenderConfig(64, CameraBounds(workload.NEAR, workload.FAR),
                                                                        perturb_sampled_points=False), device=DEV)
    loss = vm.distortion_loss(Rays(ro, rd))
    loss.backward()
    want_loss, _, want = _call(spec, ops.RenderParams(num_samples=64, near=workload.NEAR, far=workload.FAR), dens, ro, rd)
    assert abs(float(loss) - float(want_loss)) <= 1e-7 and float(loss) > 1e-3
    assert vg.densities.grad is not None and _rel_l2(vg.densities.grad, want) < 1e-5 and vg.features.grad is None


# ---- 3: isolation -----------------------------------------------------------------------------------------------------
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
    for with_distortion in (False, True):
        d, f = dens0.clone().requires_grad_(True), feat0.clone().requires_grad_(True)
        ws = ops.Workspace()
        col = ops.render(spec, params, d, f, ro, rd, workspace=ws, rng=(3, 4))[0]
        if with_distortion:
            loss, ray, dd = _call(spec, params, d, ro, rd, rng=(3, 4))
            assert float(loss) > 1e-3 and float(dd.abs().max()) > 0
        (col * g_col).sum().backward()
        grads.append((d.grad.clone(), f.grad.clone()))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    assert float(grads[0][0].abs().max()) > 0


# ---- 4: descent on the floater ----------------------------------------------------------------------------------------
def test_descent_on_the_floater():
    """fixture: a dense ball and a faint shell in front of it (test_distortion_host.floater_field, checked there in float64)"""
    from thre3d_atom.modules.optim import VoxeAdam

    spec, params, dens, feat, ro, rd, ball, shell = T.floater_inputs(DEV)
    loss0, _, g = _call(spec, params, dens, ro, rd)
    loss0 = float(loss0)
    assert loss0 > 1e-3
    eta = 0.05 * loss0 / float((g.double() ** 2).sum())          # first order: lowers the loss by 5 %
    loss1 = float(_call(spec, params, dens - eta * g, ro, rd, grad=False)[0])
    print(f"floater: loss {loss0:.6f} -> {loss1:.6f} after one step of eta {eta:.3g}")
    assert loss1 < loss0
    d = torch.nn.Parameter(dens.clone())
    opt = VoxeAdam([d], lr=T.FLOATER_LR)
    for _ in range(T.FLOATER_STEPS):
        opt.zero_grad()
        ops.distortion_loss(spec, params, d, ro, rd).backward()
        opt.step()
    loss30 = float(_call(spec, params, d.detach(), ro, rd, grad=False)[0])
    peak0, peak30 = float(dens[ball].max()), float(d.detach()[ball].max())
    print(f"floater: loss {loss0:.6f} -> {loss30:.6f} after {T.FLOATER_STEPS} VoxeAdam steps; ball peak {peak0:.3f} -> {peak30:.3f}; "
          f"shell mean {float(dens[shell].mean()):.3f} -> {float(d.detach()[shell].mean()):.3f}")
    assert loss30 < 0.5 * loss0
    assert abs(peak30 - peak0) <= 0.1 * peak0


# ---- 5: the trainer ---------------------------------------------------------------------------------------------------
class _Capture(logging.Handler):
    def __init__(self):
        super().__init__()
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def test_trainer_with_the_distortion_term_on_both_optimiser_paths(tmp_path):
    import re

    from test_trainers_gpu import _sphere_model
    from thre3d_atom.data.datasets import InMemoryPosedImages
    from thre3d_atom.modules.trainers import train_sh_vox_grid_vol_mod_with_posed_images
    from thre3d_atom.modules.volumetric_model import VolumetricModel
    from thre3d_atom.thre3d_reprs.renderers import SHVoxGridRenderConfig, render_sh_voxel_grid
    from thre3d_atom.thre3d_reprs.voxels import VoxelGrid, VoxelSize
    from thre3d_atom.utils.imaging_utils import CameraBounds, CameraIntrinsics, pose_spherical
    from thre3d_atom.utils.logging import log

    # the synthetic views of test_reconstruction_trainer_fits_synthetic_views
    torch.manual_seed(1)
    truth = _sphere_model(side=24, samples=96)
    intr = CameraIntrinsics(48, 48, 0.5 * 48 / np.tan(0.5 * 0.6911112))
    poses, images = [], []
    for i in range(16):
        pose = pose_spherical(360.0 * i / 16, 20.0 + 50.0 * ((i * 0.618) % 1.0), 4.0311)
        poses.append(torch.cat([pose.rotation, pose.translation], dim=1))
        images.append(truth.render(pose, intr, perturb_sampled_points=False).colour.permute(2, 0, 1).cpu())
    data = InMemoryPosedImages(torch.stack(images), torch.stack(poses), intr, CameraBounds(1.8, 6.6))

    def run(weight, fused, out):
        torch.manual_seed(5)
        g = torch.Generator().manual_seed(3)
        vg = VoxelGrid(torch.empty(24, 24, 24, 1).uniform_(-1, 1, generator=g), torch.empty(24, 24, 24, 3).uniform_(-1, 1, generator=g),
                       VoxelSize(0.125, 0.125, 0.125), density_preactivation=torch.nn.Identity(),
                       density_postactivation=torch.nn.Softplus(), expected_density_scale=100.0 / 3.0, tunable=True)
        vm = VolumetricModel(vg, render_sh_voxel_grid, SHVoxGridRenderConfig(96, CameraBounds(1.8, 6.6), white_bkgd=True), device=DEV)
        cap = _Capture()
        log.addHandler(cap)
        try:
            # (the initializer is the identity: the three runs start from the same grid)
            train_sh_vox_grid_vol_mod_with_posed_images(vm, data, out, random_initializer=lambda t: t, ray_batch_size=4096,
                                                        num_stages=1, num_iterations_per_stage=3, summary_freq=1,
                                                        fast_debug_mode=True, fused_grid_step=fused, distortion_weight=weight)
        finally:
            log.removeHandler(cap)
        return vm.thre3d_repr.densities.detach().clone(), cap.lines

    base, lines0 = run(0.0, True, tmp_path / "w0")
    assert not any("distortion" in line for line in lines0)
    finals = {}
    for fused in (True, False):
        dens, lines = run(0.01, fused, tmp_path / f"w1_{int(fused)}")
        values = [float(m.group(1)) for m in (re.search(r"distortion:\s*([-+0-9.eE]+|nan|inf)", line) for line in lines) if m]
        print(f"fused_grid_step {fused}: distortion {values}")
        assert len(values) == 3 and all(np.isfinite(v) and v > 0 for v in values)
        assert not torch.equal(dens, base) and bool(torch.isfinite(dens).all())
        if fused:
            assert sum("no one-call iteration" in line for line in lines) == 1
        finals[fused] = dens
    err = _rel_l2(finals[True], finals[False])
    print(f"final densities, FusedGridAdam vs VoxeAdam: rel_l2 {err:.3e}")
    assert err < 1e-4
