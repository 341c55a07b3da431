"""GPU checks of the orientation loss (voxe_orientation_fwd_bwd, ops.orientation_loss, thre3d_reprs.orientation, the trainer's
orientation_weight): agreement of value and gradient with the float64 restatement tests/orientation_ref.py for every
lanes-per-ray split of the kernel, the analytic tie to voxe_render_normals, the call's semantics, the buffer contract, no
interference with a forward / backward, descent on a fuzzy ball, and the trainer on both optimiser paths.  The inputs come from
tests/test_orientation_host.py, which checks on the host that they are well conditioned and not vacuous.

Bounds (the precedent of tests/test_depth_gpu.py).  Gradient: rel_l2 < 1e-4 against the restatement.  ray_loss / loss: the
restatement's own formula run in float32 torch on the same probed samples is the yardstick; the kernel's max abs error against
float64 must be at most 4 x that figure, floor 1e-6.

Measured on an MI355X (worst lanes-per-ray split, worse of normal_eps 0 / 1e-2 and of with / without ray_weight; ray_loss error
(float32 torch's) / loss error / gradient rel_l2), identity + Softplus:
    plain 9.4e-08 (9.4e-08) / 1.3e-09 / 3.0e-07          hash_clip 9.1e-08 (9.9e-08) / 1.9e-09 / 3.7e-07
    multiview_lindisp 6.9e-08 (8.2e-08) / 2.3e-09 / 1.9e-06    jitter_shuffled 7.6e-08 (7.0e-08) / 2.1e-09 / 3.0e-07
    linear_R1/63/65 6.0e-08 (5.5e-08) / 2.3e-08 / 3.7e-07      linear_S1 1.5e-07 (2.0e-07) / 5.7e-09 / 2.2e-07
    linear_S2/37 1.7e-07 (1.7e-07) / 3.4e-09 / 6.8e-07         dense_faces 9.8e-08 (8.5e-08) / 8.0e-09 / 3.8e-07
abs + ReLU is within the same figures; the ramp's ray_loss equals u_x^2 acc to 8.6e-08 relative; DESIGN.md 4.20 holds the whole
table."""
import ctypes as C
import functools
import logging

import numpy as np
import pytest
import torch

import orientation_ref as OR
import test_orientation_host as T
import test_visibility_host as H
from voxe_hip import abi, ops, workload

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GRAD_REL_L2 = 1e-4
LANES = (0, 1, 2, 4, 8)          # 0: the dispatcher's choice by R


def _rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def _call(spec, params, dens, ro, rd, omega=None, jitter=None, rng=(0, 0), lanes=0, grad=True, grad_scale=1.0, accumulate=False,
          out=None, want_loss=True, eps=OR.NORMAL_EPS):
    d = out if out is not None else (torch.empty_like(dens) if grad else None)
    loss, ray = ops.orientation_fwd_bwd(spec, params, dens, ro, rd, omega, jitter, rng, normal_eps=eps, grad_scale=grad_scale,
                                        want_loss=want_loss, want_ray_loss=True, d_densities=d, accumulate=accumulate, lanes=lanes)
    return loss, ray, d


def _agreement(name, inputs, eps, omega):
    spec, params, dens, feat, ro, rd, jitter, rng = inputs
    L64, g64 = OR.loss_and_gradient(OR.orientation, spec, params, dens, feat, ro, rd, omega, jitter=jitter, rng=rng, eps=eps)
    with torch.no_grad():
        L32 = OR.orientation(spec, params, dens, feat, ro, rd, jitter=jitter, rng=rng, eps=eps, dtype=torch.float32)
    om = torch.ones_like(L64) if omega is None else omega.double()
    mean64 = float((L64 * om).mean())
    yard_ray = float((L32.double() - L64).abs().max())
    yard_loss = abs(float((L32.double() * om).mean()) - mean64)
    bound_ray, bound_loss = max(4.0 * yard_ray, 1e-6), max(4.0 * yard_loss, 1e-6)
    results = []
    for lanes in LANES:
        loss, ray, d = _call(spec, params, dens, ro, rd, omega, jitter, rng, lanes=lanes, eps=eps)
        err_ray = float((ray.double() - L64).abs().max())
        err_loss = abs(float(loss) - mean64)
        err_g = _rel_l2(d, g64) if float(g64.norm()) > 0 else float(d.abs().max())
        print(f"{name} lanes {lanes}: ray_loss err {err_ray:.3e} (f32 torch {yard_ray:.3e})  "
              f"loss err {err_loss:.3e} (f32 torch {yard_loss:.3e})  grad rel_l2 {err_g:.3e}")
        results.append((lanes, err_ray, err_loss, err_g, ray, d))
    for lanes, err_ray, err_loss, err_g, ray, d in results:
        assert err_ray <= bound_ray, (lanes, err_ray, bound_ray)
        assert err_loss <= bound_loss, (lanes, err_loss, bound_loss)
        assert err_g < GRAD_REL_L2, (lanes, err_g)
        assert bool((ray[L64 == 0] == 0).all()) and bool((d[g64 == 0] == 0).all())      # exact zeros where the restatement has them
        assert bool(torch.isfinite(ray).all()) and bool(torch.isfinite(d).all())
    # (every split within the bounds of the same reference: within twice the bounds of each other)
    for _, _, _, _, ray, d in results[1:]:
        assert float((ray - results[0][4]).abs().max()) <= 2 * bound_ray
        if float(g64.norm()) > 0:
            assert _rel_l2(d, results[0][5]) < 2 * GRAD_REL_L2
    return L64, g64


# ---- 1: agreement with the restatement, every lanes-per-ray split -----------------------------------------------------
@pytest.mark.parametrize("eps", T.EPS)
@pytest.mark.parametrize("pre,post", T.ACTS)
@pytest.mark.parametrize("case", T.agreement_cases(), ids=lambda c: c[0])
def test_orientation_matches_the_restatement(case, pre, post, eps):
    inputs = T.agreement_inputs(case, pre, post, DEV)
    spec, params, dens, feat, ro, rd, jitter, rng = inputs
    name = f"{case[0]} pre {pre} post {post} eps {eps}"
    L64, g64 = _agreement(name, inputs, eps, None)
    _, g_n = OR.loss_and_gradient(OR.orientation, spec, params, dens, feat, ro, rd, jitter=jitter, rng=rng, eps=eps, part="normals")
    T.assert_agreement_not_vacuous(case, L64, g64, g_n)
    _agreement(name + " weighted", inputs, eps, T.ray_weights(ro.shape[0], DEV))


# ---- 2: the analytic tie to voxe_render_normals -----------------------------------------------------------------------
def test_ramp_in_x_ties_the_loss_to_the_rendered_normals():
    """v is a ramp in x only and every sample lies in an interior cell: n = (-1, 0, 0) everywhere.  Rays towards -x see the
    normal's back: L_r = u_x^2 * acc_r with voxe_render_normals' acc of the same rays; rays towards +x: exactly nothing"""
    spec, params, dens, feat, ro, rd = T.ramp_inputs(DEV)
    normals, _, acc = ops.render_normals(spec, params, dens, ro, rd)
    acc = acc.reshape(-1).double()
    ux = OR.unit_directions(rd)[:, 0]
    assert float((normals[:, 0].double() + acc).abs().max()) < 1e-5 and float(normals[:, 1:].abs().max()) == 0.0
    for lanes in LANES:
        _, ray, _ = _call(spec, params, dens, ro, rd, lanes=lanes, eps=0.0)
        want = ux[:36] ** 2 * acc[:36]
        err = float(((ray[:36].double() - want).abs() / want).max())
        print(f"ramp lanes {lanes}: max relative error of ray_loss against u_x^2 acc {err:.3e}")
        assert err < 1e-6 and float(want.min()) > 1e-2
        assert int(ray[36:].count_nonzero()) == 0
        _, ray_pos, d_pos = _call(spec, params, dens, ro[36:].contiguous(), rd[36:].contiguous(), lanes=lanes, eps=0.0)
        assert int(ray_pos.count_nonzero()) == 0 and int(d_pos.count_nonzero()) == 0


# ---- 3: semantics -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base():
    spec, params, dens, feat, ro, rd, jitter, rng = T.agreement_inputs(T.agreement_cases()[1], *T.ACTS[0], DEV)  # hash + clip
    omega = T.ray_weights(ro.shape[0], DEV)
    loss, ray, d = _call(spec, params, dens, ro, rd, omega, jitter, rng)
    return dict(spec=spec, params=params, dens=dens, feat=feat, ro=ro, rd=rd, jitter=jitter, rng=rng, omega=omega,
                loss=loss, ray=ray, d=d)


def _again(p, omega="base", **kw):
    return _call(p["spec"], p["params"], p["dens"], p["ro"], p["rd"], p["omega"] if isinstance(omega, str) else omega,
                 p["jitter"], p["rng"], **kw)


def test_accumulate_adds_to_the_buffer_and_clear_leaves_exact_zeros(base):
    pre = torch.randn(base["dens"].shape, generator=torch.Generator().manual_seed(1)).to(DEV) * float(base["d"].abs().max())
    _, _, onto = _again(base, accumulate=True, out=pre.clone())
    assert _rel_l2(onto, pre + base["d"]) < 1e-5
    assert torch.equal(onto[base["d"] == 0], pre[base["d"] == 0])            # voxels no sample touches keep the prefill's bits
    _, _, fresh = _again(base, out=torch.full_like(base["dens"], float("nan")))
    untouched = fresh == 0
    assert bool(torch.isfinite(fresh).all()) and int(untouched.sum()) > 1000 and int((~untouched).sum()) > 100


def test_grad_scale_scales_the_gradient_only(base):
    loss, ray, d3 = _again(base, grad_scale=3.0)
    assert _rel_l2(d3, 3.0 * base["d"]) < 1e-6
    assert torch.equal(loss, base["loss"]) and torch.equal(ray, base["ray"])


def test_no_ray_weight_equals_all_ones_bit_for_bit(base):
    ones = torch.ones_like(base["omega"])
    a = [_again(base, omega=None), _again(base, omega=ones)]
    assert torch.equal(a[0][0], a[1][0]) and torch.equal(a[0][1], a[1][1])
    assert _rel_l2(a[0][2], a[1][2]) < 1e-6 and not torch.equal(a[0][0], base["loss"])
    assert torch.equal(a[0][1], base["ray"])                                 # L_r does not carry omega_r


def test_null_outputs_and_no_rays(base):
    loss, ray, d = _again(base, grad=False)
    assert d is None and torch.equal(ray, base["ray"]) and torch.equal(loss, base["loss"])
    none, ray, _ = _again(base, grad=False, want_loss=False)
    assert none is None and torch.equal(ray, base["ray"])
    _, _, d = _again(base, want_loss=False)
    assert _rel_l2(d, base["d"]) < 1e-6
    p = base
    only_grad = torch.empty_like(p["dens"])
    got = ops.orientation_fwd_bwd(p["spec"], p["params"], p["dens"], p["ro"], p["rd"], p["omega"], p["jitter"], p["rng"],
                                  want_loss=False, want_ray_loss=False, d_densities=only_grad)
    assert got == (None, None) and _rel_l2(only_grad, base["d"]) < 1e-6
    only_loss, none = ops.orientation_fwd_bwd(p["spec"], p["params"], p["dens"], p["ro"], p["rd"], p["omega"], p["jitter"], p["rng"])
    assert none is None and torch.equal(only_loss, base["loss"])
    assert ops.orientation_fwd_bwd(p["spec"], p["params"], p["dens"], p["ro"], p["rd"], want_loss=False) == (None, None)
    # R == 0 with accumulate = 0 still zeroes the gradient
    e = torch.zeros((0, 3), device=DEV)
    buf = torch.ones_like(base["dens"])
    loss0, ray0, _ = _call(base["spec"], base["params"], base["dens"], e, e, out=buf)
    assert int(buf.count_nonzero()) == 0 and ray0.shape == (0,) and float(loss0) == 0.0


def test_bad_normal_eps_and_short_scratch_are_refused(base):
    from voxe_hip.desc import make_grid_desc, make_render_cfg
    from voxe_hip.runtime import VoxeError, lib, ptr, stream_ptr

    for eps in (-1e-5, float("inf"), float("nan")):
        with pytest.raises(VoxeError):
            _again(base, eps=eps)
    p, L = base, lib()
    g = make_grid_desc(p["dens"].data_ptr(), 0, H.DIMS, 3, H.AABB, 2.0, *T.ACTS[0])
    c = make_render_cfg(p["params"].num_samples, p["params"].near, p["params"].far)
    R = p["ro"].shape[0]
    need = L.voxe_orientation_scratch_bytes(R)
    sc = torch.zeros(need, dtype=torch.uint8, device=DEV)
    loss = torch.full((1,), 7.0, device=DEV)

    def call(eps, nbytes):
        return L.voxe_orientation_fwd_bwd(C.byref(g), C.byref(c), ptr(p["ro"]), ptr(p["rd"]), R, None, None, eps, 1.0, ptr(loss), None,
                                          None, 0, ptr(sc), nbytes, stream_ptr(DEV))

    assert call(-1.0, need) == abi.ERR_BAD_SHAPE and call(float("inf"), need) == abi.ERR_BAD_SHAPE
    assert call(1e-2, need - 1) == abi.ERR_WORKSPACE
    torch.cuda.synchronize()
    assert float(loss) == 7.0 and int(sc.count_nonzero()) == 0
    assert call(0.0, need) == abi.OK
    torch.cuda.synchronize()
    assert float(loss) > 0.0 and float(loss) != 7.0


def test_loss_and_ray_loss_are_the_same_bits_from_run_to_run(base):
    for lanes in (1, 8):
        a, b = _again(base, lanes=lanes), _again(base, lanes=lanes)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert _rel_l2(a[2], b[2]) < 1e-6


def test_an_empty_relu_grid_gives_exact_zero(base):
    """sigma = 0 everywhere: every w is 0, and under ReLU at v < 0 post' is 0 too; G is not 0 (random negative raws) but the
    normals part carries the factor w"""
    spec = ops.GridSpec(aabb=H.AABB, density_scale=2.0, density_pre_act=abi.ACT_IDENTITY, density_post_act=abi.ACT_RELU)
    dens = -torch.rand((*H.DIMS, 1), generator=torch.Generator().manual_seed(2)).to(DEV) - 0.01
    for lanes in LANES:
        loss, ray, d = _call(spec, base["params"], dens, base["ro"], base["rd"], None, base["jitter"], base["rng"], lanes=lanes)
        assert float(loss) == 0.0 and int(ray.count_nonzero()) == 0 and int(d.count_nonzero()) == 0


def test_no_interference_with_a_forward_and_its_deterministic_backward():
    g = torch.Generator().manual_seed(8)
    dens0 = torch.empty((40, 40, 40, 1)).uniform_(-1, 1, generator=g).to(DEV)
    feat0 = torch.empty((40, 40, 40, 3)).uniform_(-1, 1, generator=g).to(DEV)
    spec = ops.GridSpec(aabb=((-1.5, 1.5),) * 3, density_scale=3.0)
    ro, rd = H.cameras(64, 1, DEV)
    params = ops.RenderParams(num_samples=64, near=workload.NEAR, far=workload.FAR, perturb=True, white_bkgd=True, image_width=64,
                              deterministic=True)
    g_col = torch.rand((ro.shape[0], 3), generator=torch.Generator().manual_seed(2)).to(DEV)
    grads = []
    for with_term in (False, True):
        d, f = dens0.clone().requires_grad_(True), feat0.clone().requires_grad_(True)
        ws = ops.Workspace()
        col = ops.render(spec, params, d, f, ro, rd, workspace=ws, rng=(3, 4))[0]
        if with_term:
            loss, ray, dd = _call(spec, params, d, ro, rd, rng=(3, 4))
            assert float(loss) > 1e-3 and float(dd.abs().max()) > 0
        (col * g_col).sum().backward()
        grads.append((d.grad.clone(), f.grad.clone()))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    assert float(grads[0][0].abs().max()) > 0


# ---- 4: the buffer contract (tests/contract.py, tests/arena.py) ---------------------------------------------------------
def _scene(name):
    import test_buffer_contract_gpu as BC

    return BC, BC.scene(name)


def _contract_weights(sc):
    rng = np.random.default_rng(sc.R)
    return (rng.uniform(0.0, 2.0, sc.R) * (rng.uniform(size=sc.R) > 0.2)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _contract_reference(name):
    BC, sc = _scene(name)
    spec = ops.GridSpec(aabb=BC.AABB, density_scale=BC.SCALE, density_pre_act=abi.ACT_IDENTITY, density_post_act=abi.ACT_SOFTPLUS,
                        feature_kind=sc.kind)
    params = ops.RenderParams(num_samples=sc.S, near=BC.NEAR, far=BC.FAR, perturb=True)
    t = torch.from_numpy
    _, g64 = OR.loss_and_gradient(OR.orientation_host, spec, params, t(sc.dens), t(sc.feat), t(sc.ro), t(sc.rd),
                                  t(_contract_weights(sc)), rng=(5, 3))
    return g64.numpy().reshape(-1)


def orientation_case(k, name, with_loss):
    from contract import P
    from voxe_hip.runtime import lib, stream_ptr

    L, (BC, sc), st = lib(), _scene(name), stream_ptr(DEV)
    R = sc.R
    dens, ro, rd = k.inp("densities", sc.dens), k.inp("rays_o", sc.ro), k.inp("rays_d", sc.rd)
    omega = k.inp("ray_weight", _contract_weights(sc))
    g, c = sc.desc(dens.ptr, None), sc.cfg()
    loss = k.out("loss", 1) if with_loss else None
    ray_loss, d_dens = k.out("ray_loss", R), k.out("d_densities", sc.nvox)
    scr = k.scratch("scratch", L.voxe_orientation_scratch_bytes(R)) if with_loss else None
    k.begin()
    k.call(L.voxe_orientation_fwd_bwd, C.byref(g), C.byref(c), ro.ptr, rd.ptr, R, None, omega.ptr, 1e-2, 0.7,
           P(loss), ray_loss.ptr, d_dens.ptr, 0, P(scr), k.size(scr, "scratch") if scr else 0, st)
    k.bits(ray_loss)
    if with_loss:
        k.bits(loss)
    k.tol(d_dens, 0.7 * _contract_reference(name), GRAD_REL_L2)


def orientation_empty_case(k):
    """R == 0 with only the loss outputs: VOXE_OK, no launch (with a d_densities the header has it zeroed: not this case)"""
    from voxe_hip.runtime import lib, stream_ptr

    L, (BC, sc), st = lib(), _scene("packed_scatter"), stream_ptr(DEV)
    dens, ro, rd = k.inp("densities", sc.dens), k.inp("rays_o", sc.ro), k.inp("rays_d", sc.rd)
    omega = k.inp("ray_weight", _contract_weights(sc))
    g, c = sc.desc(dens.ptr, None), sc.cfg()
    loss, ray_loss = k.out("loss", 1), k.out("ray_loss", sc.R)
    scr = k.scratch("scratch", L.voxe_orientation_scratch_bytes(sc.R))
    k.begin()
    k.call(L.voxe_orientation_fwd_bwd, C.byref(g), C.byref(c), ro.ptr, rd.ptr, k.count(sc.R), None, omega.ptr, 1e-2, 1.0,
           loss.ptr, ray_loss.ptr, None, 0, scr.ptr, scr.nbytes, st)
    raise AssertionError("only run_empty() runs this case")


@pytest.mark.parametrize("name,with_loss", [("packed_scatter", True), ("tile_s33", False), ("views_tile", True)])
def test_buffer_contract(name, with_loss):
    from contract import run_contract

    run_contract(orientation_case, name, with_loss)


def test_buffer_contract_short_scratch_and_no_rays():
    from contract import run_empty, run_short

    run_short(orientation_case, "scratch", "packed_scatter", True)
    run_empty(orientation_empty_case)


# ---- the autograd op and the model ------------------------------------------------------------------------------------
def test_autograd_op_equals_the_direct_call(base):
    d = base["dens"].clone().requires_grad_(True)
    loss, ray = ops.orientation_loss(base["spec"], base["params"], d, base["ro"], base["rd"], base["omega"], base["jitter"],
                                     base["rng"], return_ray_loss=True)
    assert loss.dim() == 0 and torch.equal(loss.detach(), base["loss"]) and torch.equal(ray, base["ray"]) and not ray.requires_grad
    (2.5 * loss).backward()
    assert _rel_l2(d.grad, 2.5 * base["d"]) < 1e-5
    with torch.no_grad():
        again = ops.orientation_loss(base["spec"], base["params"], base["dens"], base["ro"], base["rd"], base["omega"],
                                     base["jitter"], base["rng"])
    assert torch.equal(again, base["loss"]) and not again.requires_grad


def test_gradient_through_the_volumetric_model():
    from thre3d_atom.modules.volumetric_model import VolumetricModel
    from thre3d_atom.rendering.volumetric.render_interface import Rays
    from thre3d_atom.thre3d_reprs.renderers import SHVoxGridRenderConfig, render_sh_voxel_grid
    from thre3d_atom.thre3d_reprs.voxels import VoxelGrid, VoxelSize
    from thre3d_atom.utils.imaging_utils import CameraBounds

    spec, params, dens, feat, ro, rd = T.fuzzy_inputs(DEV)
    vg = VoxelGrid(dens.clone(), feat.clone(), VoxelSize(*(3.0 / 32,) * 3), density_preactivation=torch.nn.Identity(),
                   density_postactivation=torch.nn.Softplus(), expected_density_scale=2.0, tunable=True)
    vm = VolumetricModel(vg, render_sh_voxel_grid, SHVoxGridRenderConfig(64, CameraBounds(workload.NEAR, workload.FAR),
                                                                         perturb_sampled_points=False), device=DEV)
    omega = T.ray_weights(ro.shape[0], DEV)
    loss = vm.orientation_loss(Rays(ro, rd), ray_weight=omega, normal_eps=0.05)
    loss.backward()
    want_loss, _, want = _call(spec, ops.RenderParams(num_samples=64, near=workload.NEAR, far=workload.FAR), dens, ro, rd, omega, eps=0.05)
    got_loss = float(loss.detach())
    assert abs(got_loss - float(want_loss)) <= 1e-6 * float(want_loss) and got_loss > 1e-3
    assert vg.densities.grad is not None and _rel_l2(vg.densities.grad, want) < 1e-5 and vg.features.grad is None


# ---- 5: descent on the fuzzy ball -------------------------------------------------------------------------------------
def test_descent_on_the_fuzzy_ball():
    """fixture: test_orientation_host.fuzzy_inputs, whose float64 descent is checked there: FUZZY_STEPS Adam steps on the term
    alone reach the restatement's loss ratio plus a quarter of its distance to 1, and no voxel moves further than it does in the
    restatement plus 10 %"""
    spec, params, dens, feat, ro, rd = T.fuzzy_inputs(DEV)
    losses, final = T.fuzzy_descent(lambda d: ops.orientation_loss(spec, params, d, ro, rd), dens, torch.float32)
    ratio, move = losses[-1] / losses[0], float((final - dens).abs().max())
    print(f"fuzzy ball: loss {losses[0]:.6f} -> {losses[-1]:.6f} (ratio {ratio:.4f}; float64 restatement {T.FUZZY_LOSS_RATIO}); largest "
          f"move {move:.4f} (restatement {T.FUZZY_MAX_MOVE})")
    assert losses[0] > 1e-3
    assert ratio <= T.FUZZY_LOSS_RATIO + 0.25 * (1.0 - T.FUZZY_LOSS_RATIO)
    assert move <= 1.1 * T.FUZZY_MAX_MOVE


# ---- 6: the trainer -------------------------------------------------------------------------------------------------------
class _Capture(logging.Handler):
    def __init__(self):
        super().__init__()
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def test_trainer_with_the_orientation_term_on_both_optimiser_paths(tmp_path):
    import re

    from test_trainers_gpu import _sphere_model
    from thre3d_atom.data.datasets import InMemoryPosedImages
    from thre3d_atom.modules.trainers import train_sh_vox_grid_vol_mod_with_posed_images
    from thre3d_atom.modules.volumetric_model import VolumetricModel
    from thre3d_atom.thre3d_reprs.renderers import SHVoxGridRenderConfig, render_sh_voxel_grid
    from thre3d_atom.thre3d_reprs.voxels import VoxelGrid, VoxelSize
    from thre3d_atom.utils.imaging_utils import CameraBounds, CameraIntrinsics, pose_spherical
    from thre3d_atom.utils.logging import log

    # the synthetic views of the depth trainer test
    torch.manual_seed(1)
    truth = _sphere_model(side=24, samples=96)
    intr = CameraIntrinsics(48, 48, 0.5 * 48 / np.tan(0.5 * 0.6911112))
    poses, images = [], []
    for i in range(16):
        pose = pose_spherical(360.0 * i / 16, 20.0 + 50.0 * ((i * 0.618) % 1.0), 4.0311)
        poses.append(torch.cat([pose.rotation, pose.translation], dim=1))
        images.append(truth.render(pose, intr, perturb_sampled_points=False).colour.permute(2, 0, 1).cpu())
    data = InMemoryPosedImages(torch.stack(images), torch.stack(poses), intr, CameraBounds(1.8, 6.6))

    def run(fused, out, **kw):
        torch.manual_seed(5)
        g = torch.Generator().manual_seed(3)
        vg = VoxelGrid(torch.empty(24, 24, 24, 1).uniform_(-1, 1, generator=g), torch.empty(24, 24, 24, 3).uniform_(-1, 1, generator=g),
                       VoxelSize(0.125, 0.125, 0.125), density_preactivation=torch.nn.Identity(),
                       density_postactivation=torch.nn.Softplus(), expected_density_scale=100.0 / 3.0, tunable=True)
        vm = VolumetricModel(vg, render_sh_voxel_grid, SHVoxGridRenderConfig(96, CameraBounds(1.8, 6.6), white_bkgd=True), device=DEV)
        cap = _Capture()
        log.addHandler(cap)
        try:
            # (the initializer is the identity: the runs start from the same grid)
            train_sh_vox_grid_vol_mod_with_posed_images(vm, data, out, random_initializer=lambda t: t, ray_batch_size=4096,
                                                        num_stages=1, num_iterations_per_stage=3, summary_freq=1,
                                                        fast_debug_mode=True, fused_grid_step=fused, **kw)
        finally:
            log.removeHandler(cap)
        return vm.thre3d_repr.densities.detach().clone(), cap.lines

    def logged(lines, term):
        return [float(m.group(1)) for m in (re.search(term + r":\s*([-+0-9.eE]+|nan|inf)", line) for line in lines) if m]

    # weight 0: the one-call iteration, no word of the term
    base, lines0 = run(True, tmp_path / "w0")
    assert not any("orientation" in line or "no one-call iteration" in line for line in lines0)
    for kw in (dict(orientation_weight=0.1), dict(orientation_weight=0.1, distortion_weight=0.01)):
        finals = {}
        for fused in (True, False):
            dens, lines = run(fused, tmp_path / f"w{len(kw)}_{int(fused)}", **kw)
            values = logged(lines, "orientation")
            print(f"{kw} fused_grid_step {fused}: orientation {values}")
            assert len(values) == 3 and all(np.isfinite(v) and v > 0 for v in values)
            assert all(np.isfinite(v) for v in logged(lines, "loss")) and len(logged(lines, "loss")) == 3
            if "distortion_weight" in kw:
                assert len(logged(lines, "distortion")) == 3
            assert not torch.equal(dens, base) and bool(torch.isfinite(dens).all())
            if fused:
                assert sum("orientation_weight > 0" in line and "no one-call iteration" in line for line in lines) == (
                    0 if "distortion_weight" in kw else 1)
            finals[fused] = dens
        err = _rel_l2(finals[True], finals[False])
        print(f"{kw}: final densities, FusedGridAdam vs VoxeAdam: rel_l2 {err:.3e}")
        assert err < 1e-5
