"""GPU checks of the ray and camera-pose gradients (voxe_render_bwd_rays, voxe_cast_rays_bwd, ops.render with rays that require
grad, ops.cast_rays_from_poses, CameraPoseDeltas): agreement with the float64 restatement tests/ray_grad_ref.py for every
lanes-per-ray split, agreement with the reference's own autograd (tests/golden/ray_grads.npz), the call's semantics, the autograd
glue, the ray casting's backward, and pose recovery.  The inputs come from tests/test_ray_grad_host.py.

Bound of every gradient comparison: rel-L2 over [R,3] <= max(4 x yardstick, 1e-4), the yardstick being the restatement's own
float32 run against its float64 run on the same probed samples; 1e-4 is the project's bound for render gradients."""
import numpy as np
import pytest
import torch

import ray_grad_ref as RR
import test_ray_grad_host as T
import test_visibility_host as H
from voxe_hip import ops, workload

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LANES = (0, 1, 2, 4, 8)          # 0: the dispatcher's choice by R
rel_l2 = T.rel_l2


def _call(p, lanes=0, g=("g_col", "g_dep", "g_acc"), **kw):
    ups = [p[k] if k in g else None for k in ("g_col", "g_dep", "g_acc")]
    return ops.render_bwd_rays(p["spec"], p["params"], p["dens"], p["feat"], p["ro"], p["rd"], p["jitter"], p["rng"], *ups,
                               lanes=lanes, **kw)


def _samples(p):
    return RR.probe_device(p["spec"], p["params"], p["dens"], p["feat"], p["ro"], p["rd"], p["jitter"], p["rng"])


def _check_against(p, want, yard, tag):
    """every lanes split against `want` = (d_o, d_d) under the bounds max(4 yard, 1e-4); exact zeros; splits among each other"""
    bounds = [max(4.0 * y, T.GRAD_REL_L2) for y in yard]
    results = []
    for lanes in LANES:
        got = _call(p, lanes)
        errs = [rel_l2(g, w) if float(w.norm()) > 0 else float(g.abs().max()) for g, w in zip(got, want)]
        print(f"{tag} lanes {lanes}: d_o rel_l2 {errs[0]:.3e} (float32 restatement {yard[0]:.3e})  d_d rel_l2 {errs[1]:.3e} "
              f"(float32 restatement {yard[1]:.3e})")
        results.append((lanes, got, errs))
    for lanes, got, errs in results:
        for g, w, e, b in zip(got, want, errs, bounds):
            assert e <= b, (tag, lanes, e, b)
            assert bool(torch.isfinite(g).all())
            # misses and empty fields: exact 0 (also where float64 keeps a softplus tail of 1e-260: T.assert_agreement_not_vacuous)
            assert bool((g[T.blind_rays(*want)[1]] == 0).all()), (tag, lanes)
    for _, got, _ in results[1:]:
        for g, g0, w, b in zip(got, results[0][1], want, bounds):
            if float(w.norm()) > 0:
                assert rel_l2(g, g0) <= 2 * b


# ---- 1: agreement with the restatement, every lanes-per-ray split -----------------------------------------------------
@pytest.mark.parametrize("pre,post", T.TD.ACTS)
@pytest.mark.parametrize("case,deg", T.agreement_cases(), ids=lambda v: v[0] if isinstance(v, tuple) else f"sh{v}")
def test_kernel_matches_the_restatement(case, deg, pre, post):
    """Measured over the cases and splits: abs + ReLU 3.6e-7 .. 2.6e-6, at most 1.94 x the yardstick of the case; identity +
    Softplus 1.0e-6 .. 6.0e-4, at most 1.01 x the yardstick of the case (the carved field's slopes of hundreds per cell amplify
    the float32 rounding of p = o + d z, which the kernel and the float32 restatement share: DESIGN.md 4.13)."""
    p = T.agreement_inputs(case, deg, pre, post, DEV)
    samples = _samples(p)
    want = T.restatement(p, samples)
    f32 = T.restatement(p, samples, dtype=torch.float32)
    S, R = p["params"].num_samples, p["ro"].shape[0]
    T.assert_agreement_not_vacuous(case, post, *want)          # both norms > 0 and, in the image cases, rays that see nothing
    yard = [rel_l2(a, b) for a, b in zip(f32, want)]
    _check_against(p, want, yard, f"{case[0]} sh{deg} pre {pre} post {post} R {R} S {S}")


@pytest.mark.parametrize("case", T.golden_cases())
def test_kernel_matches_the_restatement_on_the_golden_inputs(case):
    p = T.golden_inputs(case, DEV)
    samples = _samples(p)
    want = T.restatement(p, samples)
    f32 = T.restatement(p, samples, dtype=torch.float32)
    _check_against(p, want, [rel_l2(a, b) for a, b in zip(f32, want)], case)


# ---- 2: against the reference's own autograd --------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.golden_cases())
def test_kernel_matches_the_references_autograd(case):
    p = T.golden_inputs(case, DEV)
    samples = _samples(p)
    f64 = T.restatement(p, samples)
    f32 = T.restatement(p, samples, dtype=torch.float32)
    _check_against(p, (p["d_o"], p["d_d"]), [rel_l2(a, b) for a, b in zip(f32, f64)], case + " vs golden")


# ---- 3: semantics -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base():
    p = T.agreement_inputs(T.TD.agreement_cases()[1], 2, *T.TD.ACTS[0], DEV)     # hash jitter + clip, SH-2
    p["d_o"], p["d_d"] = _call(p)
    return p


def test_accumulate_null_arguments_and_empty_batches(base):
    R = base["ro"].shape[0]
    g = torch.Generator().manual_seed(1)
    pre_o, pre_d = torch.randn((R, 3), generator=g).to(DEV), torch.randn((R, 3), generator=g).to(DEV)
    o, d = _call(base, d_rays_o=pre_o.clone(), d_rays_d=pre_d.clone(), accumulate=True)
    assert torch.equal(o, pre_o + base["d_o"]) and torch.equal(d, pre_d + base["d_d"])
    # overwrite: garbage in the buffers does not matter
    o, d = _call(base, d_rays_o=torch.full((R, 3), float("nan"), device=DEV), d_rays_d=torch.full((R, 3), float("nan"), device=DEV))
    assert torch.equal(o, base["d_o"]) and torch.equal(d, base["d_d"])
    # each output NULL: the other one keeps its bits
    o, none = _call(base, want_d=False)
    assert none is None and torch.equal(o, base["d_o"])
    none, d = _call(base, want_o=False)
    assert none is None and torch.equal(d, base["d_d"])
    # each upstream gradient NULL == that gradient 0, and the three parts add up (the gradient is linear in them)
    parts = []
    for k in ("g_col", "g_dep", "g_acc"):
        alone = _call(base, g=(k,))
        zeros = dict(base, **{n: torch.zeros_like(base[n]) for n in ("g_col", "g_dep", "g_acc") if n != k})
        same = _call(zeros)
        assert torch.equal(alone[0], same[0]) and torch.equal(alone[1], same[1])
        assert float(alone[0].norm()) > 0 and float(alone[1].norm()) > 0
        parts.append(alone)
    for i in range(2):
        assert rel_l2(parts[0][i] + parts[1][i] + parts[2][i], (base["d_o"], base["d_d"])[i]) < 1e-5
    # R == 0
    e = torch.zeros((0, 3), device=DEV)
    o, d = ops.render_bwd_rays(base["spec"], base["params"], base["dens"], base["feat"], e, e, None, base["rng"], None, None, None)
    assert o.shape == (0, 3) and d.shape == (0, 3)


def test_two_calls_give_identical_bits(base):
    for lanes in LANES:
        a, b = _call(base, lanes), _call(base, lanes)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_a_rays_gradient_does_not_depend_on_the_launch_order():
    """image order against the same rays shuffled as a linear batch (no jitter: the hash stream follows a ray's index): each
    ray's gradient within the bound"""
    p = T.agreement_inputs(T.TD.agreement_cases()[0], 2, *T.TD.ACTS[0], DEV)      # plain image, no jitter
    R = p["ro"].shape[0]
    perm = torch.randperm(R, generator=torch.Generator().manual_seed(3)).to(DEV)
    q = dict(p, ro=p["ro"][perm].contiguous(), rd=p["rd"][perm].contiguous(), g_col=p["g_col"][perm].contiguous(),
             g_dep=p["g_dep"][perm].contiguous(), g_acc=p["g_acc"][perm].contiguous(),
             params=ops.RenderParams(**{**vars(p["params"]), "image_width": 0, "image_height": 0}))
    assert p["params"].image_width > 0
    a, b = _call(p), _call(q)
    for x, y in zip(a, b):
        assert rel_l2(y, x[perm]) <= T.GRAD_REL_L2 and float(x.norm()) > 0


def test_the_forward_record_of_a_workspace_is_not_touched(base):
    """a forward / backward of the same rays on a workspace, with the call in between forward and backward, gives the bits it
    gives without it (deterministic backward: two backward passes of one forward agree bit for bit)"""
    g = torch.Generator().manual_seed(8)
    dens0 = torch.empty((40, 40, 40, 1)).uniform_(-1, 1, generator=g).to(DEV)
    feat0 = torch.empty((40, 40, 40, 3)).uniform_(-1, 1, generator=g).to(DEV)
    spec = ops.GridSpec(aabb=((-1.5, 1.5),) * 3, density_scale=3.0)
    ro, rd = H.cameras(64, 1, DEV)
    params = ops.RenderParams(num_samples=64, near=workload.NEAR, far=workload.FAR, perturb=True, white_bkgd=True, image_width=64,
                              deterministic=True)
    g_col = torch.rand((ro.shape[0], 3), generator=torch.Generator().manual_seed(2)).to(DEV)
    outs = []
    for between in (False, True):
        d, f = dens0.clone().requires_grad_(True), feat0.clone().requires_grad_(True)
        ws = ops.Workspace()
        col = ops.render(spec, params, d, f, ro, rd, workspace=ws, rng=(3, 4))[0]
        if between:
            o, dd = ops.render_bwd_rays(spec, params, d, f, ro, rd, None, (3, 4), g_col, None, None)
            assert float(o.abs().max()) > 0 and float(dd.abs().max()) > 0
        (col * g_col).sum().backward()
        outs.append((col.detach().clone(), d.grad.clone(), f.grad.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert float(outs[0][1].abs().max()) > 0


# ---- 4: autograd glue -------------------------------------------------------------------------------------------------
def _render_loss(p, dens, feat, ro, rd, workspace=None):
    col, depth, acc, disp = ops.render(p["spec"], p["params"], dens, feat, ro, rd, p["jitter"], workspace=workspace, rng=p["rng"])
    return (col * p["g_col"]).sum() + (depth[:, 0] * p["g_dep"]).sum() + (acc[:, 0] * p["g_acc"]).sum()


def test_render_returns_ray_gradients_with_a_frozen_and_a_trainable_grid(base):
    p = base
    ro, rd = p["ro"].clone().requires_grad_(True), p["rd"].clone().requires_grad_(True)
    _render_loss(p, p["dens"], p["feat"], ro, rd).backward()                               # grid frozen
    assert torch.equal(ro.grad, p["d_o"]) and torch.equal(rd.grad, p["d_d"])
    # only one of the two
    ro1 = p["ro"].clone().requires_grad_(True)
    _render_loss(p, p["dens"], p["feat"], ro1, p["rd"]).backward()
    assert torch.equal(ro1.grad, p["d_o"])
    # grid trainable: the same ray gradients, and the grid's gradient bit for bit what it is without them
    q = T.agreement_inputs(T.TD.agreement_cases()[1], 0, *T.TD.ACTS[0], DEV)
    q["params"] = ops.RenderParams(**{**vars(q["params"]), "deterministic": True})     # (SH-0 image order: bit-reproducible backward)
    want_o, want_d = _call(q)
    grads = []
    for with_rays in (False, True):
        d, f = q["dens"].clone().requires_grad_(True), q["feat"].clone().requires_grad_(True)
        ro, rd = q["ro"].clone().requires_grad_(with_rays), q["rd"].clone().requires_grad_(with_rays)
        _render_loss(q, d, f, ro, rd).backward()
        grads.append((d.grad.clone(), f.grad.clone()))
        if with_rays:
            assert torch.equal(ro.grad, want_o) and torch.equal(rd.grad, want_d)
        else:
            assert ro.grad is None and rd.grad is None
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1]) and float(grads[0][0].abs().max()) > 0


def test_disparity_chains_into_the_ray_gradient(base):
    p = base
    ro, rd = p["ro"].clone().requires_grad_(True), p["rd"].clone().requires_grad_(True)
    col, depth, acc, disp = ops.render(p["spec"], p["params"], p["dens"], p["feat"], ro, rd, p["jitter"], rng=p["rng"])
    g_disp = torch.rand(disp.shape, generator=torch.Generator().manual_seed(4)).to(DEV)
    (disp * g_disp).sum().backward()
    gd, ga = ops.disparity_bwd(depth.detach(), acc.detach(), g_disp)
    want = ops.render_bwd_rays(p["spec"], p["params"], p["dens"], p["feat"], p["ro"], p["rd"], p["jitter"], p["rng"], None, gd, ga)
    assert torch.equal(ro.grad, want[0]) and torch.equal(rd.grad, want[1]) and float(want[1].norm()) > 0


def test_render_under_the_deferred_gradient_mode_still_returns_ray_gradients():
    from thre3d_atom.modules.optim import FusedGridAdam
    from thre3d_atom.thre3d_reprs.voxels import VoxelGrid, VoxelSize

    spec, params, dens, feat = T.pose_scene(DEV)
    ro, rd = H.cameras(T.POSE_HW, 1, DEV)
    g_col, g_dep, g_acc = T.upstream(ro.shape[0], DEV)
    vg = VoxelGrid(dens.clone(), feat.clone(), VoxelSize(*(3.0 / 16,) * 3), density_preactivation=torch.nn.Identity(),
                   density_postactivation=torch.nn.Softplus(), expected_density_scale=100.0 / 3.0, tunable=True)
    p = dict(spec=vg.voxe_grid_spec(attn=False), params=params, ro=ro, rd=rd, jitter=None, rng=(0, 0), g_col=g_col, g_dep=g_dep,
             g_acc=g_acc)
    q = p
    want = _call(dict(q, dens=vg.densities.detach(), feat=vg.features.detach()))
    opt = FusedGridAdam(vg, lr=1e-3, betas=(0.9, 0.999))
    try:
        ro, rd = p["ro"].clone().requires_grad_(True), p["rd"].clone().requires_grad_(True)
        _render_loss(q, vg.densities, vg.features, ro, rd, workspace=opt.workspace).backward()
        assert vg.densities.grad is None and vg.features.grad is None                  # deferred: the gradient stays in the workspace
        assert opt.workspace.deferred is not None and opt.workspace.deferred.dirty
        assert torch.equal(ro.grad, want[0]) and torch.equal(rd.grad, want[1]) and float(want[0].norm()) > 0
    finally:
        opt.detach()


# ---- 5: cast_rays_from_poses ------------------------------------------------------------------------------------------
def _poses(K, device):
    from thre3d_atom.utils.imaging_utils import pose_spherical

    out = []
    for i in range(K):
        pose = pose_spherical(*workload.synth_pose_angles(i + 1, 8), workload.RADIUS)
        out.append(torch.cat([torch.as_tensor(pose.rotation).float(), torch.as_tensor(pose.translation).float().reshape(3, 1)], dim=1))
    return torch.stack(out).to(device)


def test_cast_rays_from_poses_forward_bits_and_backward():
    """backward bound 1e-6 rel-L2: double sums of at most 192 terms, cast once"""
    K, hw, focal = 3, 8, workload.focal_for(8)
    poses = _poses(K, DEV)
    # forward: the bits of cast_rays (per camera) and of cast_rays_indexed
    ro, rd = ops.cast_rays_from_poses(hw, hw, focal, poses)
    for k in range(K):
        o, d = ops.cast_rays(hw, hw, focal, poses[k, :, :3].cpu(), poses[k, :, 3].cpu(), DEV)
        assert torch.equal(ro[k * 64:(k + 1) * 64], o) and torch.equal(rd[k * 64:(k + 1) * 64], d)
    g = torch.Generator().manual_seed(6)
    idx = torch.cat([torch.randperm(64, generator=g), 128 + torch.randperm(64, generator=g)])          # camera 1 absent
    idx = idx[torch.randperm(128, generator=g)].to(DEV)
    o, d = ops.cast_rays_indexed(hw, hw, focal, poses, idx)
    ro_i, rd_i = ops.cast_rays_from_poses(hw, hw, focal, poses, idx)
    assert torch.equal(ro_i, o) and torch.equal(rd_i, d)
    # backward against the float64 restatement: whole images, then the index batch
    for index in (None, idx):
        B = K * 64 if index is None else int(index.shape[0])
        g_o, g_d = torch.randn((B, 3), generator=g).to(DEV), torch.randn((B, 3), generator=g).to(DEV)
        p64 = poses.double().clone().requires_grad_(True)
        f64 = torch.tensor(focal, dtype=torch.float64, device=DEV, requires_grad=True)
        o64, d64 = RR.cast_rays(hw, hw, f64, p64, index)
        want_p, want_f = torch.autograd.grad((o64 * g_o).sum() + (d64 * g_d).sum(), (p64, f64))
        pt = poses.clone().requires_grad_(True)
        ft = torch.tensor(focal, dtype=torch.float32, requires_grad=True)
        o32, d32 = ops.cast_rays_from_poses(hw, hw, ft, pt, index)
        ((o32 * g_o).sum() + (d32 * g_d).sum()).backward()
        err_p, err_f = rel_l2(pt.grad, want_p), abs(float(ft.grad) - float(want_f)) / abs(float(want_f))
        print(f"cast_rays_from_poses backward ({'whole images' if index is None else 'index batch'}): d_poses rel_l2 {err_p:.3e}  "
              f"d_focal rel {err_f:.3e}")
        assert err_p <= 1e-6 and err_f <= 1e-6
        if index is not None:
            assert int(pt.grad[1].count_nonzero()) == 0 and int(pt.grad[0].count_nonzero()) == 12      # no ray: exact 0
        # the direct call: accumulate adds to the buffers, either upstream gradient may be missing
        d_poses, d_focal = ops.cast_rays_bwd(hw, hw, focal, poses, index, g_o, g_d, want_focal=True)
        assert rel_l2(d_poses, want_p) <= 1e-6
        acc_p, acc_f = ops.cast_rays_bwd(hw, hw, focal, poses, index, g_o, g_d, d_poses=torch.ones_like(d_poses),
                                         d_focal=torch.ones_like(d_focal), accumulate=True)
        assert rel_l2(acc_p - 1.0, want_p) <= 1e-5 and abs(float(acc_f) - 1.0 - float(want_f)) <= 1e-5 * abs(float(want_f))
        only_o, _ = ops.cast_rays_bwd(hw, hw, focal, poses, index, g_o, None)
        assert int(only_o[:, :, :3].count_nonzero()) == 0 and rel_l2(only_o[:, :, 3], want_p[:, :, 3]) <= 1e-6


# ---- 6: pose recovery -------------------------------------------------------------------------------------------------
def test_pose_recovery():
    """the host test's scene and conditions with the kernels: cast_rays_from_poses -> ops.render -> MSE, Adam on the deltas"""
    from thre3d_atom.thre3d_reprs.poses import CameraPoseDeltas, rotation_error_degrees, translation_error

    spec, params, dens, feat = T.pose_scene(DEV)
    true, noisy, focal = T.pose_cameras(DEV)
    hw, per = T.POSE_HW, T.POSE_HW * T.POSE_HW
    params = ops.RenderParams(**{**vars(params), "image_width": hw, "image_height": hw})
    ws = ops.Workspace()

    def render(poses):
        ro, rd = ops.cast_rays_from_poses(hw, hw, focal, poses)
        return ops.render(spec, params, dens, feat, ro, rd, workspace=ws)[0]

    with torch.no_grad():
        target = render(true)
    deltas = CameraPoseDeltas(3).to(DEV)
    opt = torch.optim.Adam(deltas.parameters(), lr=T.POSE_LR)
    losses = []
    for step in range(T.POSE_STEPS + 1):
        opt.zero_grad()
        loss = ((render(deltas.apply(noisy)) - target) ** 2).reshape(3, per, 3).mean(dim=(1, 2)).sum()
        losses.append(loss.detach())
        if step < T.POSE_STEPS:
            loss.backward()
            opt.step()
    losses = [float(v) for v in torch.stack(losses).cpu()]
    final = deltas.apply(noisy).detach()
    T.assert_pose_recovery(losses, rotation_error_degrees(noisy, true).cpu(), rotation_error_degrees(final, true).cpu(),
                           translation_error(noisy, true).cpu(), translation_error(final, true).cpu())


# ---- 7: the trainer and the command-line tool -------------------------------------------------------------------------
def _synthetic_views(n, hw=48):
    from test_trainers_gpu import _sphere_model
    from thre3d_atom.utils.imaging_utils import CameraIntrinsics, pose_spherical

    torch.manual_seed(1)
    truth = _sphere_model(side=24, samples=96)
    intr = CameraIntrinsics(hw, hw, 0.5 * hw / np.tan(0.5 * 0.6911112))
    poses, images = [], []
    for i in range(n):
        pose = pose_spherical(360.0 * i / n, 20.0 + 50.0 * ((i * 0.618) % 1.0), 4.0311)
        poses.append(torch.cat([pose.rotation, pose.translation], dim=1))
        images.append(truth.render(pose, intr, perturb_sampled_points=False).colour.permute(2, 0, 1).cpu())
    return truth, torch.stack(images), torch.stack(poses), intr


def test_trainer_with_pose_refinement_on_both_optimiser_paths(tmp_path):
    import json
    import logging
    import re

    from thre3d_atom.data.datasets import InMemoryPosedImages
    from thre3d_atom.modules.trainers import train_sh_vox_grid_vol_mod_with_posed_images
    from thre3d_atom.modules.volumetric_model import VolumetricModel
    from thre3d_atom.thre3d_reprs.renderers import SHVoxGridRenderConfig, render_sh_voxel_grid
    from thre3d_atom.thre3d_reprs.voxels import VoxelGrid, VoxelSize
    from thre3d_atom.utils.imaging_utils import CameraBounds
    from thre3d_atom.utils.logging import log

    _, images, poses, intr = _synthetic_views(16)
    data = InMemoryPosedImages(images, poses, intr, CameraBounds(1.8, 6.6))

    class Capture(logging.Handler):
        def __init__(self):
            super().__init__()
            self.lines = []

        def emit(self, record):
            self.lines.append(record.getMessage())

    def run(fused, out, **kw):
        torch.manual_seed(5)
        g = torch.Generator().manual_seed(3)
        vg = VoxelGrid(torch.empty(24, 24, 24, 1).uniform_(-1, 1, generator=g), torch.empty(24, 24, 24, 3).uniform_(-1, 1, generator=g),
                       VoxelSize(0.125, 0.125, 0.125), density_preactivation=torch.nn.Identity(),
                       density_postactivation=torch.nn.Softplus(), expected_density_scale=100.0 / 3.0, tunable=True)
        vm = VolumetricModel(vg, render_sh_voxel_grid, SHVoxGridRenderConfig(96, CameraBounds(1.8, 6.6), white_bkgd=True), device=DEV)
        cap = Capture()
        log.addHandler(cap)
        try:
            # (the initializer is the identity: every run starts from the same grid)
            train_sh_vox_grid_vol_mod_with_posed_images(vm, data, out, random_initializer=lambda t: t, ray_batch_size=4096,
                                                        num_stages=1, num_iterations_per_stage=3, summary_freq=1,
                                                        fast_debug_mode=True, fused_grid_step=fused, **kw)
        finally:
            log.removeHandler(cap)
        return vm.thre3d_repr.densities.detach().clone(), vm.thre3d_repr.features.detach().clone(), cap.lines

    for fused in (True, False):
        parent = run(fused, tmp_path / f"parent_{int(fused)}")                            # the argument not given at all
        zero = run(fused, tmp_path / f"zero_{int(fused)}", pose_learning_rate=0.0)
        # (two runs of one command differ in the last bits: the render backward adds with float atomics.  1e-4 is the bound
        #  tests/test_distortion_gpu.py holds the two optimiser paths of this trainer to; that 0 takes the parent's code path,
        #  call for call, is tests/test_ray_grad_host.py::test_pose_learning_rate_zero_leaves_the_one_call_iteration)
        err = max(rel_l2(zero[0], parent[0]), rel_l2(zero[1], parent[1]))
        print(f"fused_grid_step {fused}: pose_learning_rate 0 against the argument not given: rel_l2 {err:.3e}")
        assert err < 1e-4
        assert not (tmp_path / f"zero_{int(fused)}" / "saved_models" / "refined_train_camera_params.json").exists()
        assert not any("pose_learning_rate" in line for line in zero[2])
        dens, feat, lines = run(fused, tmp_path / f"rate_{int(fused)}", pose_learning_rate=1e-3)
        losses = [float(m.group(1)) for m in (re.search(r"loss:\s*([-+0-9.eE]+|nan|inf)", line) for line in lines) if m]
        assert len(losses) == 3 and all(np.isfinite(v) for v in losses)
        assert bool(torch.isfinite(dens).all()) and bool(torch.isfinite(feat).all()) and not torch.equal(dens, parent[0])
        assert sum("no one-call iteration" in line for line in lines) == (1 if fused else 0)
        saved = json.loads((tmp_path / f"rate_{int(fused)}" / "saved_models" / "refined_train_camera_params.json").read_text())
        refined = torch.tensor([[r + t for r, t in zip(e["extrinsic"]["rotation"], e["extrinsic"]["translation"])]
                                for _, e in sorted(saved.items())])
        moved = (refined - poses).abs().amax(dim=(1, 2))
        print(f"fused_grid_step {fused}: losses {losses}; cameras moved by {[round(float(v), 5) for v in moved]}")
        # three Adam steps at 1e-3 move a delta by at most 3e-3; cameras that were drawn moved, none jumped
        assert float(moved.max()) > 1e-4 and float(moved.max()) < 1e-2 and int((moved > 0).sum()) >= 8


def test_refine_camera_poses_command_line(tmp_path):
    import importlib.util
    import os
    import re

    from click.testing import CliRunner
    from PIL import Image

    from conftest import ROOT
    from thre3d_atom.data.datasets import InMemoryPosedImages, PosedImagesDataset
    from thre3d_atom.thre3d_reprs.poses import (axis_angle_to_matrix, rotation_error_degrees, translation_error,
                                                write_camera_params)
    from thre3d_atom.utils.constants import CAMERA_BOUNDS, CAMERA_INTRINSICS, HEMISPHERICAL_RADIUS
    from thre3d_atom.utils.imaging_utils import CameraBounds

    truth, images, poses, intr = _synthetic_views(3)
    bounds = CameraBounds(1.8, 6.6)
    torch.save(truth.get_save_info({CAMERA_BOUNDS: bounds, CAMERA_INTRINSICS: intr, HEMISPHERICAL_RADIUS: 4.0311}), tmp_path / "model.pth")
    (tmp_path / "data" / "train").mkdir(parents=True)
    for i in range(3):
        Image.fromarray((images[i].permute(1, 2, 0).clamp(0, 1).numpy() * 255 + 0.5).astype(np.uint8)).save(
            tmp_path / "data" / "train" / f"{i:04d}.png")
    g = torch.Generator().manual_seed(9)
    w = torch.randn(3, 3, generator=g)
    w = w / w.norm(dim=1, keepdim=True) * float(np.radians(2.0))
    noisy = torch.cat([axis_angle_to_matrix(w) @ poses[:, :, :3], poses[:, :, 3:] + 0.05 * torch.randn(3, 3, 1, generator=g)], dim=2)
    write_camera_params(tmp_path / "data" / "train_camera_params.json", InMemoryPosedImages(images, noisy, intr, bounds), noisy)
    spec = importlib.util.spec_from_file_location("refine_camera_poses_cli", os.path.join(ROOT, "refine_camera_poses.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.manual_seed(2)
    res = CliRunner().invoke(mod.main, ["-i", str(tmp_path / "model.pth"), "-d", str(tmp_path / "data"), "-o", str(tmp_path / "out"),
                                        "--num_iterations", "60", "--ray_batch_size", "4096"])
    assert res.exit_code == 0, (res.output, res.exception)
    first, last = (float(v) for v in re.search(r"mse ([0-9.eE+-]+) -> ([0-9.eE+-]+)", res.output).groups())
    back = PosedImagesDataset(tmp_path / "data" / "train", tmp_path / "out" / "refined_train_camera_params.json")
    rot0, rot1 = rotation_error_degrees(noisy, poses), rotation_error_degrees(back.poses, poses)
    print(f"refine_camera_poses: mse {first:.3e} -> {last:.3e}; rotation error {[round(float(v), 3) for v in rot0]} -> "
          f"{[round(float(v), 3) for v in rot1]} deg; translation error "
          f"{[round(float(v), 4) for v in translation_error(noisy, poses)]} -> "
          f"{[round(float(v), 4) for v in translation_error(back.poses, poses)]}")
    assert last < first and tuple(back.poses.shape) == (3, 3, 4) and not torch.equal(back.poses, noisy)
    assert float(rot1.mean()) < float(rot0.mean())
