"""The trainer's composed (not one-call) iteration against its float64 restatement tests/iteration_ref.py.

train_sh_vox_grid_vol_mod_with_posed_images runs two iterations of one stage on tiny data (a 14 x 12 x 10 grid in a 2.8 x 2.4 x 2.0
box, 16 views of 32 x 32, 32 samples per ray, no jitter).  Wrappers that change nothing record what each iteration drew (flat pixel
indices and picks, target pixels, image ids, the keypoint rows of the depth batch, the robust mask) and every parameter tensor as
it stands when the iteration begins; the optimisers are only kept a handle on.  The observable is Adam's first moment, in API
layout on both optimiser paths: exp_avg = (1 - beta1) g1 after one step and beta1 (1 - beta1) g1 + (1 - beta1) g2 after two,
where Adam's normalisation has not yet amplified rounding.  g1 and g2 are the restatement's gradients at the recorded
parameters.  The second step is what sees a gradient region that was not cleared, a packed grid that was not refreshed after a
step with extra gradients, or a `.grad` that lingered.

Bounds (none invented here).  rel-L2 <= 1e-4 for every tensor: for densities and features it is the project's bound of a render
gradient against its reference (tests/test_hip_configs.py); for the background texels tests/test_background_gpu.py's
GRAD_REL_L2; for the pose deltas and the intrinsics the bound tests/test_ray_grad_gpu.py holds the ray gradients to, of which both
are the linear image through the cast's backward (whose own bounds, 1e-6 and 4.4e-6 in tests/test_camera_gpu.py, lie below it); for
the exposure deltas tests/test_exposure_gpu.py bounds each element by a few 2^-24 of its sum of |terms| for exact float32 inputs,
which the composed iteration does not have: its colours carry the render's own error.  Their bound is that per-op bound plus
the named source, the project's colour bound (5e-6, 6e-6 behind the background composite) pushed through the affine backward
(iteration_ref.exposure_gradient_bound), taken through the first moment as a rel-L2 and never above 1e-4: about 1e-5 without the
SSIM term, 1e-4 with it (the SSIM gradient's own 1e-4 dominates).  The loss: every term's value is held by its own GPU test to max(4 x float32 torch's error, 1e-6), the
largest figure asserted anywhere being 2e-5 (tests/test_depth_gpu.py, plain); the composed loss is held to 2e-5 x the sum of the
active weights (each L1 term counting 1), and the logged line, which prints three decimals, to that plus 5e-4.

Every term must be visible: on the batches the runs drew, every active term holds at least 1 % of the gradient of each grid
tensor it reaches, and the sum without or with twice any term lies outside the bound of the run's own gradient
(test_iteration_host.assert_every_term_is_visible).  The distortion, depth and orientation terms reach the densities only (their
kernels have no feature gradient), and the exposure regulariser no grid tensor at all.  The robust mask is compared with the
restatement's own, whose residuals keep a gap around the quantile (assert_mask_is_off_the_edges).  One edge condition is NOT
asserted as literally stated: "no 3 x 3 count lies exactly at its cut" cannot hold, the cut being the integer count 5 of 9 that
many pixels of any batch reach.  A count moves only when an inlier flag flips, which the gap around the quantile excludes; what
is asserted is that gap (1e-4, relative), no patch's count of forgiven pixels at its cut, and a patch cut f P^2 that is no integer.  No ray, voxel or element is
exempt from any figure.  The smallest |residual| of the L1 terms is printed: their gradient is the residual's sign.
One term cannot be made visible and is not a grid term: exposure_regularization * mean(delta^2) has no gradient at the deltas'
zero start and about 1e-7 of the L1's after one step of 1e-3; its value enters the loss check, its gradient no figure.

Layouts.  In the deferred-gradient mode every render of a step is asked for the linear layout (ops._RenderFn sets linear_grad), so
abi.GRAD_LINEAR is what every fused case reports and no batch shape can make the region bricked: the layout query of ops
(predicted_grad_layout, which does not set linear_grad) names GRAD_BRICKED for the 300- and 576-ray batches and GRAD_LINEAR for
16384 rays, and the mode reported GRAD_LINEAR at every step.  What a batch shape does change is the render route: 2 for the small
batches, 3 for `plain_large` (L1, diffuse and distortion over 16384 rays), which is there for that.  Both are recorded per case.

Measured on an MI355X (profiles/iteration_pytest_gpu.log), worst rel-L2 of exp_avg over all cases, paths and both steps:
    densities 5.3e-06 (one_background)   features 1.2e-06   texels 5.0e-07   poses 2.2e-06   intrinsics 7.6e-07 (all_ssim, both
    paths alike); exposure 4.3e-07 with the SSIM term (bound 1.0e-04) and 4.9e-08 without (bounds 0.9e-05 .. 1.2e-05);
    |loss - restatement| at most 6.4e-08 (bounds 2.0e-05 .. 4.6e-05); the robust masks are equal; the smallest |residual| of a ray
    that meets the grid was 1.6e-06 (plain_large, 49152 residuals).  The whole file takes 7 s.  The log's header lists what
    halving or removing four of the trainer's terms did to these tests."""
import logging
import re

import numpy as np
import pytest
import torch

import iteration_ref as IR
import ray_grad_ref as RR
import test_iteration_host as TH
from voxe_hip import abi, ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BOUNDS = {"densities": IR.BOUND, "features": IR.BOUND, "texels": 1e-4, "exposure": 1e-4, "poses": 1e-4, "intrinsics": 1e-4}
TERM_VALUE_ABS = 2e-5
LOG_DECIMALS = 5e-4
COLOUR_ABS = 5e-6            # the project's bound of a rendered colour (tests/test_ray_grad_host.py)
COMPOSITE_ABS = 1e-6         # and of the background composite on top of it (tests/test_background_gpu.py)
# torch.manual_seed of each case's run.  The robust case needs two batches that keep the mask off its edges, a condition on the
# inputs that about a quarter of all batches fail (rays that miss the grid all render the same background against the same white
# pixel, so their residuals tie, and 512 residuals lie about 4e-3 apart around their median): seeds 5 to 8 draw such batches (a
# tie at the quantile twice, a patch count at its cut, a gap of 7.9e-05) and 9 does not
SEEDS = {"all_robust": 9}
SEED = 5


def _render_images():
    """the synthetic views, rendered from the sphere model as the other trainer tests render theirs"""
    from test_trainers_gpu import _sphere_model
    from thre3d_atom.utils.imaging_utils import CameraIntrinsics, CameraPose

    torch.manual_seed(1)
    truth = _sphere_model(side=24, samples=64)
    intr = CameraIntrinsics(IR.HW, IR.HW, IR.FOCAL)
    out = []
    for pose in IR.view_poses():
        out.append(truth.render(CameraPose(pose[:, :3], pose[:, 3:]), intr, perturb_sampled_points=False).colour.permute(2, 0, 1).cpu())
    return torch.stack(out)


@pytest.fixture(scope="module")
def images():
    return _render_images()


def _probe(spec, params, dens, feat, ro, rd):
    return RR.probe_device(spec, params, dens.to(DEV), feat.to(DEV), ro.to(DEV).contiguous(), rd.to(DEV).contiguous())


class _Capture(logging.Handler):
    def __init__(self):
        super().__init__()
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


class _Recorder:
    """what the wrappers saw; nothing here alters a call"""

    def __init__(self, vm):
        self.vm, self.optimisers, self.iterations, self.in_depth = vm, [], [], False
        self.layouts, self.losses = [], []

    def named_parameters(self):
        vm, out = self.vm, {}
        grid = vm.thre3d_repr
        for opt in self.optimisers:
            for group in opt.param_groups:
                for p in group["params"]:
                    if p is grid.densities:
                        out["densities"] = (opt, p)
                    elif p is grid.features:
                        out["features"] = (opt, p)
                    elif vm.background is not None and p is vm.background.texels:
                        out["texels"] = (opt, p)
                    elif vm.exposure is not None and p is vm.exposure.delta:
                        out["exposure"] = (opt, p)
                    elif tuple(p.shape) == (IR.VIEWS, 6):
                        out["poses"] = (opt, p)
                    elif tuple(p.shape) == (4,):
                        out["intrinsics"] = (opt, p)
                    else:
                        raise AssertionError(f"an optimiser holds a parameter this test does not know: {tuple(p.shape)}")
        return out

    def moments(self):
        return {k: opt.state[p]["exp_avg"].detach().cpu().clone() for k, (opt, p) in self.named_parameters().items()
                if opt.state.get(p)}

    def begin_iteration(self):
        if self.iterations:
            self.iterations[-1]["moments_after"] = self.moments()
        self.iterations.append({"params": {k: p.detach().cpu().clone() for k, (_, p) in self.named_parameters().items()}})

    def finish(self):
        self.iterations[-1]["moments_after"] = self.moments()
        self.steps = {k: int(opt.state[p]["step"]) for k, (opt, p) in self.named_parameters().items()}


def _install(monkeypatch, rec):
    import thre3d_atom.modules.optim as optim
    import thre3d_atom.modules.trainers as trainers
    import thre3d_atom.rendering.volumetric.utils.misc as misc

    def keep_handle(cls):
        init = cls.__init__

        def wrapped(self, *a, **kw):
            init(self, *a, **kw)
            rec.optimisers.append(self)
        monkeypatch.setattr(cls, "__init__", wrapped)

    for cls in (optim.FusedGridAdam, optim.VoxeAdam, torch.optim.Adam):
        keep_handle(cls)

    fused_step = optim.FusedGridAdam.step

    def step(self, *a, **kw):
        d = self.workspace.deferred
        rec.layouts.append((None, False) if d is None else (d.layout, d.dirty))
        return fused_step(self, *a, **kw)
    monkeypatch.setattr(optim.FusedGridAdam, "step", step)

    cast_and_gather = misc._cast_and_gather

    def cast(camera_intrinsics, poses, images, flat_index, image_ids, differentiable, intrinsics, **kw):
        out = cast_and_gather(camera_intrinsics, poses, images, flat_index, image_ids, differentiable, intrinsics, **kw)
        it = rec.iterations[-1]
        prefix = "depth_" if rec.in_depth else ""
        it[prefix + "flat_index"] = flat_index.detach().cpu().clone()
        it[prefix + "rays32"] = (out[0].origins.detach().cpu().clone(), out[0].directions.detach().cpu().clone())
        if not rec.in_depth:
            it["picks"] = torch.as_tensor(image_ids).detach().cpu().clone()
            it["pixels"] = out[1].detach().cpu().clone()
            it["image_ids"] = out[2].detach().cpu().clone() if len(out) > 2 else None
        return out
    monkeypatch.setattr(misc, "_cast_and_gather", cast)
    monkeypatch.setattr(trainers, "_cast_and_gather", cast)

    def sampler(name):
        inner = getattr(trainers, name)

        def wrapped(*a, **kw):
            rec.begin_iteration()
            return inner(*a, **kw)
        monkeypatch.setattr(trainers, name, wrapped)

    sampler("sample_random_rays_and_pixels_from_cameras")
    sampler("sample_random_patches_and_pixels_from_cameras")

    depth_batch, depth_targets = trainers._depth_batch, trainers.depth_targets_on_rays

    def wrapped_depth_batch(*a, **kw):
        rec.in_depth = True
        try:
            out = depth_batch(*a, **kw)
        finally:
            rec.in_depth = False
        rec.iterations[-1]["depth_targets"] = tuple(t.detach().cpu().clone() for t in out[1:])
        return out

    def wrapped_depth_targets(rays, points):
        rec.iterations[-1]["depth_points"] = points.detach().cpu().clone()
        return depth_targets(rays, points)
    monkeypatch.setattr(trainers, "_depth_batch", wrapped_depth_batch)
    monkeypatch.setattr(trainers, "depth_targets_on_rays", wrapped_depth_targets)

    def mask_of(name, index):
        inner = getattr(trainers, name)

        def wrapped(*a, **kw):
            out = inner(*a, **kw)
            if kw.get("mask") is None:
                rec.iterations[-1]["mask"] = out[index].detach().cpu().clone()
            return out
        monkeypatch.setattr(trainers, name, wrapped)

    mask_of("robust_mask_on_patches", 0)
    mask_of("robust_loss_on_patches", 2)

    backward = torch.Tensor.backward

    def wrapped_backward(self, *a, **kw):
        if self.dim() == 0 and rec.iterations and "loss" not in rec.iterations[-1]:
            rec.iterations[-1]["loss"] = float(self.detach())
        return backward(self, *a, **kw)
    monkeypatch.setattr(torch.Tensor, "backward", wrapped_backward)


def _run(name, fused, images, monkeypatch, out_dir):
    from thre3d_atom.data.datasets import InMemoryPosedImages, SparsePoints
    from thre3d_atom.modules.trainers import train_sh_vox_grid_vol_mod_with_posed_images
    from thre3d_atom.modules.volumetric_model import VolumetricModel
    from thre3d_atom.thre3d_reprs.renderers import SHVoxGridRenderConfig, _render_params, render_sh_voxel_grid
    from thre3d_atom.thre3d_reprs.voxels import VoxelGrid, VoxelSize
    from thre3d_atom.utils.imaging_utils import CameraBounds, CameraIntrinsics
    from thre3d_atom.utils.logging import log

    degree, white, ray_batch, kw = IR.CASES[name]
    scene = IR.make_scene(images, white)
    data = InMemoryPosedImages(scene.images, scene.poses, CameraIntrinsics(IR.HW, IR.HW, IR.FOCAL), CameraBounds(IR.NEAR, IR.FAR),
                               sparse_points=SparsePoints(*scene.sparse))
    dens, feat = IR.initial_grid(degree)
    vg = VoxelGrid(dens, feat, VoxelSize(IR.VOXEL, IR.VOXEL, IR.VOXEL), density_preactivation=torch.nn.Identity(),
                   density_postactivation=torch.nn.Softplus(), expected_density_scale=IR.DENSITY_SCALE, tunable=True)
    config = SHVoxGridRenderConfig(IR.SAMPLES, CameraBounds(IR.NEAR, IR.FAR), perturb_sampled_points=False, white_bkgd=white)
    vm = VolumetricModel(vg, render_sh_voxel_grid, config, device=DEV)
    rec = _Recorder(vm)
    _install(monkeypatch, rec)
    cap = _Capture()
    log.addHandler(cap)
    torch.manual_seed(SEEDS.get(name, SEED))
    try:
        train_sh_vox_grid_vol_mod_with_posed_images(vm, data, out_dir, random_initializer=lambda t: t, ray_batch_size=ray_batch,
                                                    num_stages=1, num_iterations_per_stage=2, summary_freq=1, fast_debug_mode=True,
                                                    fused_grid_step=fused, **kw)
    finally:
        log.removeHandler(cap)
    rec.finish()
    spec = vm.thre3d_repr.voxe_grid_spec(attn=False)
    assert np.allclose(np.asarray(spec.aabb), np.asarray(scene.spec.aabb), rtol=0, atol=1e-12)
    assert (spec.density_scale, spec.density_pre_act, spec.density_post_act) == \
        (scene.spec.density_scale, scene.spec.density_pre_act, scene.spec.density_post_act)
    grid = vm.thre3d_repr
    params = _render_params(grid, None, config, attn=False)
    R = rec.iterations[0]["flat_index"].numel()
    rec.route = ops._route(*ops._descs(spec, params, grid.densities, grid.features, 0, 0, False), R)
    rec.predicted_layout = ops.predicted_grad_layout(spec, params, grid.densities, grid.features, R)
    rec.logged = [float(m.group(1)) for m in (re.search(r"loss:\s*([-+0-9.eE]+|nan|inf)", line) for line in cap.lines) if m]
    return scene, rec


def _batch_of(scene, it):
    """the restatement's batch of one recorded iteration; what the restatement re-derives itself is checked against the record"""
    batch = {"picks": it["picks"], "flat_index": it["flat_index"], "rays32": it["rays32"]}
    if "depth_points" in it:
        xyz = scene.sparse[2]
        match = (it["depth_points"][:, None, :] == xyz[None, :, :]).all(dim=-1)
        assert bool((match.sum(dim=1) == 1).all())
        rows = match.float().argmax(dim=1)
        per = IR.HW * IR.HW
        cam = torch.div(it["depth_flat_index"], per, rounding_mode="floor")
        # (the keypoint's nearest pixel, in a camera that sees it)
        assert torch.equal(IR.depth_flat_index(scene, cam, rows), it["depth_flat_index"])
        seen_by = torch.searchsorted(scene.sparse[0], rows, right=True) - 1
        assert torch.equal(seen_by, it["picks"][cam])
        batch.update(depth_rows=rows, depth_flat_index=it["depth_flat_index"], depth_rays32=it["depth_rays32"])
    return batch


def _check(name, fused, scene, rec):
    kw = IR.CASES[name][3]
    options = IR.options_of(kw)
    assert len(rec.iterations) == 2 and len(rec.logged) == 2
    results = []
    for i, it in enumerate(rec.iterations):
        res = IR.evaluate(scene, options, it["params"], _batch_of(scene, it), probe=_probe)
        aux = res["aux"]
        # the batch as the restatement gathers it is the batch the run saw
        assert torch.equal(aux["pixels"], it["pixels"].double())
        if it["image_ids"] is not None:
            assert torch.equal(aux["image_ids"], it["image_ids"].long())
        assert float((aux["rays"][1] - it["rays32"][1].double()).abs().max()) <= 1e-5        # the float64 recast is the run's cast
        if "depth_targets" in it:
            for got, want in zip(it["depth_targets"], aux["depth_targets"]):
                assert float((got.double() - want).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max()))
        if "robust" in aux:
            # (a condition on the inputs: if it fails, the batches have moved and SEEDS needs another seed for this case)
            TH.assert_mask_is_off_the_edges(aux["robust"])
            assert torch.equal(it["mask"].reshape(-1).double(), aux["mask"]), (name, i)
            print(f"{name} fused {fused} it {i + 1}: mask equal; inliers / forgiven / mask {aux['robust']['stats']}, "
                  f"gap around the quantile {aux['robust']['gap']:.2e}")
        print(f"{name} fused {fused} it {i + 1}: smallest |residual| of the rays that meet the grid {aux['min_abs_residual']:.2e}; "
              f"terms " + "  ".join(f"{t} {v:.6f}" for t, v in res["values"].items()))
        results.append(res)
    names = list(results[0]["sum"])
    assert set(names) == set(rec.iterations[0]["params"]) == set(rec.steps)
    run_g1 = {k: rec.iterations[0]["moments_after"][k].double() / (1.0 - IR.BETA1) for k in names}
    TH.assert_every_term_is_visible(name, results[0], run=run_g1)
    TH.assert_every_term_is_visible(name, results[1])
    failures = []
    for k in names:
        want = IR.first_moments(results[0]["sum"][k], results[1]["sum"][k])
        bounds = (BOUNDS[k], BOUNDS[k])
        if k == "exposure":
            # the per-op bound with the render's colour error pushed through the affine backward, through Adam's first moment
            # (two float32 roundings of its own, voxe_grid_elem.hpp), as a rel-L2; never above the project's 1e-4
            eps = COLOUR_ABS + (COMPOSITE_ABS if "texels" in names else 0.0)
            each = [IR.exposure_gradient_bound(results[i], rec.iterations[i]["params"]["exposure"].numpy(), eps) for i in (0, 1)]
            derived = IR.first_moments(*each)
            bounds = tuple(min(BOUNDS[k], float(derived[i].norm() / want[i].norm()) + 2.0 * IR.U24) for i in (0, 1))
        for i in (0, 1):
            got = rec.iterations[i]["moments_after"][k]
            assert got.shape == want[i].shape and bool(torch.isfinite(got).all())
            err = IR.rel_l2(got, want[i])
            print(f"{name} fused {fused} exp_avg after step {i + 1} {k}: rel_l2 {err:.3e} (bound {bounds[i]:.2e})")
            if not err <= bounds[i]:
                failures.append((k, i + 1, err, bounds[i]))
    assert not failures, failures
    assert all(v == 2 for v in rec.steps.values()), rec.steps
    weights = 1.0 + float(options["diffuse"]) + sum(float(options.get(t + "_weight", 0.0)) for t in ("distortion", "depth", "orientation", "ssim"))
    margin = TERM_VALUE_ABS * weights
    for i in (0, 1):
        err = abs(rec.iterations[i]["loss"] - results[i]["total"])
        print(f"{name} fused {fused} it {i + 1}: loss {rec.iterations[i]['loss']:.7f} restatement {results[i]['total']:.7f} "
              f"|difference| {err:.2e} (bound {margin:.1e}); logged {rec.logged[i]:.3f}")
        assert err <= margin
        assert abs(rec.logged[i] - results[i]["total"]) <= margin + LOG_DECIMALS
    layouts = sorted({l for l, _ in rec.layouts if l is not None})
    print(f"{name} fused {fused}: R {rec.iterations[0]['flat_index'].numel()} route {rec.route} predicted layout "
          f"{rec.predicted_layout} deferred layouts at step {layouts} (GRAD_LINEAR {abi.GRAD_LINEAR}, GRAD_BRICKED {abi.GRAD_BRICKED})")
    if fused:
        assert len(rec.layouts) == 2 and all(dirty for _, dirty in rec.layouts) and layouts == [abi.GRAD_LINEAR]
    return rec.route


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("name", ["all_ssim", "all_robust"])
def test_every_term_at_once(name, fused, images, monkeypatch, tmp_path):
    scene, rec = _run(name, fused, images, monkeypatch, tmp_path)
    _check(name, fused, scene, rec)


@pytest.mark.parametrize("name", IR.ONE_TERM)
def test_one_term_alone_under_the_fused_step(name, images, monkeypatch, tmp_path):
    scene, rec = _run(name, True, images, monkeypatch, tmp_path)
    _check(name, True, scene, rec)


def test_the_other_render_route(images, monkeypatch, tmp_path):
    """L1, diffuse and distortion over 16384 rays; the small batches above all take one route, this one the other"""
    scene, rec = _run("plain_large", True, images, monkeypatch, tmp_path)
    route = _check("plain_large", True, scene, rec)
    from thre3d_atom.thre3d_reprs.renderers import _render_params

    grid = rec.vm.thre3d_repr
    params = _render_params(grid, None, rec.vm.render_config, attn=False)
    small = ops._route(*ops._descs(grid.voxe_grid_spec(attn=False), params, grid.densities, grid.features, 0, 0, False), 300)
    print(f"route of 16384 rays {route}, of 300 rays {small}")
    assert route != small
