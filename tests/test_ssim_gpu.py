"""SSIM on the GPU: voxe_ssim_fwd_bwd against the float64 restatement tests/ssim_ref.py with the bounds that file
states (yardstick: the float32 torch restatement's own error on the same inputs), the call's semantics, the autograd op behind a
render, the patch sampler, the held-out tester and the trainer's D-SSIM term."""
import logging
import re

import numpy as np
import pytest
import torch

import ssim_ref as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from voxe_hip import ops

    DEV = torch.device("cuda:0")


def _call(x, y, grad=True, **kw):
    d_x = kw.pop("out", None)
    if grad and d_x is None:
        d_x = torch.full_like(x, float("nan"))
    mean, per, smap = ops.ssim_fwd_bwd(x, y, want_map=kw.pop("want_map", True), d_x=d_x, **kw)
    return mean, per, smap, d_x


# ---- 1: agreement with the float64 restatement --------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "{}-n{}-{}x{}x{}".format(*c))
def test_ssim_matches_the_restatement(case):
    ref = R.reference(case)
    x, y = ref["x"].to(DEV), ref["y"].to(DEV)
    mean, per, smap, d_x = _call(x, y)
    mean, per, smap, d_x = (t.cpu().double() for t in (mean, per, smap, d_x))
    err_map, err_per = float((smap - ref["map"]).abs().max()), float((per - ref["per_image"]).abs().max())
    err_mean, err_grad = abs(float(mean) - float(ref["mean"])), R.rel_l2(d_x, ref["grad"])
    err_abs = float((d_x - ref["grad"]).abs().max())
    print(f"{case}: ssim {float(mean):.4f}  max|err| map {err_map:.2e} (bound {ref['bound_map']:.2e}) per_image {err_per:.2e} "
          f"({ref['bound_per_image']:.2e}) mean {err_mean:.2e} ({ref['bound_mean']:.2e})  gradient rel-L2 {err_grad:.2e} "
          f"({ref['bound_grad_rel']:.2e}) max|err| {err_abs:.2e} ({ref['bound_grad_abs']:.2e})")
    assert smap.shape == ref["map"].shape and bool(torch.isfinite(d_x).all())
    assert err_map <= ref["bound_map"] and err_per <= ref["bound_per_image"] and err_mean <= ref["bound_mean"]
    assert err_grad <= ref["bound_grad_rel"]
    assert err_abs <= ref["bound_grad_abs"]
    # not vacuous
    assert 0.05 < float(mean) < 0.98
    if case[0] == "noise":
        assert float((d_x.abs() > 0).float().mean()) > 0.5
    if case[0] == "white_background":
        # float32 window sums would cancel here: a gradient that is an exact 0, reached from terms of about 2000
        only = R.white_only_pixels(ref["x"], ref["y"])
        worst = float(d_x[only].abs().max())
        print(f"{case}: {int(only.sum())} surround-only elements, max |gradient| {worst:.2e}")
        assert only.any() and worst <= ref["bound_grad_abs"]


def test_identical_images():
    case = ("white_background", 3, 48, 40, 3)
    ref = R.reference(case)
    y = ref["y"].to(DEV)
    mean, per, smap, d_x = _call(y, y)
    m32 = R.ssim32_torch(ref["y"], ref["y"])[0]
    bound = max(4.0 * abs(float(m32) - 1.0), 1e-6)
    print(f"x is y: mean - 1 = {float(mean) - 1:.2e} (bound {bound:.2e}), max |gradient| {float(d_x.abs().max()):.2e} "
          f"(bound {ref['bound_grad_abs']:.2e})")
    assert abs(float(mean) - 1.0) <= bound and float((per - 1).abs().max()) <= bound and float((smap - 1).abs().max()) <= bound
    assert float(d_x.abs().max()) <= ref["bound_grad_abs"]


# ---- 2: semantics of the call ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base():
    ref = R.reference(("noise", 1, 27, 43, 3))
    x, y = ref["x"].to(DEV), ref["y"].to(DEV)
    mean, per, smap, d_x = _call(x, y)
    return dict(x=x, y=y, mean=mean, per=per, map=smap, d_x=d_x)


def test_two_runs_give_the_same_bits(base):
    for case in (("noise", 1, 27, 43, 3), ("white_background", 3, 48, 40, 3)):
        ref = R.reference(case)
        x, y = ref["x"].to(DEV), ref["y"].to(DEV)
        a, b = _call(x, y), _call(x, y)
        for s, t in zip(a, b):
            assert torch.equal(s, t)


def test_accumulate_adds_to_the_buffer(base):
    pre = torch.rand(base["x"].shape, generator=torch.Generator().manual_seed(4)).mul_(2e-3).sub_(1e-3).to(DEV)
    out = pre.clone()
    _call(base["x"], base["y"], out=out, accumulate=True)
    want = pre.double() + base["d_x"].double()
    ulp = 2.0 ** -23 * torch.maximum(pre.abs(), base["d_x"].abs()).double()      # the rounding of that one addition
    assert bool(((out.double() - want).abs() <= ulp).all()) and not torch.equal(out, pre)
    over = torch.full_like(pre, 7.0)
    _call(base["x"], base["y"], out=over)
    assert torch.equal(over, base["d_x"])                                       # without it every element is overwritten


def test_grad_scale_scales_the_gradient_only(base):
    for scale in (4.0, 0.25):
        mean, per, smap, d_x = _call(base["x"], base["y"], grad_scale=scale)
        assert torch.equal(d_x, base["d_x"] * scale)
        assert torch.equal(mean, base["mean"]) and torch.equal(per, base["per"]) and torch.equal(smap, base["map"])


def test_null_outputs(base):
    x, y = base["x"], base["y"]
    mean, per, smap, d_x = _call(x, y, want_mean=False)
    assert mean is None and torch.equal(per, base["per"]) and torch.equal(smap, base["map"]) and torch.equal(d_x, base["d_x"])
    mean, per, smap, d_x = _call(x, y, want_per_image=False)
    assert per is None and torch.equal(mean, base["mean"]) and torch.equal(smap, base["map"]) and torch.equal(d_x, base["d_x"])
    mean, per, smap, d_x = _call(x, y, want_map=False)
    assert smap is None and torch.equal(mean, base["mean"]) and torch.equal(per, base["per"]) and torch.equal(d_x, base["d_x"])
    mean, per, smap, d_x = _call(x, y, grad=False)
    assert d_x is None and torch.equal(mean, base["mean"]) and torch.equal(per, base["per"]) and torch.equal(smap, base["map"])
    mean, per, smap, d_x = _call(x, y, want_mean=False, want_per_image=False, want_map=False)
    assert torch.equal(d_x, base["d_x"])
    assert ops.ssim_fwd_bwd(x, y, want_mean=False, want_per_image=False) == (None, None, None)


def test_wrapper_checks_its_tensors(base):
    x, y = base["x"], base["y"]
    for bad in ((x[:, :10], y[:, :10]), (x, y[:, :-1]), (x.double(), y.double()), (x.permute(0, 2, 1, 3), y.permute(0, 2, 1, 3)),
                (x.repeat(1, 1, 1, 2), y.repeat(1, 1, 1, 2)), (x[0], y[0])):
        with pytest.raises(ops.VoxeError):
            ops.ssim(*bad)
    with pytest.raises(ops.VoxeError):
        ops.ssim(x, y, data_range=0.0)
    with pytest.raises(ops.VoxeError):
        ops.ssim(x, y.clone().requires_grad_(True))


def test_data_range(base):
    mean255, _ = ops.ssim(base["x"] * 255.0, base["y"] * 255.0, data_range=255.0)
    assert abs(float(mean255) - float(base["mean"])) < 1e-5


def test_metric_helper_takes_either_layout(base):
    from thre3d_atom.utils import metric_utils

    x, y = base["x"][0], base["y"][0]
    assert metric_utils.ssim(x, y) == float(base["mean"])
    assert metric_utils.ssim(x.permute(2, 0, 1), y.permute(2, 0, 1)) == float(base["mean"])


# ---- 3: the autograd op behind a render ------------------------------------------------------------------------------------
def _scene(views=10, side=48):
    """the synthetic views of tests/test_trainers_gpu.py: a textured ball on white, `views` cameras around it"""
    from test_trainers_gpu import _sphere_model
    from thre3d_atom.utils.imaging_utils import CameraIntrinsics, pose_spherical

    truth = _sphere_model(side=24, samples=96)
    intr = CameraIntrinsics(side, side, 0.5 * side / np.tan(0.5 * 0.6911112))
    poses, images = [], []
    for i in range(views):
        pose = pose_spherical(360.0 * i / views, 20.0 + 50.0 * ((i * 0.618) % 1.0), 4.0311)
        poses.append(torch.cat([pose.rotation, pose.translation], dim=1))
        images.append(truth.render(pose, intr, perturb_sampled_points=False).colour.permute(2, 0, 1))
    return truth, intr, torch.stack(poses).to(DEV), torch.stack(images).to(DEV).contiguous()


@pytest.fixture(scope="module")
def scene():
    return _scene()


def _random_model(seed=3, samples=96, perturb=True):
    from thre3d_atom.modules.volumetric_model import VolumetricModel
    from thre3d_atom.thre3d_reprs.renderers import SHVoxGridRenderConfig, render_sh_voxel_grid
    from thre3d_atom.thre3d_reprs.voxels import VoxelGrid, VoxelSize
    from thre3d_atom.utils.imaging_utils import CameraBounds

    g = torch.Generator().manual_seed(seed)
    vg = VoxelGrid(torch.empty(24, 24, 24, 1).uniform_(-1, 1, generator=g), torch.empty(24, 24, 24, 3).uniform_(-1, 1, generator=g),
                   VoxelSize(0.125, 0.125, 0.125), density_preactivation=torch.nn.Identity(),
                   density_postactivation=torch.nn.Softplus(), expected_density_scale=100.0 / 3.0, tunable=True)
    return VolumetricModel(vg, render_sh_voxel_grid, SHVoxGridRenderConfig(samples, CameraBounds(1.8, 6.6), white_bkgd=True,
                                                                          render_num_samples_per_ray=96,
                                                                          perturb_sampled_points=perturb), device=DEV)


def test_gradient_reaches_the_grid_through_a_render(scene):
    """(1 - ssim).backward() through render_rays of 4 patches of 16 x 16: the render's backward is the same whichever SSIM made
    its incoming gradient, so the grid's gradients compare the hand-over of ops.ssim with the float32 torch restatement's"""
    from thre3d_atom.rendering.volumetric.render_interface import Rays
    from thre3d_atom.rendering.volumetric.utils.misc import _cast_and_gather, patch_flat_indices

    truth, intr, poses, images = scene
    n, P = 4, 16
    # patches over the ball (the centre of the 48 x 48 views), one camera each
    flat = patch_flat_indices(torch.tensor([0, 3, 5, 8], device=DEV), torch.tensor([16, 12, 18, 14], device=DEV),
                              torch.tensor([16, 18, 13, 20], device=DEV), P, intr.height, intr.width)
    rays, pixels = _cast_and_gather(intr, poses, images, flat, None, False, None)
    target = pixels.contiguous().view(n, P, P, 3)
    grads = {}
    for which in ("kernel", "torch"):
        vm = _random_model()
        colour = vm.render_rays(Rays(rays.origins, rays.directions), perturb_sampled_points=False).colour.view(n, P, P, 3)
        value = ops.ssim(colour, target)[0] if which == "kernel" else R.ssim32_torch(colour, target)[0]
        (1.0 - value).backward()
        grid = vm.thre3d_repr
        assert grid.densities.grad is not None and grid.features.grad is not None
        grads[which] = (float(value.detach()), grid.densities.grad.clone(), grid.features.grad.clone())
    err_d, err_f = R.rel_l2(grads["kernel"][1], grads["torch"][1]), R.rel_l2(grads["kernel"][2], grads["torch"][2])
    print(f"ssim {grads['kernel'][0]:.5f} (torch {grads['torch'][0]:.5f}); grid gradients, ops.ssim vs torch: rel-L2 densities "
          f"{err_d:.2e} features {err_f:.2e}")
    assert float(grads["kernel"][1].abs().max()) > 0 and float(grads["kernel"][2].abs().max()) > 0
    assert 0.0 < grads["kernel"][0] < 0.9 and abs(grads["kernel"][0] - grads["torch"][0]) < 1e-5
    assert err_d <= 1e-4 and err_f <= 1e-4


def test_autograd_op_scales_and_skips(base):
    x = base["x"].clone().requires_grad_(True)
    mean, per = ops.ssim(x, base["y"])
    assert torch.equal(mean.detach(), base["mean"]) and torch.equal(per, base["per"]) and not per.requires_grad
    (3.0 * mean).backward()
    assert torch.equal(x.grad, base["d_x"] * 3.0)
    with torch.no_grad():
        mean, _ = ops.ssim(base["x"], base["y"])
    assert not mean.requires_grad and torch.equal(mean, base["mean"])


# ---- 4: the patch sampler --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", (False, True), ids=("hwf", "lens"))
def test_patch_sampler_equals_a_full_image_cast_and_gather(scene, lens):
    from thre3d_atom.rendering.volumetric.utils import misc
    from thre3d_atom.utils.imaging_utils import CameraPose, PinholeCamera

    _, intr, poses, images = scene
    if lens:
        intr = PinholeCamera(intr.height, intr.width, intr.focal, 0.97 * intr.focal, 23.1, 25.2, (0.08, -0.03, 0.002, -0.001, 0.01))
    K, n, P = 4, 6, 13
    picks = [7, 2, 9, 4]
    torch.manual_seed(11)
    rays, pixels = misc.sample_random_patches_and_pixels_from_cameras(intr, poses[picks], images, n, P, image_ids=picks)
    assert rays.origins.shape == (n * P * P, 3) and pixels.shape == (n * P * P, 3)
    torch.manual_seed(11)   # the sampler's three draws, in its order
    cams = torch.randint(0, K, (n,), device=DEV)
    top = torch.randint(0, intr.height - P + 1, (n,), device=DEV)
    left = torch.randint(0, intr.width - P + 1, (n,), device=DEV)
    full = [misc.cast_rays(intr, CameraPose(rotation=poses[i][:, :3], translation=poses[i][:, 3:]), DEV) for i in picks]
    for p in range(n):
        c, t, l = int(cams[p]), int(top[p]), int(left[p])
        block = slice(p * P * P, (p + 1) * P * P)
        assert torch.equal(rays.origins[block].view(P, P, 3), full[c].origins[t:t + P, l:l + P])
        assert torch.equal(rays.directions[block].view(P, P, 3), full[c].directions[t:t + P, l:l + P])
        assert torch.equal(pixels[block].view(P, P, 3), images[picks[c]].permute(1, 2, 0)[t:t + P, l:l + P])


# ---- 5: the held-out tester ---------------------------------------------------------------------------------------------
def test_tester_reports_ssim(scene, monkeypatch):
    from thre3d_atom.data.datasets import InMemoryPosedImages
    from thre3d_atom.modules import testers
    from thre3d_atom.utils.imaging_utils import CameraBounds, CameraPose

    _, intr, poses, _ = scene
    # (unjittered samples: two evaluations of one model render the same bits)
    truth, other = _random_model(perturb=False), _random_model(seed=3, perturb=False)
    with torch.no_grad():
        truth.thre3d_repr.densities.copy_(scene[0].thre3d_repr.densities)
        truth.thre3d_repr.features.copy_(scene[0].thre3d_repr.features)

    def views(model):   # what the tester renders of `model`
        cfg = model.render_config
        return torch.stack([model.render(CameraPose(rotation=p[:, :3], translation=p[:, 3:]), intr, gpu_render=True,
                                         optimized_sampling=True, num_samples_per_ray=cfg.render_num_samples_per_ray
                                         ).colour.detach().permute(2, 0, 1).cpu() for p in poses[:3]])

    own = InMemoryPosedImages(views(truth), poses[:3].cpu(), intr, CameraBounds(1.8, 6.6))
    same = testers.test_sh_vox_grid_vol_mod_with_posed_images(truth, own)
    with torch.no_grad():   # the truth, perturbed: noisier colours and a softer surface
        other.thre3d_repr.features.copy_(truth.thre3d_repr.features + 1.0 * other.thre3d_repr.features)
        other.thre3d_repr.densities.copy_(truth.thre3d_repr.densities + 0.3 * other.thre3d_repr.densities)
    worse = testers.test_sh_vox_grid_vol_mod_with_posed_images(other, own)
    print(f"tester: own views {same}, perturbed model {worse}")
    assert same["ssim"] > 0.99 and "lpips" not in same
    assert 0.0 < worse["ssim"] < same["ssim"] - 0.02
    monkeypatch.setattr(testers, "ssim", lambda a, b: 0.25)
    stubbed = testers.test_sh_vox_grid_vol_mod_with_posed_images(other, own)
    assert stubbed["psnr"] == worse["psnr"] and stubbed["ssim"] == 0.25


# ---- 6: the trainer ----------------------------------------------------------------------------------------------------------
class _Capture(logging.Handler):
    def __init__(self):
        super().__init__()
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def _train(scene, out, weight, fused=True, iterations=3, model=None, **kw):
    from thre3d_atom.data.datasets import InMemoryPosedImages
    from thre3d_atom.modules.trainers import train_sh_vox_grid_vol_mod_with_posed_images
    from thre3d_atom.utils.imaging_utils import CameraBounds
    from thre3d_atom.utils.logging import log

    _, intr, poses, images = scene
    data = InMemoryPosedImages(images[:8].cpu(), poses[:8].cpu(), intr, CameraBounds(1.8, 6.6))
    torch.manual_seed(5)
    vm = _random_model(seed=3) if model is None else model
    cap = _Capture()
    log.addHandler(cap)
    try:
        # (the initializer is the identity: every run starts from the same grid)
        train_sh_vox_grid_vol_mod_with_posed_images(vm, data, out, random_initializer=lambda t: t, ray_batch_size=4096, num_stages=1,
                                                    num_iterations_per_stage=iterations, summary_freq=1, fast_debug_mode=True,
                                                    fused_grid_step=fused, ssim_weight=weight, **kw)
    finally:
        log.removeHandler(cap)
    return vm, cap.lines


def test_trainer_with_the_ssim_term_on_both_optimiser_paths(scene, tmp_path):
    """three iterations at ssim_weight 0.2 under FusedGridAdam and under VoxeAdam end on the same densities; the bound is the one the
    distortion term's test of the two paths has (rel-L2 1e-4); measured 0.8e-6 to 1.0e-6"""
    base, lines0 = _train(scene, tmp_path / "w0", 0.0)
    assert not any("ssim" in line for line in lines0)
    finals = {}
    for fused in (True, False):
        vm, lines = _train(scene, tmp_path / f"w1_{int(fused)}", 0.2, fused)
        values = [float(m.group(1)) for m in (re.search(r"ssim:\s*([-+0-9.eE]+|nan|inf)", line) for line in lines) if m]
        print(f"fused_grid_step {fused}: ssim {values}")
        assert len(values) == 3 and all(np.isfinite(v) and -1.0 < v < 1.0 for v in values)
        dens = vm.thre3d_repr.densities.detach()
        assert not torch.equal(dens, base.thre3d_repr.densities.detach()) and bool(torch.isfinite(dens).all())
        if fused:
            assert sum("no one-call iteration" in line for line in lines) == 1
        finals[fused] = dens.clone()
    err = R.rel_l2(finals[True], finals[False])
    print(f"final densities, FusedGridAdam vs VoxeAdam: rel_l2 {err:.3e}")
    assert err < 1e-4   # (the bound of the distortion term's test of the two paths)


def test_training_with_the_term_lowers_one_minus_ssim_of_a_held_out_view(scene, tmp_path):
    """measured: 1 - ssim of the held-out view 0.2047 -> 0.1398"""
    from thre3d_atom.utils import metric_utils
    from thre3d_atom.utils.imaging_utils import CameraPose

    _, intr, poses, images = scene
    held = 9   # (the trainer sees views 0..7)
    pose = CameraPose(rotation=poses[held][:, :3], translation=poses[held][:, 3:])

    def one_minus_ssim(vm):
        with torch.no_grad():
            return 1.0 - metric_utils.ssim(vm.render(pose, intr, perturb_sampled_points=False).colour, images[held].permute(1, 2, 0))

    # the fixture: the scene's own grid with noise on its colours and its surface (what the tester test calls the perturbed model);
    # a random grid is no use here, 30 iterations into a fit from noise its held-out views are fog
    vm = _random_model(seed=3)
    with torch.no_grad():
        vm.thre3d_repr.features.copy_(scene[0].thre3d_repr.features + 3.0 * vm.thre3d_repr.features)
        vm.thre3d_repr.densities.copy_(scene[0].thre3d_repr.densities + 0.5 * vm.thre3d_repr.densities)
    start = one_minus_ssim(vm)
    vm, lines = _train(scene, tmp_path / "descent", 0.2, iterations=30, ssim_patch_size=16, model=vm)
    end = one_minus_ssim(vm)
    print(f"held-out view, 1 - ssim: {start:.4f} -> {end:.4f} after 30 iterations at ssim_weight 0.2")
    assert end < start
