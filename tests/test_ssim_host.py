"""SSIM, the part that needs no device: the float64 restatement tests/ssim_ref.py checked against itself, the teeth
of the GPU test's bounds, the C ABI's symbols and argument validation, the patch sampler's index arithmetic, the options and the
trainer's two code paths."""
import ctypes
import importlib.util
import inspect
import os
import re

import pytest
import torch

import ssim_ref as R
from conftest import ROOT
from voxe_hip import abi

CPU = torch.device("cpu")


# ---- the restatement itself ------------------------------------------------------------------------------------------------
def test_identical_images_give_one_and_the_measure_is_symmetric():
    x, y = (t.double() for t in R.noise(1, 2, 20, 17, 3))
    mean, per, smap = R.ssim64(x, x)
    assert float((smap - 1).abs().max()) < 1e-12 and abs(float(mean) - 1) < 1e-12 and per.shape == (2,)
    assert smap.shape == (2, 10, 7, 3)                       # valid windows only
    a, b = R.ssim64(x, y), R.ssim64(y, x)
    assert float((a[2] - b[2]).abs().max()) < 1e-14 and 0.05 < float(a[0]) < 0.98


def test_constant_images_have_the_closed_form():
    C1, _ = R.constants(1.0)
    for a, b in ((0.2, 0.7), (1.0, 1.0), (0.0, 0.5)):
        x, y = torch.full((1, 13, 12, 2), a, dtype=torch.float64), torch.full((1, 13, 12, 2), b, dtype=torch.float64)
        # (the float-rounded window sums to 1 - 1.3e-8, not to 1: the closed form holds with the window's own sum s)
        s = float(R.gaussian().sum()) ** 2
        ma, mb = a * s, b * s
        va, vb, vab = a * a * s - ma * ma, b * b * s - mb * mb, a * b * s - ma * mb
        _, C2 = R.constants(1.0)
        want = (2 * ma * mb + C1) * (2 * vab + C2) / ((ma * ma + mb * mb + C1) * (va + vb + C2))
        got = R.ssim64(x, y)[2]
        assert float((got - want).abs().max()) < 1e-12
        assert abs(want - (2 * a * b + C1) / (a * a + b * b + C1)) < 1e-5   # the textbook form, up to the window's rounding


def test_data_range_scales_the_constants():
    x, y = (t.double() for t in R.noise(3, 1, 14, 14, 1))
    assert abs(float(R.ssim64(255 * x, 255 * y, data_range=255.0)[0]) - float(R.ssim64(x, y)[0])) < 1e-12


def test_agrees_with_skimage():
    metrics = pytest.importorskip("skimage.metrics")
    x, y = R.noise(5, 1, 24, 31, 3)
    want = metrics.structural_similarity(x[0].double().numpy(), y[0].double().numpy(), gaussian_weights=True, sigma=1.5,
                                         use_sample_covariance=False, data_range=1, channel_axis=-1)
    # (skimage keeps its window in double; the contract rounds it to float, which moves the mean by ~1e-8)
    assert abs(float(R.ssim64(x.double(), y.double(), rounded_window=False)[0]) - want) < 1e-12
    assert abs(float(R.ssim64(x.double(), y.double())[0]) - want) < 1e-6


def test_closed_form_gradient_is_autograd_and_finite_differences():
    for case in (("noise", 2, 15, 13, 3), ("white_background", 1, 26, 26, 3), ("rendered", 1, 12, 27, 4)):
        x, y = R.make(case)
        grad = R.ssim64_grad(x, y)
        P, Q, Rm, closed = R.closed_form64(x, y)
        assert float((closed - grad).abs().max()) < 1e-12, case
        assert P.shape == Q.shape == Rm.shape == R.ssim64(x.double(), y.double())[2].shape
    x, y = (t.double() for t in R.noise(9, 1, 13, 14, 2))
    grad = R.ssim64_grad(x, y)
    for at in ((0, 6, 7, 1), (0, 0, 0, 0), (0, 12, 13, 1)):
        h = 1e-6
        xp, xm = x.clone(), x.clone()
        xp[at] += h
        xm[at] -= h
        fd = (float(R.ssim64(xp, y)[0]) - float(R.ssim64(xm, y)[0])) / (2 * h)
        assert abs(fd - float(grad[at])) < 1e-8 * max(1.0, abs(fd)), (at, fd, float(grad[at]))


def test_fixtures_are_what_the_gpu_test_needs():
    seen = set()
    for case in R.CASES:
        name, N, H, W, C = case
        ref = R.reference(case)
        seen.add(name)
        assert ref["x"].shape == (N, H, W, C) and ref["x"].dtype == torch.float32 and ref["x"].is_contiguous()
        assert 0.0 <= float(ref["x"].min()) and float(ref["x"].max()) <= 1.0
        assert 0.05 < float(ref["mean"]) < 0.98, case
        if name == "noise":
            assert float((ref["grad"].abs() > 0).float().mean()) > 0.5
        if name == "white_background":
            assert float(R.white_only_windows(ref["x"], ref["y"]).float().mean()) >= 0.5, case
            only = R.white_only_pixels(ref["x"], ref["y"])
            assert only.any() and float(ref["grad"][only].abs().max()) <= ref["bound_grad_abs"]
    assert seen == {"noise", "white_background", "rendered"}
    assert {c[1] for c in R.CASES} == {1, 3} and {c[4] for c in R.CASES} == {1, 3, 4}
    for ragged in ((12, 27), (27, 43)):
        assert {c[4] for c in R.CASES if c[2:4] == ragged} == {1, 3, 4}


def test_the_bounds_have_teeth(capsys):
    """a restatement with zero-padded windows, with sigma = 1.0 or without the Q term misses the GPU test's bounds on the GPU
    test's own cases (the factor by which it misses is printed)"""
    worst = {"pad": 1e30, "sigma": 1e30, "drop_q": 1e30}
    for case in R.CASES:
        ref = R.reference(case)
        x, y = ref["x"].double(), ref["y"].double()
        pad = abs(float(R.ssim64(x, y, pad=True)[0]) - float(ref["mean"])) / ref["bound_mean"]
        sigma = float((R.ssim64(x, y, sigma=1.0)[2] - ref["map"]).abs().max()) / ref["bound_map"]
        drop_q = R.rel_l2(R.closed_form64(x, y, drop_q=True)[3], ref["grad"]) / ref["bound_grad_rel"]
        with capsys.disabled():
            print(f"\n{case}: misses its bound by a factor of  zero padding (mean) {pad:.3g}  sigma 1.0 (map) {sigma:.3g}  "
                  f"no Q term (gradient rel-L2) {drop_q:.3g}", end="")
        worst = {k: min(worst[k], v) for k, v in (("pad", pad), ("sigma", sigma), ("drop_q", drop_q))}
    assert min(worst.values()) > 10.0, worst


def test_the_float32_yardstick_is_a_restatement_too():
    for case in R.CASES[:4]:
        ref = R.reference(case)
        mean, per, smap = R.ssim32_torch(ref["x"], ref["y"])
        assert smap.dtype == torch.float32 and float((smap.double() - ref["map"]).abs().max()) < 1e-3
        assert R.rel_l2(R.ssim32_torch_grad(ref["x"], ref["y"]), ref["grad"]) < 1e-3


# ---- symbols and validation -------------------------------------------------------------------------------------------------
def _library():
    from voxe_hip import build

    return abi.declare(ctypes.CDLL(build.build()), "voxe_")


def test_symbols_are_declared_and_have_no_cpu_twin():
    header = open(os.path.join(ROOT, "include", "voxe.h")).read()
    for name in ("voxe_ssim_fwd_bwd", "voxe_ssim_scratch_bytes"):
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in abi.hip_symbols()
        assert hasattr(_library(), name)
    assert "voxe_cpu_ssim" not in header and not [s for s in abi.cpu_symbols() if "ssim" in s]
    assert abi.ABI_VERSION == 13 and re.search(r"#define VOXE_ABI_VERSION 13\b", header)
    assert _library().voxe_abi_version() == 13


def test_argument_validation_needs_no_device():
    L = _library()
    ok = dict(x=8, y=8, N=2, H=16, W=12, C=3, data_range=1.0, scratch=8)
    big = 1 << 24

    def call(scratch_bytes=big, d_x=8, **kw):
        a = {**ok, **kw}
        return L.voxe_ssim_fwd_bwd(a["x"], a["y"], a["N"], a["H"], a["W"], a["C"], a["data_range"], 1.0, 8, 8, None, d_x, 0,
                                   a["scratch"], scratch_bytes, None)

    assert call(x=None) == abi.ERR_NULL_POINTER and call(y=None) == abi.ERR_NULL_POINTER
    assert call(scratch=None) == abi.ERR_NULL_POINTER
    for bad in (dict(H=10), dict(W=10), dict(C=5), dict(C=0), dict(N=0), dict(data_range=0.0), dict(data_range=-1.0)):
        assert call(**bad) == abi.ERR_BAD_SHAPE, bad
    with_grad, without = L.voxe_ssim_scratch_bytes(2, 16, 12, 3, 1), L.voxe_ssim_scratch_bytes(2, 16, 12, 3, 0)
    assert with_grad >= without + 3 * 4 * 2 * 3 * 6 * 2 and without >= 8 * 2 * 3   # three float maps; a double per block
    assert call(scratch_bytes=with_grad - 1) == abi.ERR_WORKSPACE
    assert call(scratch_bytes=without, d_x=8) == abi.ERR_WORKSPACE
    assert call(scratch_bytes=without - 1, d_x=None) == abi.ERR_WORKSPACE
    assert L.voxe_ssim_scratch_bytes(2, 10, 12, 3, 1) == 0 and L.voxe_ssim_scratch_bytes(2, 16, 12, 5, 1) == 0
    # every output NULL: nothing to do, and nothing is launched
    assert L.voxe_ssim_fwd_bwd(8, 8, 2, 16, 12, 3, 1.0, 1.0, None, None, None, None, 0, 8, big, None) == abi.OK


def test_python_wrapper_refuses_what_the_kernel_cannot_take():
    from voxe_hip import ops

    x = torch.rand(1, 16, 16, 3)
    with pytest.raises(ops.VoxeError):
        ops.ssim(x, x.clone())                                     # not on a GPU: there is no fall-back
    from thre3d_atom.utils import metric_utils

    with pytest.raises(ValueError):
        metric_utils.ssim(torch.rand(16, 16, 3), torch.rand(16, 15, 3))


# ---- patch sampler: index arithmetic ---------------------------------------------------------------------------------------
def test_patch_indices_are_patch_major_row_column_and_inside_the_image():
    from thre3d_atom.rendering.volumetric.utils.misc import patch_flat_indices

    H, W, P = 14, 19, 11
    cameras, top, left = torch.tensor([2, 0, 1]), torch.tensor([3, 0, 1]), torch.tensor([8, 0, 5])
    flat = patch_flat_indices(cameras, top, left, P, H, W)
    assert flat.shape == (3 * P * P,) and flat.dtype == torch.long
    cam, rem = flat // (H * W), flat % (H * W)
    row, col = (rem // W).view(3, P, P), (rem % W).view(3, P, P)
    for i in range(3):
        assert (cam.view(3, P, P)[i] == cameras[i]).all()
        assert (row[i] == (top[i] + torch.arange(P))[:, None]).all() and (col[i] == (left[i] + torch.arange(P))[None, :]).all()
    assert int(row.max()) == H - 1 and int(col.max()) == W - 1 and int(row.min()) == 0 and int(col.min()) == 0


def test_patch_sampler_draws_every_corner_and_camera(monkeypatch):
    from thre3d_atom.rendering.volumetric.utils import misc
    from thre3d_atom.utils.imaging_utils import CameraIntrinsics

    H, W, P, K = 14, 16, 11, 3
    seen = {}

    def capture(intr, poses, images, flat_index, image_ids, differentiable, intrinsics):
        seen["flat"], seen["args"] = flat_index, (image_ids, differentiable, intrinsics)
        return None, None

    monkeypatch.setattr(misc, "_cast_and_gather", capture)
    torch.manual_seed(0)
    misc.sample_random_patches_and_pixels_from_cameras(CameraIntrinsics(H, W, 20.0), torch.zeros(K, 3, 4), torch.zeros(5, 3, H, W),
                                                       2000, P, image_ids=[4, 0, 2], differentiable=True)
    flat = seen["flat"].view(2000, P, P)
    assert seen["args"] == ([4, 0, 2], True, None)
    first = flat[:, 0, 0]
    cam, rem = first // (H * W), first % (H * W)
    assert sorted(set(cam.tolist())) == list(range(K))
    assert sorted(set((rem // W).tolist())) == list(range(H - P + 1))     # the whole range [0, H - P]
    assert sorted(set((rem % W).tolist())) == list(range(W - P + 1))
    last = flat[:, -1, -1] % (H * W)
    assert int((last // W).max()) == H - 1 and int((last % W).max()) == W - 1   # every patch lies inside its image
    assert (flat[:, 0, 1] == first + 1).all() and (flat[:, 1, 0] == first + W).all()
    with pytest.raises(ValueError):
        misc.sample_random_patches_and_pixels_from_cameras(CameraIntrinsics(H, W, 20.0), torch.zeros(K, 3, 4),
                                                           torch.zeros(5, 3, H, W), 4, 15)


# ---- options, documents, trainer --------------------------------------------------------------------------------------------
def test_cli_options_trainer_arguments_and_documents():
    spec = importlib.util.spec_from_file_location("train_ssim_cli", os.path.join(ROOT, "train_sh_based_voxel_grid_with_posed_images.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    options = {p.name: p for p in mod.main.params}
    assert options["ssim_weight"].default == 0.0 and "--ssim_weight" in options["ssim_weight"].opts
    assert options["ssim_patch_size"].default == 32 and "--ssim_patch_size" in options["ssim_patch_size"].opts
    from thre3d_atom.modules import trainers

    sig = inspect.signature(trainers.train_sh_vox_grid_vol_mod_with_posed_images)
    assert sig.parameters["ssim_weight"].default == 0.0 and sig.parameters["ssim_patch_size"].default == 32
    for doc in ("README.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "--ssim_weight" in text and "--ssim_patch_size" in text, doc
    assert "### 4.18" in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "ssim_bench.py" in open(os.path.join(ROOT, "tools", "README.md")).read()


def test_weight_zero_leaves_the_one_call_iteration(tmp_path, monkeypatch):
    """ssim_weight = 0 takes the trainer's code path as it was: the one-call iteration runs and neither the patch sampler nor
    ops.ssim is called; above 0 it is the other way round, with floor(ray_batch_size / P^2) patches of min(P, H, W) a side"""
    from thre3d_atom.modules import trainers
    from thre3d_atom.modules.volumetric_model import VolumetricModel
    from thre3d_atom.thre3d_reprs.renderers import SHVoxGridRenderConfig, render_sh_voxel_grid
    from thre3d_atom.thre3d_reprs.voxels import VoxelGrid, VoxelSize
    from thre3d_atom.utils.imaging_utils import CameraBounds, CameraIntrinsics

    calls = {"one_call": 0, "ssim": 0, "render": 0, "patches": 0, "pixels": 0}
    side = 16

    class FakeOpt(torch.optim.Optimizer):
        def __init__(self, grid, lr, betas):
            super().__init__(list(grid.parameters()), dict(lr=lr))

        def reconstruction_step(self, *a, **k):
            calls["one_call"] += 1

        def reconstruction_prefetch(self, *a, **k):
            pass

        def detach(self):
            pass

        def step(self, closure=None):
            pass

    class Data:
        def __init__(self):
            self.images = torch.rand(4, 3, side, side)
            self.poses = torch.eye(4)[None, :3].repeat(4, 1, 1)
            self.camera_intrinsics = CameraIntrinsics(side, side, 10.0)
            self.camera_bounds = CameraBounds(1.0, 4.0)

        def downsampled(self, f):
            return self

        def to(self, device):
            return self

        def __len__(self):
            return 4

        def get_hemispherical_radius_estimate(self):
            return 4.0

    def fake_render_rays(self, rays, **kw):
        calls["render"] += 1
        return type("Out", (), {"colour": self.thre3d_repr.features.sum() * 0 + torch.zeros(rays.origins.shape[0], 3)})()

    def fake_ssim(x, y, data_range=1.0):
        calls["ssim"] += 1
        assert x.shape == y.shape == (2, side, side, 3)            # 600 // 16^2 patches of min(32, 16, 16)
        return x.sum() * 0 + 0.5, torch.full((x.shape[0],), 0.5)

    def fake_patches(intr, poses, images, num_patches, patch_size, **k):
        calls["patches"] += 1
        n = num_patches * patch_size * patch_size
        return type("R", (), {"origins": torch.zeros(n, 3)})(), torch.zeros(n, 3)

    def fake_pixels(intr, poses, images, n, **k):
        calls["pixels"] += 1
        return type("R", (), {"origins": torch.zeros(16, 3)})(), torch.zeros(16, 3)

    monkeypatch.setattr(trainers, "FusedGridAdam", FakeOpt)
    monkeypatch.setattr(trainers, "scale_voxel_grid_with_required_output_size", lambda grid, size: grid)
    monkeypatch.setattr(trainers, "_render_params", lambda *a, **k: None)
    monkeypatch.setattr(trainers, "_next_rng", lambda: (0, 0))
    monkeypatch.setattr(VolumetricModel, "render_rays", fake_render_rays)
    monkeypatch.setattr(trainers._ops, "ssim", fake_ssim)
    monkeypatch.setattr(trainers, "sample_random_patches_and_pixels_from_cameras", fake_patches)
    monkeypatch.setattr(trainers, "sample_random_rays_and_pixels_from_cameras", fake_pixels)
    for weight, want in ((0.0, {"one_call": 3, "ssim": 0, "render": 0, "patches": 0, "pixels": 0}),
                         (0.2, {"one_call": 0, "ssim": 3, "render": 6, "patches": 3, "pixels": 0})):
        for k in calls:
            calls[k] = 0
        vg = VoxelGrid(torch.zeros(4, 4, 4, 1), torch.zeros(4, 4, 4, 3), VoxelSize(0.1, 0.1, 0.1), tunable=True)
        vm = VolumetricModel(vg, render_sh_voxel_grid, SHVoxGridRenderConfig(8, CameraBounds(1.0, 4.0)), device=CPU)
        trainers.train_sh_vox_grid_vol_mod_with_posed_images(vm, Data(), tmp_path, num_stages=1, num_iterations_per_stage=3,
                                                             fast_debug_mode=True, ssim_weight=weight, ray_batch_size=600)
        assert calls == want, (weight, calls)
    # a stage whose images are smaller than the window keeps the random pixel set and has no SSIM term
    side = 8
    for k in calls:
        calls[k] = 0
    vg = VoxelGrid(torch.zeros(4, 4, 4, 1), torch.zeros(4, 4, 4, 3), VoxelSize(0.1, 0.1, 0.1), tunable=True)
    vm = VolumetricModel(vg, render_sh_voxel_grid, SHVoxGridRenderConfig(8, CameraBounds(1.0, 4.0)), device=CPU)
    trainers.train_sh_vox_grid_vol_mod_with_posed_images(vm, Data(), tmp_path, num_stages=1, num_iterations_per_stage=2,
                                                         fast_debug_mode=True, ssim_weight=0.2, ray_batch_size=600)
    assert calls == {"one_call": 0, "ssim": 0, "render": 4, "patches": 0, "pixels": 2}, calls
