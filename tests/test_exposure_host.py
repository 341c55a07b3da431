"""CPU checks of the per-image exposure compensation: the float64 restatement tests/exposure_ref.py against
central differences, the C ABI's declarations and argument validation (no device work), the shared inputs of
tests/test_exposure_gpu.py (the L1 residuals that are too close to 0 for a float32 sign stay under the cap the GPU test
asserts), the samplers' `return_image_ids`, the trainer's options, the host-side solve, and the documents."""
import ctypes
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest
import torch

import exposure_ref as ER
from conftest import ROOT
from voxe_hip import abi, ops

CPU = torch.device("cpu")


# ---- the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ER.KINDS)
@pytest.mark.parametrize("weighted", (False, True))
def test_reference_gradients_equal_central_differences(kind, weighted):
    R, N = 37, 3
    x, y, ids, delta, w = ER.inputs(R, N, "shuffle", weighted, seed=1)
    x, y, delta = x.astype(np.float64), y.astype(np.float64), delta.astype(np.float64)
    ref = ER.fwd_bwd(x, y, ids, delta, kind, w, grad_scale=0.7)
    assert not ref["flip"].any()       # (no residual at a kink of |.|: the differences below see a smooth function)
    h = 1e-6

    def loss(x_, d_):
        return ER.fwd_bwd(x_, y, ids, d_, kind, w)["loss"][0]

    for which, arr, got in (("x", x, ref["d_x"][0]), ("delta", delta, ref["d_delta"][0])):
        num = np.zeros_like(arr)
        for i in np.ndindex(arr.shape):
            p, m = arr.copy(), arr.copy()
            p[i] += h
            m[i] -= h
            num[i] = 0.7 * (loss(p, delta) - loss(m, delta) if which == "x" else loss(x, p) - loss(x, m)) / (2 * h)
        err = np.abs(num - got).max()
        print(f"{kind} weighted={weighted} d_{which}: max |central difference - closed form| {err:.2e}")
        assert err < 1e-9
    # the pieces: corrected and mse by hand for one ray
    A, b = ER.affine(delta)
    r = 5
    c = A[ids[r]] @ x[r] + b[ids[r]]
    assert np.allclose(ref["corrected"][0][r], c, rtol=0, atol=1e-15)
    assert np.isclose(ref["mse"][0], ((ref["corrected"][0] - y) ** 2).mean(), rtol=1e-14)
    # apply_bwd is the chain rule of corrected alone: the L2 gradient is apply_bwd of 2 w e / 3R
    e = ref["corrected"][0] - y
    if kind == "l2":
        g = 0.7 * 2.0 * (np.ones(R) if w is None else w.astype(np.float64))[:, None] * e / (3 * R)
        ab = ER.apply_bwd(x, ids, delta, g)
        assert np.allclose(ab["d_x"][0], ref["d_x"][0], rtol=1e-12, atol=1e-18)
        assert np.allclose(ab["d_delta"][0], ref["d_delta"][0], rtol=1e-12, atol=1e-18)


def test_reference_sign_of_zero_is_zero_and_ids_are_clamped():
    x = np.array([[0.25, 0.5, 0.75]], np.float32)
    delta = np.zeros((2, 12), np.float32)
    ref = ER.fwd_bwd(x, x.copy(), [7], delta, "l1")
    assert ref["loss"][0] == 0.0 and not ref["d_x"][0].any() and not ref["d_delta"][0].any()
    assert ref["count"].tolist() == [0, 1]       # (7 clamps to N - 1)
    assert ER.fwd_bwd(x, x.copy(), [-3], delta, "l1")["count"].tolist() == [1, 0]


@pytest.mark.parametrize("R,N", ER.cases())
def test_shared_inputs_keep_the_l1_residuals_away_from_zero(R, N):
    """the GPU test leaves out of its d_x / d_delta comparison what a residual with |e| < 8 * 2^-24 * mag enters, and asserts
    that this is at most 0.1 % of the 3R residuals: the restatement alone must stay inside that cap on every case"""
    for kind, weighted, pattern in ER.variants():
        x, y, ids, delta, w = ER.inputs(R, N, pattern, weighted)
        assert x.min() >= 0 and x.max() <= 1 and np.abs(delta).max() <= 0.3 and 0 <= ids.min() and ids.max() < N
        ref = ER.fwd_bwd(x, y, ids, delta, kind, w)
        assert ref["flip"].mean() <= ER.FLIP_CAP, (kind, weighted, pattern, int(ref["flip"].sum()))
        # ... and so must what the GPU test then leaves out: whole rays of d_x, and the d_delta elements a flip enters
        left_x = ref["flip"].any(axis=1).mean()
        left_d = ER.delta_rows_with_flips(ids, N, ref["flip"]).mean()
        assert left_x <= ER.FLIP_CAP and left_d <= ER.FLIP_CAP, (kind, weighted, pattern, left_x, left_d)
        if pattern == "unused" and N > 1:
            assert not ref["used"].all()
        if pattern.startswith("runs") and N > 1 and R > 65:
            first = int(pattern[4:])
            assert ids[first - 1] == 0 and ids[first] == 1 and (np.diff(ids) >= 0).all()


@pytest.mark.parametrize("N,P", [(1, 1), (3, 5), (2, 1499)])
def test_reference_fit_sums_solve_to_the_affine(N, P):
    rng = np.random.default_rng(P)
    x = rng.uniform(0, 1, (N, P, 3)).astype(np.float32)
    A = np.eye(3) + rng.uniform(-0.3, 0.3, (N, 3, 3))
    b = rng.uniform(-0.05, 0.05, (N, 3))
    y = (np.einsum("ncj,npj->npc", A, x.astype(np.float64)) + b[:, None, :]).astype(np.float32)
    sums, sabs = ER.fit_sums(x, y)
    assert sums.shape == (N, 25) and (sabs >= np.abs(sums)).all() and np.array_equal(sums[:, 9], np.full(N, float(P)))
    G, h = ER.gram(sums)
    assert np.allclose(G[:, 0, 3], x.astype(np.float64)[..., 0].sum(1)) and np.allclose(h[:, 3, 2], y.astype(np.float64)[..., 2].sum(1))
    # the host-side solve of the library on these sums: finite always, the affine where the image determines it
    As, bs = ops.solve_affine_colour(torch.from_numpy(sums))
    assert As.shape == (N, 3, 3) and bs.shape == (N, 3) and As.dtype == torch.float64
    assert bool(torch.isfinite(As).all()) and bool(torch.isfinite(bs).all())
    if P >= 1000:
        assert np.abs(As.numpy() - A).max() < 1e-5 and np.abs(bs.numpy() - b).max() < 1e-5     # (y was rounded to float32)


def test_solve_of_a_constant_image_is_finite_and_reproduces_it():
    x = np.full((1, 50, 3), 0.5, np.float32)
    y = np.full((1, 50, 3), 0.25, np.float32)
    A, b = ops.solve_affine_colour(torch.from_numpy(ER.fit_sums(x, y)[0]))
    assert bool(torch.isfinite(A).all()) and bool(torch.isfinite(b).all())
    assert np.allclose((A[0] @ torch.full((3,), 0.5, dtype=torch.float64) + b[0]).numpy(), 0.25, atol=1e-8)


# ---- C ABI ------------------------------------------------------------------------------------------------------------
def _lib():
    from voxe_hip import build

    return abi.declare(ctypes.CDLL(build.build()), "voxe_")


CTYPES = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "float": ctypes.c_float, "size_t": ctypes.c_size_t}
PROTOTYPES = {
    "voxe_exposure_fwd_bwd": ["x", "y", "image_id", "R", "delta", "N", "kind", "ray_weight", "grad_scale", "loss_out", "mse_out",
                              "corrected", "d_x", "d_delta", "accumulate", "scratch", "scratch_bytes", "stream"],
    "voxe_exposure_apply_bwd": ["x", "image_id", "R", "delta", "N", "d_corrected", "d_x", "d_delta", "accumulate", "scratch",
                                "scratch_bytes", "stream"],
    "voxe_exposure_fit_sums": ["x", "y", "N", "P", "sums", "scratch", "scratch_bytes", "stream"],
}
SIZES = ("voxe_exposure_scratch_bytes", "voxe_exposure_fit_scratch_bytes")


def test_exposure_symbols_are_declared_and_match_the_header():
    text = open(os.path.join(ROOT, "include", "voxe.h")).read()
    L = _lib()
    assert abi.ABI_VERSION == 13 and L.voxe_abi_version() == 13
    assert not any("exposure" in s for s in abi.cpu_symbols())
    assert "voxe_exposure.hip" in __import__("voxe_hip.build", fromlist=["SOURCES"]).SOURCES
    for name in tuple(PROTOTYPES) + SIZES:
        assert re.search(rf"\b{name}\s*\(", text) and name in abi.hip_symbols() and hasattr(L, name), name
    for name, names in PROTOTYPES.items():
        proto = re.search(rf"int {name}\((.*?)\);", text, re.S).group(1)
        proto = re.sub(r"/\*.*?\*/", "", proto, flags=re.S)
        args = [a.split() for a in proto.split(",")]
        assert [a[-1].lstrip("*") for a in args] == names, name
        argtypes = getattr(L, name).argtypes
        assert len(argtypes) == len(names), name
        for a, ct in zip(args, argtypes):
            if "*" in "".join(a):
                assert ct not in CTYPES.values(), (name, a)
            else:
                assert ct is CTYPES[a[-2]], (name, a)
    for name in SIZES:
        assert getattr(L, name).argtypes == [ctypes.c_int64, ctypes.c_int64] and getattr(L, name).restype is ctypes.c_size_t


def test_validation_without_a_device():
    L = _lib()
    P = ctypes.c_void_p(16)
    need = L.voxe_exposure_scratch_bytes(1499, 7)
    assert need >= 7 * 12 * 8 + 2 * 8 * 2 and L.voxe_exposure_scratch_bytes(-1, 7) == 0 and L.voxe_exposure_scratch_bytes(4, 0) == 0
    assert L.voxe_exposure_scratch_bytes(1 << 31, 1) == 0

    def call(x=P, y=P, ids=P, R=1499, delta=P, N=7, kind=abi.DREG_L1, w=None, loss=None, mse=None, corr=None, dx=None, dd=None,
             acc=0, sc=P, nbytes=need):
        return L.voxe_exposure_fwd_bwd(x, y, ids, R, delta, N, kind, w, 1.0, loss, mse, corr, dx, dd, acc, sc, nbytes, None)

    for missing in ("x", "y", "ids", "delta"):
        assert call(**{missing: None}) == abi.ERR_NULL_POINTER, missing
    assert call(R=-1) == abi.ERR_BAD_SHAPE and call(R=1 << 31) == abi.ERR_BAD_SHAPE
    assert call(N=0) == abi.ERR_BAD_SHAPE and call(N=1 << 24) == abi.ERR_BAD_SHAPE
    assert call(kind=abi.DREG_CORRELATION) == abi.ERR_UNSUPPORTED and call(kind=9) == abi.ERR_UNSUPPORTED
    # every output that is reduced needs the scratch; corrected and d_x do not
    for out in ("loss", "mse", "dd"):
        assert call(**{out: P}, sc=None) == abi.ERR_WORKSPACE and call(**{out: P}, nbytes=need - 1) == abi.ERR_WORKSPACE, out
    # no launch: all outputs NULL (with or without scratch), or R == 0 without an output to zero (NULL rays allowed)
    assert call() == abi.OK and call(sc=None, nbytes=0) == abi.OK and call(w=P, kind=abi.DREG_L2) == abi.OK
    assert call(x=None, y=None, ids=None, R=0, corr=P, dx=P, sc=None, nbytes=0) == abi.OK
    assert call(x=None, y=None, ids=None, R=0, dd=P, acc=1, sc=None, nbytes=0) == abi.OK

    def back(x=P, ids=P, R=1499, delta=P, N=7, g=P, dx=None, dd=None, acc=0, sc=P, nbytes=need):
        return L.voxe_exposure_apply_bwd(x, ids, R, delta, N, g, dx, dd, acc, sc, nbytes, None)

    for missing in ("x", "ids", "delta", "g"):
        assert back(**{missing: None}) == abi.ERR_NULL_POINTER, missing
    assert back(R=-1) == abi.ERR_BAD_SHAPE and back(N=0) == abi.ERR_BAD_SHAPE
    assert back(dd=P, sc=None) == abi.ERR_WORKSPACE and back(dd=P, nbytes=need - 1) == abi.ERR_WORKSPACE
    assert back() == abi.OK and back(x=None, ids=None, g=None, R=0, dx=P) == abi.OK

    fneed = L.voxe_exposure_fit_scratch_bytes(3, 1499)
    assert fneed >= 25 * 8 * 3 and L.voxe_exposure_fit_scratch_bytes(0, 5) == 0 and L.voxe_exposure_fit_scratch_bytes(1, 0) == 0

    def fit(x=P, y=P, N=3, Pn=1499, sums=P, sc=P, nbytes=fneed):
        return L.voxe_exposure_fit_sums(x, y, N, Pn, sums, sc, nbytes, None)

    for missing in ("x", "y", "sums"):
        assert fit(**{missing: None}) == abi.ERR_NULL_POINTER, missing
    assert fit(N=0) == abi.ERR_BAD_SHAPE and fit(Pn=0) == abi.ERR_BAD_SHAPE and fit(N=65536) == abi.ERR_BAD_SHAPE
    assert fit(sc=None) == abi.ERR_WORKSPACE and fit(nbytes=fneed - 1) == abi.ERR_WORKSPACE


def test_operator_refuses_host_tensors_and_bad_arguments():
    from voxe_hip.runtime import VoxeError

    x, y = torch.rand(8, 3), torch.rand(8, 3)
    ids, delta = torch.zeros(8, dtype=torch.int32), torch.zeros(2, 12)
    with pytest.raises(VoxeError):
        ops.exposure_loss(x, y, ids, delta)                 # host tensors
    with pytest.raises(VoxeError, match="kind"):
        ops.exposure_loss(x, y, ids, delta, kind="huber")
    with pytest.raises(VoxeError, match="target receives no gradient"):
        ops.exposure_loss(x, y.clone().requires_grad_(True), ids, delta)
    with pytest.raises(VoxeError, match="ray_weight receives no gradient"):
        ops.exposure_loss(x, y, ids, delta, ray_weight=torch.ones(8).requires_grad_(True))
    with pytest.raises(VoxeError):
        ops.fit_affine_colour(torch.rand(1, 5, 3), torch.rand(1, 5, 3))
    for name in ("exposure_fwd_bwd", "exposure_loss", "exposure_apply", "exposure_apply_bwd", "fit_affine_colour", "exposure_fit_sums",
                 "solve_affine_colour"):
        assert callable(getattr(ops, name)), name
    sig = inspect.signature(ops.exposure_loss)
    assert list(sig.parameters) == ["colour", "target", "image_ids", "delta", "kind", "ray_weight", "return_corrected"]
    assert sig.parameters["kind"].default == "l1" and sig.parameters["return_corrected"].default is False


# ---- the module and the checkpoint ------------------------------------------------------------------------------------
def test_module_starts_as_the_identity_and_round_trips_through_a_checkpoint(tmp_path):
    from thre3d_atom._keys import CHECKPOINT_KEYS
    from thre3d_atom.modules.volumetric_model import VolumetricModel, create_volumetric_model_from_saved_model
    from thre3d_atom.thre3d_reprs.exposure import PerImageExposure
    from thre3d_atom.thre3d_reprs.renderers import SHVoxGridRenderConfig, render_sh_voxel_grid
    from thre3d_atom.thre3d_reprs.voxels import VoxelGrid, VoxelSize, create_voxel_grid_from_saved_info_dict
    from thre3d_atom.utils.imaging_utils import CameraBounds

    assert CHECKPOINT_KEYS["EXPOSURE"] == "exposure"
    module = PerImageExposure(5)
    assert module.delta.shape == (5, 12) and not module.delta.detach().any() and module.get_save_config_dict() == {"num_images": 5}
    assert float(module.regulariser().detach()) == 0.0
    with torch.no_grad():
        module.delta.copy_(torch.arange(60, dtype=torch.float32).reshape(5, 12) / 64)
    assert float(module.regulariser().detach()) == pytest.approx(float((module.delta.detach() ** 2).mean()))
    with pytest.raises(ValueError):
        PerImageExposure(0)
    with pytest.raises(ValueError):
        module.check_image_ids(torch.tensor([0, 5]))
    module.check_image_ids(torch.tensor([0, 4]))

    def model(exposure=None):
        vg = VoxelGrid(torch.zeros(4, 4, 4, 1), torch.zeros(4, 4, 4, 3), VoxelSize(0.1, 0.1, 0.1), tunable=True)
        vm = VolumetricModel(vg, render_sh_voxel_grid, SHVoxGridRenderConfig(8, CameraBounds(1.0, 4.0)), device=CPU)
        vm.exposure = exposure
        return vm

    plain, with_exposure = model(), model(module)
    assert plain.exposure is None and "exposure" not in plain.get_save_info()
    torch.save(plain.get_save_info(), tmp_path / "plain.pth")
    torch.save(with_exposure.get_save_info(), tmp_path / "exposed.pth")
    loaded, _ = create_volumetric_model_from_saved_model(tmp_path / "plain.pth", create_voxel_grid_from_saved_info_dict, device=CPU)
    assert loaded.exposure is None
    loaded, _ = create_volumetric_model_from_saved_model(tmp_path / "exposed.pth", create_voxel_grid_from_saved_info_dict, device=CPU)
    assert torch.equal(loaded.exposure.delta, module.delta) and not loaded.exposure.delta.requires_grad


# ---- samplers -----------------------------------------------------------------------------------------------------------
def test_samplers_return_the_image_row_of_every_ray(monkeypatch):
    from thre3d_atom.rendering.volumetric.utils import misc
    from thre3d_atom.utils.imaging_utils import CameraIntrinsics

    H, W, K = 6, 5, 3
    seen = {}

    def fake_cast(height, width, focal, poses, flat_index):
        seen["flat"] = flat_index.clone()
        return torch.zeros(flat_index.numel(), 3), torch.ones(flat_index.numel(), 3)

    monkeypatch.setattr(misc._ops, "cast_rays_indexed", fake_cast)
    images = torch.arange(7 * 3 * H * W, dtype=torch.float32).reshape(7, 3, H, W)
    poses = torch.eye(4)[None, :3].repeat(K, 1, 1)
    intr = CameraIntrinsics(H, W, 10.0)
    picks = torch.tensor([6, 2, 4])
    for memory_order in (False, True):
        torch.manual_seed(3)
        rays, pixels, ids = misc.sample_random_rays_and_pixels_from_cameras(intr, poses, images, 40, image_ids=picks,
                                                                            memory_order=memory_order, return_image_ids=True)
        cam = seen["flat"] // (H * W)
        assert ids.dtype == torch.int32 and ids.shape == (40,) and torch.equal(ids.long(), picks[cam])
        rem = seen["flat"] % (H * W)
        assert torch.equal(pixels, images[ids.long(), :, rem // W, rem % W])
        if memory_order:
            assert bool((cam[1:] >= cam[:-1]).all())
        torch.manual_seed(3)
        two = misc.sample_random_rays_and_pixels_from_cameras(intr, poses, images, 40, image_ids=picks, memory_order=memory_order)
        assert len(two) == 2 and torch.equal(two[1], pixels)          # default calls are unchanged
    # without image_ids the row is the camera
    rays, pixels, ids = misc.sample_random_rays_and_pixels_from_cameras(intr, poses, images, 20, return_image_ids=True)
    assert torch.equal(ids.long(), seen["flat"] // (H * W))
    torch.manual_seed(5)
    rays, pixels, ids = misc.sample_random_patches_and_pixels_from_cameras(intr, poses, images, 4, 3, image_ids=picks,
                                                                           return_image_ids=True)
    cam = seen["flat"] // (H * W)
    assert ids.dtype == torch.int32 and ids.shape == (36,) and torch.equal(ids.long(), picks[cam])
    assert bool((ids.view(4, 9) == ids.view(4, 9)[:, :1]).all())       # one image per patch
    torch.manual_seed(5)
    assert len(misc.sample_random_patches_and_pixels_from_cameras(intr, poses, images, 4, 3, image_ids=picks)) == 2


# ---- trainer options and documents ------------------------------------------------------------------------------------
def test_cli_options_trainer_arguments_and_documents():
    spec = importlib.util.spec_from_file_location("train_exposure_cli", os.path.join(ROOT, "train_sh_based_voxel_grid_with_posed_images.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    opts = {p.name: p for p in mod.main.params}
    for name, default in (("exposure_learning_rate", 0.0), ("exposure_regularization", 1e-3)):
        assert opts[name].default == default and f"--{name}" in opts[name].opts
    assert "untuned" in opts["exposure_regularization"].help
    from thre3d_atom.modules import testers, trainers

    sig = inspect.signature(trainers.train_sh_vox_grid_vol_mod_with_posed_images)
    assert sig.parameters["exposure_learning_rate"].default == 0.0 and sig.parameters["exposure_regularization"].default == 1e-3
    assert inspect.signature(testers.test_sh_vox_grid_vol_mod_with_posed_images).parameters["colour_corrected"].default is False
    header = open(os.path.join(ROOT, "include", "voxe.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    for name in ("voxe_exposure_fwd_bwd", "voxe_exposure_fit_sums", "voxe_exposure_apply_bwd"):
        assert name in header and name in integration, name
    assert "--exposure_learning_rate" in readme and "--exposure_learning_rate" in integration and "voxe_exposure.hip" in readme
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "4.21" in design and "profiles/exposure_bench.txt" in design
    assert "exposure_bench.py" in open(os.path.join(ROOT, "tools", "README.md")).read()


def test_trainer_refuses_negative_options_and_other_channel_counts(tmp_path):
    from thre3d_atom.modules import trainers
    from thre3d_atom.modules.volumetric_model import VolumetricModel
    from thre3d_atom.thre3d_reprs.renderers import SHVoxGridRenderConfig, render_sh_voxel_grid
    from thre3d_atom.thre3d_reprs.voxels import VoxelGrid, VoxelSize
    from thre3d_atom.utils.imaging_utils import CameraBounds, CameraIntrinsics

    class Data:
        def __init__(self, channels):
            self.images = torch.rand(4, channels, 8, 8)
            self.poses = torch.eye(4)[None, :3].repeat(4, 1, 1)
            self.camera_intrinsics = CameraIntrinsics(8, 8, 10.0)
            self.camera_bounds = CameraBounds(1.0, 4.0)

        def downsampled(self, f):
            return self

        def to(self, device):
            return self

        def __len__(self):
            return 4

        def get_hemispherical_radius_estimate(self):
            return 4.0

    def run(channels=3, **kw):
        vg = VoxelGrid(torch.zeros(4, 4, 4, 1), torch.zeros(4, 4, 4, 3), VoxelSize(0.1, 0.1, 0.1), tunable=True)
        vm = VolumetricModel(vg, render_sh_voxel_grid, SHVoxGridRenderConfig(8, CameraBounds(1.0, 4.0)), device=CPU)
        trainers.train_sh_vox_grid_vol_mod_with_posed_images(vm, Data(channels), tmp_path, num_stages=1, num_iterations_per_stage=1,
                                                             fast_debug_mode=True, **kw)

    for bad in (dict(exposure_learning_rate=-1e-3), dict(exposure_learning_rate=1e-3, exposure_regularization=-1.0),
                dict(exposure_regularization=-1.0)):
        with pytest.raises(ValueError, match="exposure"):
            run(**bad)
    with pytest.raises(ValueError, match="3 channels"):
        run(channels=4, exposure_learning_rate=1e-3)
