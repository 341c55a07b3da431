"""CPU checks of the robust photometric loss on pixel patches: the numpy restatement tests/robust_ref.py against
cases worked by hand, the C ABI's declarations and argument validation (no device work), the Python wrappers' argument checks, the
trainer's options, and the documents."""
import ctypes
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest
import torch

import robust_ref as RR
from conftest import ROOT
from voxe_hip import abi, ops
from voxe_hip.runtime import VoxeError

CPU = torch.device("cpu")
I, O = 0.25, 0.5      # roots of an inlier's and an outlier's residual: e = 0.0625 and 0.25, both exact


# ---- the restatement -----------------------------------------------------------------------------------------------------------
#   row 0: I I I O      the outliers and the inliers in their 3x3 neighbourhoods inside the patch:
#   row 1: I O I I        (0,3) corner 3,  (1,1) interior 8,  (3,0) corner 2,  (3,1) edge 4
#   row 2: I I I I
#   row 3: O O I I
HAND = np.array([[I, I, I, O], [I, O, I, I], [I, I, I, I], [O, O, I, I]], np.float32)


def _hand():
    x = HAND.reshape(1, 4, 4, 1).copy()
    return x, np.zeros_like(x)


def test_restatement_on_a_patch_worked_by_hand():
    x, y = _hand()
    assert np.array_equal(RR.residuals(x, y)[0], HAND * HAND)
    a = (HAND == I).astype(np.int64)[None]
    assert RR.neighbour_counts(a)[0][[0, 1, 3, 3], [3, 1, 0, 1]].tolist() == [3, 8, 2, 4]
    # rank 11 is the last of the 12 inliers: tau = 0.0625.  smooth_min 4 forgives (1,1) and (3,1), not the two corners
    r = RR.fwd_bwd(x, y, rank=11, smooth_min=4, patch_min=17)
    want = np.array([[1, 1, 1, 0], [1, 1, 1, 1], [1, 1, 1, 1], [0, 1, 1, 1]], np.uint8)
    assert r["tau"] == np.float32(0.0625) and r["stats"] == (12, 14, 14) and np.array_equal(r["mask"][0], want)
    assert r["loss"] == (12 * 0.25 + 2 * 0.5) / 16 and r["mse"] == (12 * 0.0625 + 4 * 0.25) / 16
    assert np.array_equal(r["d_x"][0, :, :, 0], want.astype(np.float32) / 16)           # (sign +, g = 1 / 16)
    l2 = RR.fwd_bwd(x, y, rank=11, smooth_min=4, patch_min=17, kind="l2", grad_scale=0.5)
    assert l2["loss"] == (12 * 0.0625 + 2 * 0.25) / 16 and l2["mse"] == r["mse"]
    assert np.array_equal(l2["d_x"][0, :, :, 0], want * (2 * 0.5 / 16) * HAND)
    # rank 12 is the first outlier: everything is an inlier
    assert RR.fwd_bwd(x, y, rank=12)["stats"] == (16, 16, 16) and RR.fwd_bwd(x, y, rank=12)["tau"] == np.float32(0.25)
    # smooth_min 9 forgives nobody; the patch rule at 12 then forgives the inner outlier (1,1) and no other
    off = RR.fwd_bwd(x, y, rank=11, smooth_min=9, patch_min=13)
    on = RR.fwd_bwd(x, y, rank=11, smooth_min=9, patch_min=12)
    assert off["stats"] == (12, 12, 12) and on["stats"] == (12, 12, 13)
    assert on["mask"][0, 1, 1] == 1 and on["mask"][0, 0, 3] == 0 and on["mask"][0, 3, 0] == 0 and on["mask"][0, 3, 1] == 0
    # a mask from outside replaces all of it
    given = np.zeros((1, 4, 4), np.uint8)
    given[0, 0, 3] = 7
    m = RR.fwd_bwd(x, y, mask_in=given)
    assert m["stats"] == (0, 0, 0) and m["tau"] == 0 and m["loss"] == 0.5 / 16 and m["mask"].sum() == 1 and m["mask"][0, 0, 3] == 1
    assert m["mse"] == r["mse"]
    # sign(0) = 0, negative residuals point the other way
    z = RR.fwd_bwd(x, x.copy(), rank=3)
    assert z["loss"] == 0 and z["tau"] == 0 and z["stats"] == (16, 16, 16) and not z["d_x"].any()
    assert (RR.fwd_bwd(y, x, rank=15)["d_x"] == -1.0 / 16).all()


def test_neighbourhood_counts_at_a_corner_on_an_edge_and_inside():
    ones = np.ones((2, 6, 6), np.int64)
    n = RR.neighbour_counts(ones)
    assert n[0, 0, 0] == n[1, 5, 5] == n[0, 0, 5] == 4 and n[0, 0, 2] == n[1, 3, 0] == n[0, 5, 4] == 6 and n[0, 2, 3] == 9
    # nothing crosses into the next patch
    one = np.zeros((2, 6, 6), np.int64)
    one[0] = 1
    assert not RR.neighbour_counts(one)[1].any() and np.array_equal(RR.neighbour_counts(one)[0], n[0])
    single = np.zeros((1, 4, 4), np.int64)
    single[0, 1, 2] = 1
    assert RR.neighbour_counts(single)[0].tolist() == [[0, 1, 1, 1], [0, 1, 1, 1], [0, 1, 1, 1], [0, 0, 0, 0]]


def test_inner_region():
    assert np.array_equal(np.argwhere(RR.inner(4)), [[1, 1], [1, 2], [2, 1], [2, 2]])
    six = RR.inner(6)                       # P / 4 = 1, P / 2 = 3: rows and columns 1, 2, 3
    assert six.sum() == 9 and six[1:4, 1:4].all()
    sixteen = RR.inner(16)
    assert sixteen.sum() == 64 and sixteen[4:12, 4:12].all()


def test_rank_of_a_quantile():
    M = 768
    assert RR.rank_of_quantile(0.0, M) == 0 and RR.rank_of_quantile(1e-9, M) == 0 and RR.rank_of_quantile(1.0, M) == M - 1
    assert RR.rank_of_quantile(0.5, M) == 383           # q M = 384 exactly: the 384th smallest, 0-based 383
    assert RR.rank_of_quantile(0.5, 5) == 2 and RR.rank_of_quantile(0.25, 16) == 3 and RR.rank_of_quantile(0.26, 16) == 4
    assert RR.rank_of_quantile(1.0, 1) == 0 and RR.rank_of_quantile(0.999999, M) == M - 1
    assert RR.patch_min_of_fraction(0.6, 16) == 154 and RR.patch_min_of_fraction(0.5, 4) == 8 and RR.patch_min_of_fraction(0.0, 4) == 1
    assert RR.patch_min_of_fraction(1.0, 6) == 36 and RR.patch_min_of_fraction(None, 6) == 37
    # the library derives the same integers
    for q, f, P, N in ((0.5, 0.6, 16, 3), (0.0, 0.0, 4, 1), (1.0, 1.0, 6, 5), (0.26, None, 4, 1), (0.8, 0.9, 64, 2)):
        M = N * P * P
        assert ops.robust_parameters(M, P, q, 5, f) == (RR.rank_of_quantile(q, M), 5, RR.patch_min_of_fraction(f, P))
    for bad in (dict(inlier_quantile=-0.1), dict(inlier_quantile=1.5), dict(smooth_min_count=0), dict(smooth_min_count=10),
                dict(smooth_min_count=4.5), dict(patch_inlier_fraction=1.01), dict(patch_inlier_fraction=-1.0)):
        with pytest.raises(VoxeError):
            ops.robust_parameters(256, 16, **bad)


def test_shared_inputs_hold_no_denormal_residual():
    for N, P, C in RR.SHAPES + (RR.MANY_PATCHES,):
        x, y = RR.inputs(N, P, C)
        d = x - y
        assert x.shape == (N, P, P, C) and x.dtype == np.float32 and (np.abs(d[d != 0]) > 2.0 ** -60).all()
        e = RR.residuals(x, y)
        assert (e[e != 0] >= np.finfo(np.float32).tiny).all()


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------
def _lib():
    from voxe_hip import build

    return abi.declare(ctypes.CDLL(build.build()), "voxe_")


CTYPES = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "float": ctypes.c_float, "size_t": ctypes.c_size_t}
NAMES = ["x", "y", "N", "P", "C", "kind", "rank", "smooth_min", "patch_min", "mask_in", "grad_scale", "loss_out", "mse_out",
         "tau_out", "mask_out", "stats", "d_x", "scratch", "scratch_bytes", "stream"]


def test_robust_symbols_are_declared_and_match_the_header():
    text = open(os.path.join(ROOT, "include", "voxe.h")).read()
    L = _lib()
    assert abi.ABI_VERSION == 13 and L.voxe_abi_version() == 13
    assert not any("robust" in s for s in abi.cpu_symbols())
    assert "voxe_robust.hip" in __import__("voxe_hip.build", fromlist=["SOURCES"]).SOURCES
    for name in ("voxe_robust_fwd_bwd", "voxe_robust_scratch_bytes"):
        assert re.search(rf"\b{name}\s*\(", text) and name in abi.hip_symbols() and hasattr(L, name), name
    proto = re.search(r"int voxe_robust_fwd_bwd\((.*?)\);", text, re.S).group(1)
    proto = re.sub(r"/\*.*?\*/", "", proto, flags=re.S)
    args = [a.split() for a in proto.split(",")]
    assert [a[-1].lstrip("*") for a in args] == NAMES
    argtypes = L.voxe_robust_fwd_bwd.argtypes
    assert len(argtypes) == len(NAMES)
    for a, ct in zip(args, argtypes):
        if "*" in "".join(a):
            assert ct not in CTYPES.values(), a
        else:
            assert ct is CTYPES[a[-2]], a
    assert L.voxe_robust_scratch_bytes.argtypes == [ctypes.c_int32] * 3 and L.voxe_robust_scratch_bytes.restype is ctypes.c_size_t
    # the header says what the issue left to it: the aliasing rule and the denormals
    section = text[text.index("Robust photometric loss on pixel patches"):text.index("size_t voxe_robust_scratch_bytes")]
    assert "mask_out may be the same buffer as mask_in" in section and "denormal" in section and "No float atomic" in section


def test_validation_without_a_device():
    L = _lib()
    P = ctypes.c_void_p(16)
    need = L.voxe_robust_scratch_bytes(3, 16, 3)
    assert need >= 3 * 2048 * 4 + 768 * 4 + 3 * 2 * 8
    for bad in ((0, 16, 3), (-1, 16, 3), (3, 2, 3), (3, 66, 3), (3, 15, 3), (3, 16, 0), (3, 16, 5), (1 << 19, 64, 1)):
        assert L.voxe_robust_scratch_bytes(*bad) == 0, bad
    assert L.voxe_robust_scratch_bytes((1 << 19) - 1, 64, 4) > 0 and L.voxe_robust_scratch_bytes(1, 4, 1) > 0

    def call(x=P, y=P, N=3, Pn=16, C=3, kind=abi.DREG_L1, rank=383, smooth=5, patch=154, mask_in=None, loss=None, mse=None, tau=None,
             mask=None, stats=None, dx=None, sc=P, nbytes=need):
        return L.voxe_robust_fwd_bwd(x, y, N, Pn, C, kind, rank, smooth, patch, mask_in, 1.0, loss, mse, tau, mask, stats, dx, sc,
                                     nbytes, None)

    every = dict(loss=P, mse=P, tau=P, mask=P, stats=P, dx=P)
    for missing in ("x", "y", "sc"):
        assert call(**{missing: None}, **every) == abi.ERR_NULL_POINTER, missing
    for shape in (dict(N=0), dict(Pn=2), dict(Pn=66), dict(Pn=15), dict(C=0), dict(C=5), dict(N=1 << 19, Pn=64, C=1)):
        assert call(**shape, **every) == abi.ERR_BAD_SHAPE, shape
    for param in (dict(rank=-1), dict(rank=768), dict(smooth=0), dict(smooth=10), dict(patch=0), dict(patch=258)):
        assert call(**param, **every) == abi.ERR_BAD_SHAPE, param
        # (with a mask from outside the three integers are ignored; all outputs NULL: nothing is launched)
        assert call(**param, mask_in=P) == abi.OK, param
    assert call(kind=abi.DREG_CORRELATION, **every) == abi.ERR_UNSUPPORTED and call(kind=9, **every) == abi.ERR_UNSUPPORTED
    assert call(nbytes=need - 1, **every) == abi.ERR_WORKSPACE and call(nbytes=0, **every) == abi.ERR_WORKSPACE
    assert call(nbytes=need - 1, mask_in=P, mask=P) == abi.ERR_WORKSPACE
    # the order: pointers, shape, kind, workspace
    assert call(x=None, N=0, kind=9, nbytes=0, **every) == abi.ERR_NULL_POINTER
    assert call(N=0, kind=9, nbytes=0, **every) == abi.ERR_BAD_SHAPE and call(kind=9, nbytes=0, **every) == abi.ERR_UNSUPPORTED
    # no launch: all outputs NULL, at the extremes of the parameters too
    assert call() == abi.OK and call(rank=0, smooth=1, patch=1) == abi.OK and call(rank=767, smooth=9, patch=257) == abi.OK
    assert call(kind=abi.DREG_L2, mask_in=P) == abi.OK


def test_operators_refuse_bad_arguments():
    x, y = torch.rand(2, 4, 4, 3), torch.rand(2, 4, 4, 3)
    with pytest.raises(VoxeError, match="only runs on a ROCm GPU"):
        ops.robust_loss(x, y)                                           # host tensors
    with pytest.raises(VoxeError, match="only runs on a ROCm GPU"):
        ops.robust_mask(x, y)
    with pytest.raises(VoxeError, match="kind"):
        ops.robust_loss(x, y, kind="huber")
    with pytest.raises(VoxeError, match="y receives no gradient"):
        ops.robust_loss(x, y.clone().requires_grad_(True))
    for shape in ((2, 4, 4), (2, 4, 6, 3), (2, 5, 5, 3), (2, 2, 2, 3), (1, 66, 66, 1), (2, 4, 4, 5), (0, 4, 4, 3)):
        with pytest.raises(VoxeError, match=r"\[N,P,P,C\]|square patches"):
            ops.robust_loss(torch.rand(*shape), torch.rand(*shape))
    with pytest.raises(VoxeError, match="one shape"):
        ops.robust_loss(x, torch.rand(2, 4, 4, 1))
    with pytest.raises(VoxeError, match="contiguous float32"):
        ops.robust_loss(x.double(), y.double())
    with pytest.raises(VoxeError, match="contiguous float32"):
        ops.robust_mask(torch.rand(2, 4, 3, 4).permute(0, 1, 3, 2), y)
    for name in ("robust_loss", "robust_mask", "robust_fwd_bwd", "robust_parameters"):
        assert callable(getattr(ops, name)), name
    sig = inspect.signature(ops.robust_loss)
    assert list(sig.parameters) == ["x", "y", "inlier_quantile", "smooth_min_count", "patch_inlier_fraction", "kind", "mask"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[2:]] == [0.5, 5, 0.6, "l1", None]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig.parameters)[2:])
    assert list(inspect.signature(ops.robust_mask).parameters) == ["x", "y", "inlier_quantile", "smooth_min_count",
                                                                   "patch_inlier_fraction"]


# ---- trainer options and documents ---------------------------------------------------------------------------------------------
def test_patch_side_of_a_stage():
    from thre3d_atom.thre3d_reprs.robust import check_robust_options, robust_patch_side

    assert robust_patch_side(16, 400, 400) == 16 and robust_patch_side(16, 13, 50) == 12 and robust_patch_side(16, 50, 5) == 4
    assert robust_patch_side(16, 3, 50) == 0 and robust_patch_side(64, 48, 48) == 48 and robust_patch_side(4, 4, 4) == 4
    check_robust_options(16, 0.5, 0.6)
    check_robust_options(4, 1.0, 0.0)
    for bad in ((15, 0.5, 0.6), (2, 0.5, 0.6), (66, 0.5, 0.6), (16, 0.0, 0.6), (16, 1.1, 0.6), (16, 0.5, -0.1), (16, 0.5, 1.1)):
        with pytest.raises(ValueError, match="robust_"):
            check_robust_options(*bad)


def test_cli_options_trainer_arguments_and_documents():
    spec = importlib.util.spec_from_file_location("train_robust_cli", os.path.join(ROOT, "train_sh_based_voxel_grid_with_posed_images.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    opts = {p.name: p for p in mod.main.params}
    defaults = (("robust_loss", False), ("robust_patch_size", 16), ("robust_inlier_quantile", 0.5), ("robust_patch_inlier_fraction", 0.6))
    for name, default in defaults:
        assert opts[name].default == default and f"--{name}" in opts[name].opts
    from thre3d_atom.modules import trainers

    sig = inspect.signature(trainers.train_sh_vox_grid_vol_mod_with_posed_images)
    for name, default in defaults:
        assert sig.parameters[name].default == default, name
    header = open(os.path.join(ROOT, "include", "voxe.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "voxe_robust_fwd_bwd" in header and "voxe_robust_fwd_bwd" in integration
    assert "--robust_loss" in readme and "--robust_loss" in integration and "voxe_robust.hip" in readme
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "4.22" in design and "profiles/robust_bench.txt" in design
    assert "robust_bench.py" in open(os.path.join(ROOT, "tools", "README.md")).read()
    assert os.path.exists(os.path.join(ROOT, "profiles", "robust_bench.txt"))


def _trainer_fixture(tmp_path, monkeypatch, calls, side=8):
    """the trainer on the CPU with every device call replaced by a recorder"""
    from thre3d_atom.modules import trainers
    from thre3d_atom.modules.volumetric_model import VolumetricModel
    from thre3d_atom.thre3d_reprs.renderers import SHVoxGridRenderConfig, render_sh_voxel_grid
    from thre3d_atom.thre3d_reprs.voxels import VoxelGrid, VoxelSize
    from thre3d_atom.utils.imaging_utils import CameraBounds, CameraIntrinsics

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

    def rays_of(n):
        return type("R", (), {"origins": torch.zeros(n, 3)})()

    def fake_pixels(intr, poses, images, n, **k):
        calls["pixels"].append((n, sorted(k)))
        return rays_of(16), torch.zeros(16, 3)

    def fake_patches(intr, poses, images, num_patches, patch, **k):
        calls["patches"].append((num_patches, patch))
        return rays_of(num_patches * patch * patch), torch.zeros(num_patches * patch * patch, 3)

    def fake_robust_loss(x, y, *, inlier_quantile=0.5, smooth_min_count=5, patch_inlier_fraction=0.6, kind="l1", mask=None):
        calls["robust"].append(dict(shape=tuple(x.shape), q=inlier_quantile, f=patch_inlier_fraction, mask=mask, grad=x.requires_grad,
                                    target_grad=y.requires_grad))
        out = torch.full(x.shape[:3], len(calls["robust"]), dtype=torch.uint8)
        return x.sum() * 0, torch.tensor(0.25), out, {"stats": torch.tensor([1, 2, 3]), "tau": torch.tensor(0.0)}

    monkeypatch.setattr(trainers, "FusedGridAdam", FakeOpt)
    monkeypatch.setattr(trainers, "scale_voxel_grid_with_required_output_size", lambda grid, size: grid)
    monkeypatch.setattr(trainers, "_render_params", lambda *a, **k: None)
    monkeypatch.setattr(trainers, "_next_rng", lambda: (0, 0))
    monkeypatch.setattr(VolumetricModel, "render_rays", fake_render_rays)
    monkeypatch.setattr(trainers, "sample_random_rays_and_pixels_from_cameras", fake_pixels)
    monkeypatch.setattr(trainers, "sample_random_patches_and_pixels_from_cameras", fake_patches)
    monkeypatch.setattr(ops, "robust_loss", fake_robust_loss)

    def run(**kw):
        vg = VoxelGrid(torch.zeros(4, 4, 4, 1), torch.zeros(4, 4, 4, 3), VoxelSize(0.1, 0.1, 0.1), tunable=True)
        vm = VolumetricModel(vg, render_sh_voxel_grid, SHVoxGridRenderConfig(8, CameraBounds(1.0, 4.0)), device=CPU)
        kw.setdefault("num_iterations_per_stage", 3)
        trainers.train_sh_vox_grid_vol_mod_with_posed_images(vm, Data(), tmp_path, num_stages=1, fast_debug_mode=True, **kw)

    return run


def _fresh():
    return {"one_call": 0, "render": 0, "pixels": [], "patches": [], "robust": []}


def test_trainer_refuses_bad_options_before_any_work(tmp_path, monkeypatch):
    calls = _fresh()
    run = _trainer_fixture(tmp_path, monkeypatch, calls)
    for bad in (dict(robust_patch_size=15), dict(robust_patch_size=2), dict(robust_patch_size=128), dict(robust_inlier_quantile=0.0),
                dict(robust_inlier_quantile=1.5), dict(robust_patch_inlier_fraction=-0.5), dict(robust_patch_inlier_fraction=2.0)):
        with pytest.raises(ValueError, match="robust_"):
            run(robust_loss=True, **bad)
    with pytest.raises(ValueError, match="ssim_weight"):
        run(robust_loss=True, ssim_weight=0.2)
    with pytest.raises(ValueError, match="holds no 8 x 8 patch"):
        run(robust_loss=True, robust_patch_size=8, ray_batch_size=63)
    assert calls == _fresh()
    # off, the robust options are not looked at
    run(robust_patch_size=15, robust_inlier_quantile=7.0)
    assert calls["one_call"] == 3


def test_robust_loss_off_leaves_the_iteration_as_it_was(tmp_path, monkeypatch):
    """robust_loss=False takes the trainer's code paths as they were: the one-call iteration, and -- where another option
    switches that off -- the random pixel set through the sampler with the arguments it had; on, the batch is patches and both
    L1 terms go through ops.robust_loss, the diffuse one under the specular one's mask"""
    calls = _fresh()
    run = _trainer_fixture(tmp_path, monkeypatch, calls)
    run()
    assert calls == dict(_fresh(), one_call=3)
    calls.update(_fresh())
    run(fused_iteration=False, ray_batch_size=4096)
    keys = ["fast_subset", "image_ids", "memory_order", "return_image_ids"]
    assert calls == dict(_fresh(), render=6, pixels=[(4096, keys)] * 3)
    calls.update(_fresh())
    run(robust_loss=True, robust_patch_size=4, ray_batch_size=100, robust_inlier_quantile=0.7, robust_patch_inlier_fraction=0.4)
    assert calls["one_call"] == 0 and calls["pixels"] == [] and calls["patches"] == [(6, 4)] * 3 and calls["render"] == 6
    assert len(calls["robust"]) == 6
    for first in (0, 2, 4):
        spec, diff = calls["robust"][first], calls["robust"][first + 1]
        assert spec["shape"] == diff["shape"] == (6, 4, 4, 3) and spec["mask"] is None and (spec["q"], spec["f"]) == (0.7, 0.4)
        assert spec["grad"] and diff["grad"] and not spec["target_grad"]
        # (the fake's mask holds its call's number: the diffuse call got the mask the specular call returned)
        assert diff["mask"] is not None and int(diff["mask"][0, 0, 0]) == first + 1
    # without the diffuse term: one call per iteration
    calls.update(_fresh())
    run(robust_loss=True, robust_patch_size=4, ray_batch_size=100, apply_diffuse_render_regularization=False)
    assert len(calls["robust"]) == 3 and all(c["mask"] is None for c in calls["robust"]) and calls["render"] == 3


def test_stage_with_small_images_uses_a_smaller_patch_or_the_plain_l1(tmp_path, monkeypatch):
    calls = _fresh()
    run = _trainer_fixture(tmp_path, monkeypatch, calls, side=7)
    run(robust_loss=True, robust_patch_size=16, ray_batch_size=100, num_iterations_per_stage=1)
    assert calls["patches"] == [(2, 6)] and len(calls["robust"]) == 2          # min(7, 7) rounded down to even
    calls.update(_fresh())
    run3 = _trainer_fixture(tmp_path, monkeypatch, calls, side=3)
    run3(robust_loss=True, ray_batch_size=100, num_iterations_per_stage=1)
    assert calls["patches"] == [] and calls["robust"] == [] and len(calls["pixels"]) == 1 and calls["render"] == 2
