"""Host checks of the checkpoint compression (thre3d_reprs/compression.py, the loader, the command lines) and of the numpy
restatements tests/test_vq_gpu.py holds voxe_vq.hip to: no GPU is needed for any of these.

Non-vacuity of the GPU assign test is shown HERE, on its own cases (vq_ref.assign_shapes, the seeds of vq_ref.assign_case): the
float32 restatement of the kernel's score stays inside the slack at every point and differs from the float64 arg-min on at most
1 % of the points of a case, while an assignment that ignores |c_k|^2 and one that drops the last channel of an odd F violate the
slack on the shares of points asserted below."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import vq_ref as R
from conftest import GOLDEN, ROOT
from voxe_hip import abi

CKPT = os.path.join(GOLDEN, "ref_checkpoint.pth")


def _cp():
    from thre3d_atom.thre3d_reprs import compression

    return compression


# ---- partition ------------------------------------------------------------------------------------------------------------------
HAND_MADE = {
    "ties": [5, 5, 5, 5, 3, 3, 0, 5],
    "zeros": [0, 0, 7, 0, 1, 0, 2, 0, 0],
    "all zero": [0, 0, 0, 0],
    "one holds all": [0, 0, 1 << 40, 0, 0],
    "descending": [9, 8, 7, 6, 5, 4, 3, 2, 1],
    "large": [(1 << 60) + 3, 1 << 59, 1 << 59, 12345, 1, 0, 1 << 59],
    "single": [42],
}
SHARES = [(1e-3, 0.6), (0.0, 0.0), (0.0, 1.0), (1.0, 0.0), (1.0, 1.0), (0.25, 0.5), (0.5, 0.75), (0.1, 0.0)]


@pytest.mark.parametrize("name", sorted(HAND_MADE))
def test_partition_equals_the_brute_force_loop(name):
    imp = np.array(HAND_MADE[name], dtype=np.int64)
    for prune, keep in SHARES:
        want = R.partition_loop(imp, prune, keep)
        assert np.array_equal(R.partition(imp, prune, keep), want), (prune, keep)
        got = _cp().partition(torch.from_numpy(imp), prune, keep)
        assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), want), (prune, keep, got, want)
    # shapes travel; zeros are always pruned; with nothing pruned by share and nothing kept every seen voxel is VQ (while the
    # total is exact as a float: beyond 2^53 the thresholds are those of the rounded total, as the loop's are)
    grid = _cp().partition(torch.from_numpy(imp).reshape(1, -1, 1), 0.0, 0.0)
    assert grid.shape == (1, len(imp), 1)
    if int(imp.sum()) < 1 << 53:
        assert np.array_equal(grid.reshape(-1).numpy(), np.where(imp == 0, 0, 1))


def test_partition_on_random_importances_and_its_refusals():
    rng = np.random.default_rng(3)
    imp = rng.integers(0, 1 << 36, size=(7, 5, 6)) * (rng.uniform(size=(7, 5, 6)) < 0.7)
    imp.reshape(-1)[:6] = imp.reshape(-1)[6:12]     # ties
    for prune, keep in SHARES:
        got = _cp().partition(torch.from_numpy(imp), prune, keep).numpy()
        assert np.array_equal(got, R.partition(imp, prune, keep)) and np.array_equal(got, R.partition_loop(imp, prune, keep))
    lab = R.partition(imp, 1e-3, 0.6)
    total = int(imp.sum())
    assert int(imp[lab == 2].sum()) >= int(0.6 * total) and int(imp[lab == 0].sum()) <= int(1e-3 * total) + 1
    assert {0, 1, 2} == set(np.unique(lab))
    with pytest.raises(ValueError, match="2\\^62"):
        _cp().partition(torch.tensor([1 << 61, 1 << 61], dtype=torch.int64))
    with pytest.raises(ValueError, match="int64"):
        _cp().partition(torch.tensor([1.0, 2.0]))
    with pytest.raises(ValueError, match="non-negative"):
        _cp().partition(torch.tensor([-1, 2], dtype=torch.int64))
    with pytest.raises(ValueError, match="\\[0, 1\\]"):
        _cp().partition(torch.tensor([1, 2], dtype=torch.int64), 1.5, 0.5)


# ---- the container, the file and the loader -------------------------------------------------------------------------------------
def _hand_made_container(dims=(5, 4, 3), F=12, K=9, store=np.float16, seed=0):
    CP = _cp()
    g = torch.Generator().manual_seed(seed)
    dens = torch.empty((*dims, 1)).uniform_(-3, 3, generator=g)
    feat = torch.empty((*dims, F)).uniform_(-2, 2, generator=g)
    imp = (torch.rand(dims, generator=g) * 2 ** 36).to(torch.int64) * (torch.rand(dims, generator=g) < 0.8)
    labels = CP.partition(imp, 0.05, 0.4)
    n_vq = int((labels == 1).sum())
    codebook = torch.empty((K, F)).uniform_(-2, 2, generator=g)
    index = torch.randint(0, K, (n_vq,), generator=g, dtype=torch.int32)
    return CP.build_container(labels, dens, feat, index, codebook, -10.0, store), labels, dens, feat, index, codebook


@pytest.mark.parametrize("store", [np.float16, np.float32])
def test_container_round_trip(store):
    CP = _cp()
    comp, labels, dens, feat, index, codebook = _hand_made_container(store=store)
    assert {0, 1, 2} == set(np.unique(labels.numpy()))
    back = CP.from_entry(CP.to_entry(comp))
    for name in CP.CompressedGrid.ARRAYS:
        a, b = getattr(comp, name), getattr(back, name)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), name
        assert np.array_equal(R.container_round_trip(a).view(np.uint8), a.view(np.uint8))
        entry = CP.to_entry(comp)[name]
        assert set(entry) == {"data", "dtype", "shape"} and isinstance(entry["data"], bytes)
    assert back.dims == comp.dims and back.empty_density == -10.0 and back.dtypes == ("float32", "float32")
    assert np.array_equal(back.labels(), labels.numpy()) and back.indices.dtype == np.uint16
    assert np.array_equal(back.indices, index.numpy()) and back.codebook.tobytes() == codebook.numpy().tobytes()
    d, f = CP.decompress(back)
    want_d, want_f = R.decompressed(labels.numpy(), dens.numpy(), feat.numpy(), index.numpy(), codebook.numpy(), -10.0, store)
    assert d.shape == dens.shape and f.shape == feat.shape and d.dtype == f.dtype == torch.float32
    assert np.array_equal(d.numpy().reshape(-1), want_d) and np.array_equal(f.numpy().reshape(want_f.shape), want_f)
    lab = labels.reshape(-1)
    flat_d, flat_f = d.reshape(-1), f.reshape(-1, feat.shape[-1])
    rt = (lambda t: t.half().float()) if store == np.float16 else (lambda t: t)
    assert torch.equal(flat_f[lab == 2], rt(feat.reshape(-1, feat.shape[-1])[lab == 2]))
    assert torch.equal(flat_d[lab != 0], rt(dens.reshape(-1)[lab != 0]))
    assert bool((flat_d[lab == 0] == -10.0).all()) and bool((flat_f[lab == 0] == 0).all())
    assert torch.equal(flat_f[lab == 1], codebook[index.long()])


def test_values_beyond_float16_are_refused():
    CP = _cp()
    labels = torch.full((2, 2, 2), 2, dtype=torch.uint8)
    dens, feat = torch.zeros((2, 2, 2, 1)), torch.zeros((2, 2, 2, 3))
    feat[1, 1, 1, 2] = 7e4
    none = torch.zeros((0,), dtype=torch.int32)
    with pytest.raises(ValueError, match="float16"):
        CP.build_container(labels, dens, feat, none, torch.zeros((0, 3)), 0.0, np.float16)
    assert CP.build_container(labels, dens, feat, none, torch.zeros((0, 3)), 0.0, np.float32).kept_features.max() == np.float32(7e4)
    with pytest.raises(ValueError, match="indices"):
        CP.build_container(labels, dens, feat, torch.zeros((1,), dtype=torch.int32), torch.zeros((1, 3)), 0.0, np.float32)


def _state_equal(a, b):
    return list(a) == list(b) and all(a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]) for k in a)


def test_loader_leaves_an_uncompressed_checkpoint_alone():
    from thre3d_atom.modules.volumetric_model import create_volumetric_model_from_saved_model
    from thre3d_atom.thre3d_reprs.constants import STATE_DICT, THRE3D_REPR
    from thre3d_atom.thre3d_reprs.voxels import create_voxel_grid_from_saved_info_dict

    CP = _cp()
    data = torch.load(CKPT, map_location="cpu", weights_only=False)
    again = torch.load(CKPT, map_location="cpu", weights_only=False)
    assert not CP.is_compressed(data) and CP.expand_checkpoint_(data) is False
    assert list(data) == list(again) and list(data[THRE3D_REPR]) == list(again[THRE3D_REPR])
    assert _state_equal(data[THRE3D_REPR][STATE_DICT], again[THRE3D_REPR][STATE_DICT])
    assert CP.load_uncompressed_checkpoint(CKPT).keys() == data.keys()
    model, _ = create_volumetric_model_from_saved_model(CKPT, create_voxel_grid_from_saved_info_dict)
    loaded = model.thre3d_repr.state_dict()
    assert _state_equal({k: v for k, v in loaded.items()}, {k: v for k, v in again[THRE3D_REPR][STATE_DICT].items()})
    with pytest.raises(ValueError, match="no compressed"):
        CP.load_compressed(CKPT)


def _compressed_copy_of_the_checkpoint(tmp_path):
    """the golden checkpoint with its grid replaced by a hand-made container of the same shape (no k-means: host only)"""
    from thre3d_atom.thre3d_reprs.constants import STATE_DICT, THRE3D_REPR, u_DENSITIES, u_FEATURES

    CP = _cp()
    data = torch.load(CKPT, map_location="cpu", weights_only=False)
    state = data[THRE3D_REPR][STATE_DICT]
    dens, feat = state[u_DENSITIES].clone(), state[u_FEATURES].clone()
    g = torch.Generator().manual_seed(1)
    imp = (torch.rand(dens.shape[:3], generator=g) * 2 ** 34).to(torch.int64) * (torch.rand(dens.shape[:3], generator=g) < 0.9)
    labels = CP.partition(imp, 0.02, 0.5)
    codebook = torch.empty((7, feat.shape[-1])).uniform_(-1, 1, generator=g)
    index = torch.randint(0, 7, (int((labels == 1).sum()),), generator=g, dtype=torch.int32)
    comp = CP.build_container(labels, dens, feat, index, codebook, -10.0, np.float16)
    path = tmp_path / "model_vq.pth"
    CP.save_compressed(path, data, comp)
    return path, comp, dens, feat


def test_compressed_file_keeps_every_other_entry_and_loads(tmp_path):
    from thre3d_atom.modules.volumetric_model import create_volumetric_model_from_saved_model
    from thre3d_atom.thre3d_reprs.constants import STATE_DICT, THRE3D_REPR, u_ATTN, u_DENSITIES, u_FEATURES
    from thre3d_atom.thre3d_reprs.voxels import create_voxel_grid_from_saved_info_dict

    CP = _cp()
    path, comp, dens, feat = _compressed_copy_of_the_checkpoint(tmp_path)
    orig = torch.load(CKPT, map_location="cpu", weights_only=False)
    data, back = CP.load_compressed(path)
    assert CP.is_compressed(data) and list(data) == list(orig)
    assert u_DENSITIES not in data[THRE3D_REPR][STATE_DICT] and u_FEATURES not in data[THRE3D_REPR][STATE_DICT]
    for key in orig:
        if key != THRE3D_REPR:
            assert repr(data[key]) == repr(orig[key]), key
    assert [k for k in data[THRE3D_REPR] if k != CP.COMPRESSED] == list(orig[THRE3D_REPR])
    assert back.indices.tobytes() == comp.indices.tobytes() and back.codebook.tobytes() == comp.codebook.tobytes()
    want_d, want_f = CP.decompress(comp)
    model, extra = create_volumetric_model_from_saved_model(path, create_voxel_grid_from_saved_info_dict)
    assert torch.equal(model.thre3d_repr.densities.detach(), want_d) and torch.equal(model.thre3d_repr.features.detach(), want_f)
    assert model.thre3d_repr.densities.dtype == dens.dtype and extra is not None
    # the decompression tool writes an ordinary checkpoint with the same tensors
    from click.testing import CliRunner

    out = tmp_path / "plain.pth"
    tool = _load_cli("decompress_voxel_grid.py")
    res = CliRunner().invoke(tool.main, ["-i", str(path), "-o", str(out)])
    assert res.exit_code == 0, (res.output, res.exception)
    plain = torch.load(out, map_location="cpu", weights_only=False)
    assert not CP.is_compressed(plain) and list(plain[THRE3D_REPR]) == list(orig[THRE3D_REPR])
    assert torch.equal(plain[THRE3D_REPR][STATE_DICT][u_DENSITIES], want_d)
    assert torch.equal(plain[THRE3D_REPR][STATE_DICT][u_FEATURES], want_f)
    res = CliRunner().invoke(tool.main, ["-i", str(out), "-o", str(tmp_path / "twice.pth")])
    assert res.exit_code != 0 and "nothing to decompress" in res.output
    # attention parameters are refused with a clear message
    with_attn = torch.load(CKPT, map_location="cpu", weights_only=False)
    with_attn[THRE3D_REPR][STATE_DICT][u_ATTN] = torch.zeros_like(dens)
    with pytest.raises(ValueError, match="attention"):
        CP.compress_checkpoint_(with_attn, comp)
    assert u_DENSITIES in with_attn[THRE3D_REPR][STATE_DICT]


def _load_cli(name):
    spec = importlib.util.spec_from_file_location(name[:-3] + "_vq_cli", os.path.join(ROOT, name))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("script,args", [("prune_voxel_grid.py", []), ("transform_voxel_grid.py", ["--quarter_turns", "z", "1"]),
                                         ("export_mesh.py", [])])
def test_tools_that_rewrite_the_file_name_the_decompression_tool(tmp_path, script, args):
    from click.testing import CliRunner

    path, *_ = _compressed_copy_of_the_checkpoint(tmp_path)
    mod = _load_cli(script)
    res = CliRunner().invoke(mod.main, ["-i", str(path), "-o", str(tmp_path / "out.pth")] + args)
    assert res.exit_code != 0
    assert isinstance(res.exception, ValueError) and not isinstance(res.exception, KeyError), (res.output, res.exception)
    assert "decompress_voxel_grid.py" in str(res.exception) and str(path) in str(res.exception)
    assert not (tmp_path / "out.pth").exists()


def test_compress_command_line_declares_the_issue_options():
    mod = _load_cli("compress_voxel_grid.py")
    opts = {o for p in mod.main.params for o in p.opts}
    assert {"-i", "-o", "-d", "--num_views", "--prune_share", "--keep_share", "--codebook_size", "--kmeans_iterations",
            "--store_dtype", "--seed", "--overridden_num_samples_per_ray", "--evaluate"} <= opts
    by_name = {p.name: p for p in mod.main.params}
    CP = _cp()
    assert (by_name["prune_share"].default, by_name["keep_share"].default, by_name["codebook_size"].default) == (1e-3, 0.6, 4096)
    assert by_name["kmeans_iterations"].default == CP.DEFAULT_ITERATIONS and by_name["store_dtype"].default == "float16"


# ---- the binding ----------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_built_and_validate_before_any_device_work():
    from voxe_hip import build
    from voxe_hip.runtime import LIB_PATH

    text = open(os.path.join(ROOT, "include", "voxe.h")).read()
    for name in ("voxe_vq_assign", "voxe_vq_accumulate", "voxe_vq_debug_merge"):
        assert re.search(rf"\b{name}\s*\(", text) and name in abi.hip_symbols()
    assert "voxe_vq.hip" in build.SOURCES
    assert len(abi.HIP_ONLY["vq_assign"][1]) == 9 and len(abi.HIP_ONLY["vq_accumulate"][1]) == 9
    L = abi.declare(ctypes.CDLL(build.build() if not os.path.exists(LIB_PATH) else LIB_PATH), "voxe_")
    p = 8   # (never dereferenced: every call below is answered before a launch)
    assert L.voxe_vq_assign(None, 0, 3, None, 4, None, None, None, None) == abi.OK
    assert L.voxe_vq_accumulate(None, None, None, 0, 3, 4, None, None, None) == abi.OK
    for N, F, K in ((-1, 3, 4), (1 << 31, 3, 4), (5, 0, 4), (5, 65, 4), (5, 3, 0), (5, 3, 65537), (0, 65, 4), (0, 3, 0)):
        assert L.voxe_vq_assign(p, N, F, p, K, p, p, p, None) == abi.ERR_BAD_SHAPE, (N, F, K)
        assert L.voxe_vq_accumulate(p, p, p, N, F, K, p, p, None) == abi.ERR_BAD_SHAPE, (N, F, K)
    for hole in range(4):
        args = [p, 5, 3, p, 4, p, p, None, None]
        args[(0, 3, 5, 6)[hole]] = None
        assert L.voxe_vq_assign(*args) == abi.ERR_NULL_POINTER, hole
    for hole in (0, 1, 2, 6, 7):
        args = [p, p, p, 5, 3, 4, p, p, None]
        args[hole] = None
        assert L.voxe_vq_accumulate(*args) == abi.ERR_NULL_POINTER, hole
    for mode in (1, 2, 0):
        assert L.voxe_vq_debug_merge(mode) == abi.OK
    assert L.voxe_vq_debug_merge(3) == abi.ERR_BAD_SHAPE and L.voxe_vq_debug_merge(-1) == abi.ERR_BAD_SHAPE


def test_wrappers_refuse_host_tensors_and_wrong_buffers():
    from voxe_hip import ops
    from voxe_hip.runtime import VoxeError

    x, c = torch.zeros((4, 3)), torch.zeros((2, 3))
    with pytest.raises(VoxeError):
        ops.vq_assign_(x, c)
    with pytest.raises(VoxeError):
        ops.vq_accumulate_(x, torch.zeros(4), torch.zeros(4, dtype=torch.int32), torch.zeros((2, 3), dtype=torch.int64),
                           torch.zeros(2, dtype=torch.int64))


# ---- the restatements themselves, and the non-vacuity of the GPU assign test ------------------------------------------------------
def test_fixed_point_restatement_by_hand():
    x = np.array([[0.5, -0.25], [1.0, 0.0], [2.0 ** -34, -1.0], [0.75, 0.75]], np.float32)
    w = np.array([1.0, 0.5, 1.0, 0.0], np.float32)
    sum_wx, sum_w = R.accumulate(x, w, [1, 1, 0, 0], 3)
    one = 1 << 32
    assert sum_w.tolist() == [one, one + one // 2, 0]
    assert sum_wx.tolist() == [[0, -one], [one // 2 + one // 2, -(one // 4)], [0, 0]]     # 2^-34 quantises to 0
    new = R.lloyd_step(x, w, np.full((3, 2), 9.0, np.float32), [1, 1, 0, 0])
    assert new.tolist() == [[0.0, -1.0], [np.float32(2 / 3), np.float32(-1 / 6)], [9.0, 9.0]]     # an empty cluster keeps its codeword
    assert R.dist32([[1.0, 2.0]], [[0.0, 0.0], [1.0, 2.0]], [1]).tolist() == [0.0]
    assert R.dist32([[1.0, 2.0]], [[0.0, 0.5]], [0]).tolist() == [3.25]


def test_the_gpu_assign_test_is_not_vacuous():
    """per case: the float32 restatement is inside the slack everywhere and differs from the float64 arg-min on <= 1 % of the
    points; over the cases where the defect can show (K > 1; odd F > 1 for the dropped channel), an assignment without |c_k|^2
    breaks the slack on more than 20 % of the points of every such case and one without the last channel on more than 5 %"""
    worst, shares_norm, shares_last = 0.0, [], []
    for N, K, F in R.assign_shapes():
        x, c, _ = R.assign_case(N, K, F)
        s = R.slack(x, c)
        idx = R.argmin32(x, c)
        ratio = R.gap(x, c, idx) / s
        worst = max(worst, float(ratio.max()))
        assert float(ratio.max()) <= 1.0, (N, K, F, float(ratio.max()))
        assert int((idx != R.argmin64(x, c)).sum()) <= int(R.MAX_MISMATCH_SHARE * N), (N, K, F)
        if K >= 31 and N >= 31:
            x64, c64 = x.astype(np.float64), c.astype(np.float64)
            shares_norm.append(float((R.gap(x, c, (-2.0 * x64 @ c64.T).argmin(1)) > s).mean()))
            if F in (3, 27):
                cut = ((c64[:, :-1] ** 2).sum(1)[None, :] - 2.0 * x64[:, :-1] @ c64[:, :-1].T).argmin(1)
                shares_last.append(float((R.gap(x, c, cut) > s).mean()))
    print(f"float32 restatement: worst gap / slack {worst:.3f}; without |c|^2: violation shares {min(shares_norm):.2f} .. "
          f"{max(shares_norm):.2f}; without the last channel: {min(shares_last):.2f} .. {max(shares_last):.2f}")
    assert min(shares_norm) > 0.20 and min(shares_last) > 0.05
