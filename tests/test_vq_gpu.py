"""GPU checks of the vector quantisation (voxe_vq_assign / voxe_vq_accumulate, voxe_vq.hip), of the k-means on top of it and of
the checkpoint compression end to end (thre3d_reprs/compression.py, compress_voxel_grid.py, decompress_voxel_grid.py) against
the numpy restatements of tests/vq_ref.py.  tests/test_vq_host.py shows on the CPU that the assign check is not vacuous."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import vq_ref as R
from conftest import ROOT
from voxe_hip import ops, workload

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _assign(x, c, with_dist=True):
    dist = torch.empty(len(x), dtype=torch.float32, device=DEV) if with_dist else None
    index, dist = ops.vq_assign_(t(x), t(c), dist=dist)
    return index.cpu().numpy(), None if dist is None else dist.cpu().numpy()


def _accumulate(x, w, index, K, mode=ops.VQ_MERGE_SHIPPED, pieces=1):
    sum_wx = torch.zeros((K, x.shape[1]), dtype=torch.int64, device=DEV)
    sum_w = torch.zeros((K,), dtype=torch.int64, device=DEV)
    ops.vq_debug_merge(mode)
    try:
        for part in np.array_split(np.arange(len(x)), pieces):
            ops.vq_accumulate_(t(x[part]), t(w[part]), t(index[part].astype(np.int32)), sum_wx, sum_w)
    finally:
        ops.vq_debug_merge(ops.VQ_MERGE_SHIPPED)
    return sum_wx.cpu().numpy(), sum_w.cpu().numpy()


# ---- assign ---------------------------------------------------------------------------------------------------------------------
def test_assign_is_within_the_slack_on_every_shape():
    """For every point of every shape of vq_ref.assign_shapes (N x K x F, 216 cases):
        d64(x_n, c_index[n]) - min_k d64(x_n, c_k) <= slack_n = 4 * 2^-24 * (F + 2) * (|x_n| + max_k |c_k|)^2
    (the forward error bound of two (F + 1)-term float32 sums, times two: derived, not measured), index in range, at most 1 % of a
    case's indices differ from the float64 arg-min, and dist is bit-equal to the numpy float32 formula for the returned index.
    Worst observed gap / slack on an MI355X: 0.0 over all cases (every index equalled the float64 arg-min; the float32
    restatement on the host reaches 0.0005 at most); profiles/vq_pytest_gpu.log holds the run."""
    worst, differ = 0.0, 0
    for N, K, F in R.assign_shapes():
        x, c, _ = R.assign_case(N, K, F)
        index, dist = _assign(x, c)
        assert index.dtype == np.int32 and index.min() >= 0 and index.max() < K, (N, K, F)
        ratio = R.gap(x, c, index) / R.slack(x, c)
        worst = max(worst, float(ratio.max()))
        assert float(ratio.max()) <= 1.0, (N, K, F, float(ratio.max()))
        wrong = int((index != R.argmin64(x, c)).sum())
        differ += wrong
        assert wrong <= int(R.MAX_MISMATCH_SHARE * N), (N, K, F, wrong)
        assert np.array_equal(dist, R.dist32(x, c, index)), (N, K, F)
        if K == 1:
            assert not index.any()
    print(f"assign: worst gap / slack {worst:.3e} over {len(R.assign_shapes())} cases, {differ} indices differ from the float64 arg-min")


@pytest.mark.parametrize("N,K,F", [(257, 33, 27), (1000, 129, 3), (64, 300, 48)])
def test_assign_ties_duplicates_permutations_and_repeats(N, K, F):
    x, c, _ = R.assign_case(N, K, F)
    s = R.slack(x, c)
    index, dist = _assign(x, c)
    # the first copy of a duplicated codeword wins: bit-equal scores, lowest k
    twice, _ = _assign(x, np.concatenate([c, c]))
    assert twice.max() < K and np.array_equal(twice, index)
    # codebook rows permuted: the distances are unchanged within the slack
    perm = np.random.default_rng(K).permutation(K)
    pidx, pdist = _assign(x, c[perm])
    d = R.dist64(x, c)
    assert (np.abs(d[np.arange(N), perm[pidx]] - d[np.arange(N), index]) <= s).all()
    assert np.array_equal(pdist, R.dist32(x, c[perm], pidx))
    # two calls return the same bits, with and without dist
    again, adist = _assign(x, c)
    nodist, none = _assign(x, c, with_dist=False)
    assert np.array_equal(again, index) and np.array_equal(adist.view(np.int32), dist.view(np.int32))
    assert np.array_equal(nodist, index) and none is None
    # points that ARE codewords: dist == 0, or within the slack where another codeword scores as low
    own = np.random.default_rng(N).integers(0, K, N)
    oidx, odist = _assign(c[own], c)
    so = R.slack(c[own], c)
    assert ((odist == 0) | (odist <= so)).all() and (R.gap(c[own], c, oidx) <= so).all()
    assert (odist[oidx == own] == 0).all() and (oidx == own).mean() > 0.98


def test_assign_subnormal_and_large_coordinates_stay_finite():
    rng = np.random.default_rng(11)
    for scale in (1e18, 1e-40):
        x = (rng.uniform(-1, 1, (257, 3)) * scale).astype(np.float32)
        c = (rng.uniform(-1, 1, (33, 3)) * scale).astype(np.float32)
        index, dist = _assign(x, c)
        assert index.min() >= 0 and index.max() < 33 and np.isfinite(dist).all()
        assert np.array_equal(dist, R.dist32(x, c, index))
        if scale > 1:
            assert (R.gap(x, c, index) <= R.slack(x, c)).all() and (index != index[0]).any()


# ---- accumulate -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,F", [(1, 1, 1), (33, 2, 3), (257, 31, 12), (1000, 300, 27), (1000, 33, 64), (64, 129, 48)])
def test_accumulate_equals_the_integer_restatement_in_any_order(N, K, F):
    rng = np.random.default_rng([N, K, F])
    x = rng.uniform(-1, 1, (N, F)).astype(np.float32)
    w = rng.uniform(0, 1, N).astype(np.float32)
    w[::7] = 0.0                      # weights 0 and 1
    w[3::7] = 1.0
    w[5::11] = np.float32(2.0 ** -34)    # contributions that quantise to 0
    x[2::13] = np.float32(2.0 ** -33)
    index = rng.integers(0, K, N)
    want = R.accumulate(x, w, index, K)
    shuffled, by_index = rng.permutation(N), np.argsort(index, kind="stable")
    for mode in (ops.VQ_MERGE_SHIPPED, ops.VQ_MERGE_PER_LANE, ops.VQ_MERGE_RUNS):
        for order in (np.arange(N), shuffled, by_index):
            got = _accumulate(x[order], w[order], index[order], K, mode)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (mode, order[:4])
        got = _accumulate(x[by_index], w[by_index], index[by_index], K, mode, pieces=2)      # the call split into two launches
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), mode
        one = np.full(N, K - 1)                                                          # all points on one codeword
        got, ref = _accumulate(x, w, one, K, mode), R.accumulate(x, w, one, K)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and not got[1][:-1].any()
    assert (R.quantise(w[5::11]) == 0).all() and int(want[1].sum()) == int(R.quantise(w).sum())


# ---- Lloyd ----------------------------------------------------------------------------------------------------------------------
def _lloyd(x, w, codebook, iterations):
    from thre3d_atom.thre3d_reprs.compression import lloyd_update

    xd, wd, cb = t(x), t(w), t(codebook)
    K, F = codebook.shape
    for _ in range(iterations):
        index, _ = ops.vq_assign_(xd, cb)
        sum_wx, sum_w = torch.zeros((K, F), dtype=torch.int64, device=DEV), torch.zeros(K, dtype=torch.int64, device=DEV)
        ops.vq_accumulate_(xd, wd, index, sum_wx, sum_w)
        want = R.lloyd_step(x, w, cb.cpu().numpy(), index.cpu().numpy())
        cb = lloyd_update(cb, sum_wx, sum_w).contiguous()
        assert np.array_equal(cb.cpu().numpy().view(np.int32), want.view(np.int32))
    index, _ = ops.vq_assign_(xd, cb)
    return cb.cpu().numpy(), index.cpu().numpy()


def test_lloyd_recovers_separated_clusters_and_keeps_an_empty_codeword():
    rng = np.random.default_rng(5)
    K, F, per, sigma = 17, 12, 59, 0.004
    centres = rng.uniform(-0.9, 0.9, (K, F))
    gaps = np.linalg.norm(centres[:, None] - centres[None], axis=-1) + 1e9 * np.eye(K)
    assert gaps.min() >= 20 * sigma * np.sqrt(F)       # separation >= 20 sigma of the cluster radius
    labels = np.repeat(np.arange(K), per)
    x = np.clip(centres[labels] + sigma * rng.standard_normal((K * per, F)), -1, 1).astype(np.float32)
    w = rng.uniform(0.05, 1, K * per).astype(np.float32)
    order = rng.permutation(K * per)
    x, w, labels = x[order], w[order], labels[order]
    first = np.array([np.flatnonzero(labels == k)[0] for k in range(K)])
    far = np.full((1, F), 0.99, np.float32)               # a codeword no point chooses: it must keep its value
    codebook, index = _lloyd(x, w, np.concatenate([x[first], far]), 3)
    assert np.array_equal(index, labels)
    assert np.array_equal(codebook[K], far[0])
    means = np.stack([(w[labels == k, None].astype(np.float64) * x[labels == k]).sum(0) / w[labels == k].astype(np.float64).sum()
                      for k in range(K)])
    err = float(np.abs(codebook[:K] - means).max())
    print(f"centroids: max |kernel - float64 weighted mean| {err:.3e} (bound {1e-6 * float(np.abs(x).max()):.1e})")
    assert err <= 1e-6 * float(np.abs(x).max())


def test_train_codebook_descends_and_is_reproducible():
    from thre3d_atom.thre3d_reprs.compression import train_codebook

    rng = np.random.default_rng(9)
    N, F, K = 3000, 27, 100
    x = (rng.standard_normal((N, F)) * rng.uniform(0.2, 3, F)).astype(np.float32)
    w = rng.uniform(0, 5, N).astype(np.float32)
    codebook, index, curve = train_codebook(t(x), t(w), K, 6, seed=3)
    assert codebook.shape == (K, F) and index.shape == (N,) and index.dtype == torch.int32 and len(curve) == 7
    xn = x / np.float32(np.abs(x).max())
    wn = w / np.float32(w.max())
    norms = np.linalg.norm(xn.astype(np.float64), axis=1)
    # codewords are initial rows or weighted means of rows: no longer than the longest row
    slack = 4.0 * R.EPS * (F + 2) * (norms + norms.max()) ** 2
    allowed = float((wn.astype(np.float64) * slack).sum())
    print("distortion per iteration: " + " ".join(f"{v:.6e}" for v in curve) + f"   allowed rise {allowed:.2e}")
    assert all(b <= a + allowed for a, b in zip(curve, curve[1:])) and curve[-1] < curve[0]
    # the returned index and distortion are those of the returned codebook
    cb = codebook.cpu().numpy() / np.float32(np.abs(x).max())
    got = index.cpu().numpy()
    assert (R.gap(xn, cb, got) <= R.slack(xn, cb) + 1e-6).all()
    again = train_codebook(t(x), t(w), K, 6, seed=3)
    assert torch.equal(again[0], codebook) and torch.equal(again[1], index) and again[2] == curve
    other = train_codebook(t(x), t(w), K, 6, seed=4)
    assert not torch.equal(other[0], codebook)
    # N <= K: every row is its own codeword
    small, sidx, scurve = train_codebook(t(x[:40]), t(w[:40]), K, 2, seed=0)
    assert small.shape == (40, F) and np.array_equal(sidx.cpu().numpy(), np.arange(40)) and scurve[0] == 0.0 and max(scurve) < 1e-10
    assert float((small.cpu() - torch.from_numpy(x[:40])).abs().max()) <= 2.0 ** -22 * float(np.abs(x[:40]).max())


# ---- end to end -----------------------------------------------------------------------------------------------------------------
SIDE, HW, VIEWS, CODES = 24, 48, 4, 64


def _model():
    from thre3d_atom.modules.volumetric_model import VolumetricModel
    from thre3d_atom.thre3d_reprs.renderers import SHVoxGridRenderConfig, render_sh_voxel_grid
    from thre3d_atom.thre3d_reprs.voxels import VoxelGrid, VoxelSize
    from thre3d_atom.utils.constants import CAMERA_BOUNDS, CAMERA_INTRINSICS, HEMISPHERICAL_RADIUS
    from thre3d_atom.utils.imaging_utils import CameraBounds, CameraIntrinsics

    dens, _ = workload.sphere_grid(SIDE)
    _, feat = workload.random_grid(SIDE, nfeat=12, seed=7)                     # SH degree 1
    grid = VoxelGrid((2.0 * dens).to(DEV), feat.to(DEV), VoxelSize(*(3.0 / SIDE,) * 3), density_preactivation=torch.nn.Identity(),
                     density_postactivation=torch.nn.Softplus(), expected_density_scale=4.0, tunable=True)
    bounds = CameraBounds(workload.NEAR, workload.FAR)
    model = VolumetricModel(grid, render_sh_voxel_grid, SHVoxGridRenderConfig(48, bounds), device=DEV)
    extra = {CAMERA_BOUNDS: bounds, CAMERA_INTRINSICS: CameraIntrinsics(HW, HW, workload.focal_for(HW)),
             HEMISPHERICAL_RADIUS: workload.RADIUS}
    return model, extra


def _load_cli(name):
    spec = importlib.util.spec_from_file_location(name[:-3] + "_vq_gpu_cli", os.path.join(ROOT, name))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _load_model(path):
    from thre3d_atom.modules.volumetric_model import create_volumetric_model_from_saved_model
    from thre3d_atom.thre3d_reprs.voxels import create_voxel_grid_from_saved_info_dict

    return create_volumetric_model_from_saved_model(path, create_voxel_grid_from_saved_info_dict, device=DEV)


def test_compression_end_to_end(tmp_path):
    from click.testing import CliRunner

    from thre3d_atom.thre3d_reprs import compression as CP
    from thre3d_atom.thre3d_reprs.lifting import lift_images
    from thre3d_atom.thre3d_reprs.visibility import prune_voxel_grid_, visibility_cameras

    model, extra = _model()
    grid = model.thre3d_repr
    poses, intr = visibility_cameras(extra, None, VIEWS + 1)      # (the 360 degree path leaves its closing frame out)
    assert len(poses) == VIEWS
    importance = CP.voxel_importance(model, poses, intr)
    lifted = lift_images(model, poses, intr, torch.zeros((VIEWS, 1, HW, HW)))
    assert importance.dtype == torch.int64 and torch.equal(importance, lifted.sum_w) and int(importance.max()) > 0
    comp = CP.compress(model, importance, codebook_size=CODES, iterations=4)
    labels = comp.labels()
    assert np.array_equal(labels, R.partition(importance.cpu().numpy(), 1e-3, 0.6))
    counts = [int((labels == v).sum()) for v in (0, 1, 2)]
    assert min(counts) > CODES and comp.codebook.shape == (CODES, 12) and comp.indices.dtype == np.uint16
    assert len(comp.distortion) == 5 and comp.distortion[-1] < comp.distortion[0]
    dens0, feat0 = grid.densities.detach().cpu(), grid.features.detach().cpu()
    dens, feat = CP.decompress(comp)
    want_d, want_f = R.decompressed(labels, dens0.numpy(), feat0.numpy(), comp.indices, comp.codebook, -20.0 / 4.0)
    assert np.array_equal(dens.numpy().reshape(-1), want_d) and np.array_equal(feat.numpy().reshape(-1, 12), want_f)
    lab = torch.from_numpy(labels.reshape(-1))
    flat_f = feat.reshape(-1, 12)
    assert torch.equal(flat_f[lab == 2], feat0.reshape(-1, 12)[lab == 2].half().float())
    assert torch.equal(flat_f[lab == 1], torch.from_numpy(comp.codebook)[torch.from_numpy(comp.indices.astype(np.int64))])
    assert bool((flat_f[lab == 0] == 0).all())
    # pruned voxels hold what prune_voxel_grid_ writes
    torch.save(model.get_save_info(extra), tmp_path / "model.pth")
    pruned, _ = _load_model(tmp_path / "model.pth")
    prune_voxel_grid_(pruned.thre3d_repr, torch.from_numpy(labels != 0).to(DEV))
    assert torch.equal(dens.reshape(-1)[lab == 0], pruned.thre3d_repr.densities.detach().cpu().reshape(-1)[lab == 0])
    # the index of every VQ voxel is the kernel's choice for the stored codebook (normalised as train_codebook does)
    vq_feat = feat0.reshape(-1, 12)[lab == 1].numpy()
    scale = np.float32(np.abs(vq_feat).max())
    assert (R.gap(vq_feat / scale, comp.codebook / scale, comp.indices) <= R.slack(vq_feat / scale, comp.codebook / scale) + 1e-6).all()

    # the command lines
    tool, back = _load_cli("compress_voxel_grid.py"), _load_cli("decompress_voxel_grid.py")
    res = CliRunner().invoke(tool.main, ["-i", str(tmp_path / "model.pth"), "-o", str(tmp_path / "model_vq.pth"), "--num_views", str(VIEWS + 1),
                                         "--codebook_size", str(CODES), "--kmeans_iterations", "4", "--evaluate"])
    assert res.exit_code == 0, (res.output, res.exception)
    print(res.output)
    got = [int(v) for v in re.search(r"pruned (\d+)\s+vector-quantised (\d+)\s+kept (\d+)", res.output).groups()]
    assert got == counts and "distortion per iteration" in res.output and "k-means" in res.output
    assert float(re.search(r"PSNR .* mean ([\d.]+|inf) dB", res.output).group(1)) > 0.0
    small, big = os.path.getsize(tmp_path / "model_vq.pth"), os.path.getsize(tmp_path / "model.pth")
    assert small < big / 2, (small, big)
    _, from_file = CP.load_compressed(tmp_path / "model_vq.pth")
    for name in CP.CompressedGrid.ARRAYS:
        assert getattr(from_file, name).tobytes() == getattr(comp, name).tobytes(), name
    res = CliRunner().invoke(back.main, ["-i", str(tmp_path / "model_vq.pth"), "-o", str(tmp_path / "plain.pth")])
    assert res.exit_code == 0, (res.output, res.exception)
    a, extra_a = _load_model(tmp_path / "model_vq.pth")
    b, _ = _load_model(tmp_path / "plain.pth")
    assert torch.equal(a.thre3d_repr.densities, b.thre3d_repr.densities) and torch.equal(a.thre3d_repr.features, b.thre3d_repr.features)
    assert torch.equal(a.thre3d_repr.features.detach().cpu(), feat) and set(extra_a) == set(extra)
    kw = dict(perturb_sampled_points=False)
    ra, rb, r0 = (m.render(poses[1], intr, **kw) for m in (a, b, model))
    assert torch.equal(ra.colour, rb.colour) and torch.equal(ra.depth, rb.depth)
    assert ra.colour.shape == r0.colour.shape and float(r0.colour.max()) > 0.1
    # a compressed file is refused by the compressor itself, by name of the way back
    res = CliRunner().invoke(tool.main, ["-i", str(tmp_path / "model_vq.pth"), "-o", str(tmp_path / "twice.pth")])
    assert res.exit_code != 0 and "decompress_voxel_grid.py" in str(res.exception)
