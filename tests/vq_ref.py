"""Numpy restatements of the vector quantisation and of the checkpoint compression (voxe_vq.hip, thre3d_reprs/compression.py):
what tests/test_vq_host.py and tests/test_vq_gpu.py hold the product to."""
import zlib

import numpy as np

ONE = 1 << 32
EPS = 2.0 ** -24


# ---- the cases the GPU assign test runs (and the host test proves non-vacuous) ---------------------------------------------------
# the whole cross product N x K x F: a wave's 64 points and a block's 256 on both sides, the 64-codeword LDS tile of the shipped
# kernel on both sides (K = 129 and 300 span several tiles, ragged last ones), every k-step bucket of the channel count, odd F
ASSIGN_N = (1, 31, 33, 64, 257, 1000)
ASSIGN_K = (1, 2, 31, 33, 129, 300)
ASSIGN_F = (1, 3, 12, 27, 48, 64)
MAX_MISMATCH_SHARE = 0.01


def assign_shapes():
    return [(N, K, F) for N in ASSIGN_N for K in ASSIGN_K for F in ASSIGN_F]


_CASES = {}


def assign_case(N, K, F):
    """(points, codebook, seed) ~ U(-1, 1), float32.  The seed is the first one for which at most 1 % of the points are
    NEAR TIES -- their two nearest codewords closer to each other (in float64 squared distance) than 1/64 of the point's slack,
    which is where float32 rounding of the score can move the arg-min -- and for which the float32 restatement of the score
    differs from the float64 arg-min on at most 1 % of the points.  The seeds are chosen from the references alone."""
    if (N, K, F) not in _CASES:
        for seed in range(100):
            rng = np.random.default_rng([N, K, F, seed])
            x, c = rng.uniform(-1, 1, (N, F)).astype(np.float32), rng.uniform(-1, 1, (K, F)).astype(np.float32)
            allowed = int(MAX_MISMATCH_SHARE * N)
            if near_ties(x, c).sum() <= allowed and (argmin32(x, c) != argmin64(x, c)).sum() <= allowed:
                _CASES[(N, K, F)] = (x, c, seed)
                break
        else:
            raise AssertionError(f"no seed below 100 for {(N, K, F)}")
    return _CASES[(N, K, F)]


def dist64(x, c):
    """[N,K] float64 squared distances (expanded, in float64: its own error is 1e-9 of the slack)"""
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    return np.maximum((x * x).sum(1)[:, None] + (c * c).sum(1)[None, :] - 2.0 * (x @ c.T), 0.0)


def near_ties(x, c):
    """[N] bool: the second nearest codeword is within slack / 64 of the nearest"""
    d = dist64(x, c)
    if d.shape[1] < 2:
        return np.zeros(len(d), bool)
    two = np.partition(d, 1, axis=1)[:, :2]
    return (two[:, 1] - two[:, 0]) <= slack(x, c) / 64.0


def argmin64(x, c):
    return dist64(x, c).argmin(1)


def slack(x, c):
    """[N]: 4 * 2^-24 * (F + 2) * (|x_n| + max_k |c_k|)^2 -- the forward error bound of two (F + 1)-term float32 sums, times two"""
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    F = x.shape[1]
    return 4.0 * EPS * (F + 2) * (np.linalg.norm(x, axis=1) + np.linalg.norm(c, axis=1).max()) ** 2


def gap(x, c, index):
    """[N]: d64(x_n, c_index[n]) - min_k d64(x_n, c_k)"""
    d = dist64(x, c)
    return d[np.arange(len(x)), np.asarray(index, np.int64)] - d.min(1)


def code_norm32(c):
    """[K] float32: plain ascending sum of the rounded squares"""
    c = np.asarray(c, np.float32)
    s = np.zeros(len(c), np.float32)
    for j in range(c.shape[1]):
        s = (s + (c[:, j] * c[:, j]).astype(np.float32)).astype(np.float32)
    return s


def scores32(x, c, use_norm=True, channels=None):
    """[N,K] float32 restatement of the kernel's score: s = |c|^2, then s = fma(-2 c_j, x_j, s) over ascending j (the fused
    multiply-add through float64: the product of two float32 is exact there, the sum is rounded once to float64 and once more to
    float32 -- a double rounding the slack has room for).  use_norm=False drops |c|^2, channels=m uses channels 0..m-1 only: the
    two broken assignments of the non-vacuity checks."""
    x, c = np.asarray(x, np.float32), np.asarray(c, np.float32)
    F = x.shape[1] if channels is None else channels
    s = np.tile(code_norm32(c[:, :F]) if use_norm else np.zeros(len(c), np.float32), (len(x), 1))
    for j in range(F):
        prod = (-2.0 * c[None, :, j].astype(np.float64)) * x[:, None, j].astype(np.float64)
        s = (prod + s.astype(np.float64)).astype(np.float32)
    return s


def argmin32(x, c, **kw):
    return scores32(x, c, **kw).argmin(1)      # (numpy: the first of equal minima, as the kernel)


def dist32(x, c, index):
    """[N] float32: d = 0; for ascending j: u = x_j - c_j; d = d + u * u, every operation rounded to float32"""
    x, c = np.asarray(x, np.float32), np.asarray(c, np.float32)[np.asarray(index, np.int64)]
    d = np.zeros(len(x), np.float32)
    for j in range(x.shape[1]):
        u = (x[:, j] - c[:, j]).astype(np.float32)
        d = (d + (u * u).astype(np.float32)).astype(np.float32)
    return d


# ---- the fixed-point sums -------------------------------------------------------------------------------------------------------
def quantise(v):
    """(int64) rint(v * 2^32) of float32 values (the scaling is exact; numpy rounds half to even)"""
    return np.rint(np.asarray(v, np.float32).astype(np.float64) * float(ONE)).astype(np.int64)


def accumulate(x, w, index, K):
    """(sum_wx [K,F] int64, sum_w [K] int64); the product w * x is rounded to float32 first; zero contributions add nothing"""
    x, w, index = np.asarray(x, np.float32), np.asarray(w, np.float32), np.asarray(index, np.int64)
    sum_wx, sum_w = np.zeros((K, x.shape[1]), np.int64), np.zeros(K, np.int64)
    np.add.at(sum_w, index, quantise(w))
    np.add.at(sum_wx, index, quantise((w[:, None] * x).astype(np.float32)))
    return sum_wx, sum_w


def lloyd_step(x, w, codebook, index):
    """the codebook after one step given the assignment: float32(sum_wx / sum_w) divided in float64; empty clusters keep theirs"""
    sum_wx, sum_w = accumulate(x, w, index, len(codebook))
    new = np.array(codebook, np.float32, copy=True)
    hit = sum_w != 0
    new[hit] = (sum_wx[hit].astype(np.float64) / sum_w[hit].astype(np.float64)[:, None]).astype(np.float32)
    return new


# ---- partition ------------------------------------------------------------------------------------------------------------------
def thresholds(total, prune_share, keep_share):
    return int(keep_share * float(total)), int((1.0 - prune_share) * float(total))


def partition(importance, prune_share, keep_share):
    """uint8 labels (0 pruned, 1 VQ, 2 kept) by numpy int64 prefix sums over (importance descending, linear index ascending)"""
    imp = np.asarray(importance, np.int64)
    flat = imp.reshape(-1)
    total = int(sum(int(v) for v in flat))
    assert total < 1 << 62
    t_keep, t_prune = thresholds(total, prune_share, keep_share)
    order = np.lexsort((np.arange(flat.size), -flat))
    ordered = flat[order]
    before = np.cumsum(ordered) - ordered
    lab = np.full(flat.size, 1, np.uint8)
    lab[before < t_keep] = 2
    lab[(ordered == 0) | (before >= t_prune)] = 0
    out = np.empty_like(lab)
    out[order] = lab
    return out.reshape(imp.shape)


def partition_loop(importance, prune_share, keep_share):
    """the same by a brute-force python loop over python ints"""
    flat = [int(v) for v in np.asarray(importance).reshape(-1)]
    total = sum(flat)
    t_keep, t_prune = thresholds(total, prune_share, keep_share)
    order = sorted(range(len(flat)), key=lambda i: (-flat[i], i))
    labels, before = [1] * len(flat), 0
    for i in order:
        if flat[i] == 0 or before >= t_prune:
            labels[i] = 0
        elif before < t_keep:
            labels[i] = 2
        before += flat[i]
    return np.array(labels, np.uint8).reshape(np.asarray(importance).shape)


# ---- the container --------------------------------------------------------------------------------------------------------------
def container_round_trip(arr):
    """an array through the file format's (deflated bytes, dtype, shape) triple"""
    arr = np.ascontiguousarray(arr)
    entry = {"data": zlib.compress(arr.tobytes(), 9), "dtype": str(arr.dtype), "shape": arr.shape}
    return np.frombuffer(zlib.decompress(entry["data"]), dtype=np.dtype(entry["dtype"])).reshape(entry["shape"])


def decompressed(labels, densities, features, index, codebook, empty, store=np.float16):
    """(densities [V], features [V,F]) float32 a compress / decompress round trip must give, from flat labels, the original
    float32 tensors, the VQ voxels' indices (ascending linear index) and the codebook"""
    labels = np.asarray(labels).reshape(-1)
    dens = np.full(labels.size, np.float32(empty), np.float32)
    dens[labels != 0] = np.asarray(densities, np.float32).reshape(-1)[labels != 0].astype(store).astype(np.float32)
    feat = np.zeros((labels.size, np.asarray(features).shape[-1]), np.float32)
    flat = np.asarray(features, np.float32).reshape(labels.size, -1)
    feat[labels == 2] = flat[labels == 2].astype(store).astype(np.float32)
    feat[labels == 1] = np.asarray(codebook, np.float32)[np.asarray(index, np.int64)]
    return dens, feat
