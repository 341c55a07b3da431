"""numpy restatement of voxe_robust_fwd_bwd (include/voxe.h): the robust photometric loss on pixel patches.

Residuals in float32 in the stated order, tau by np.partition on the float32 array, the mask in integers, loss and mse in
float64, d_x in float32 from the stated g.  Nothing here is derived from the kernel: the formulas of the header are the
specification, and this file restates them with array operations."""
import math

import numpy as np

KINDS = ("l1", "l2")
# (N, P, C) of tests/test_robust_gpu.py
SHAPES = ((1, 4, 1), (3, 16, 3), (1, 64, 4), (5, 6, 3), (128, 16, 3))
MANY_PATCHES = (2049, 4, 1)


def rank_of_quantile(q, M):
    """0-based rank of the quantile q among M values: min(M - 1, max(0, ceil(q M) - 1)), the product in double"""
    return min(M - 1, max(0, math.ceil(float(q) * M) - 1))


def patch_min_of_fraction(f, P):
    """forgiven pixels a patch needs: ceil(f P^2), at least 1; None switches the rule off (P^2 + 1)"""
    return P * P + 1 if f is None else max(1, math.ceil(float(f) * (P * P)))


def residuals(x, y):
    """e [N,P,P] float32: d_0 d_0, then + d_c d_c for c = 1 .. C-1 in that order, every operation rounded to float32"""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    d = x - y
    with np.errstate(over="ignore"):       # (a residual may overflow to +inf: the select's tests ask for it)
        e = d[..., 0] * d[..., 0]
        for c in range(1, d.shape[-1]):
            e = e + d[..., c] * d[..., c]
    assert e.dtype == np.float32
    return e


def threshold(e, rank):
    """the element of 0-based rank `rank` among all values of e: an exact order statistic"""
    return np.partition(e.reshape(-1), rank)[rank]


def neighbour_counts(a):
    """[N,P,P] int: for every pixel the number of set pixels in its 3x3 neighbourhood inside its own patch, itself included"""
    N, P, _ = a.shape
    padded = np.zeros((N, P + 2, P + 2), np.int64)
    padded[:, 1:-1, 1:-1] = a
    n = np.zeros((N, P, P), np.int64)
    for dr in range(3):
        for dc in range(3):
            n += padded[:, dr:dr + P, dc:dc + P]
    return n


def inner(P):
    """[P,P] bool: row and column both in [P // 4, P // 4 + P // 2)"""
    i = np.arange(P)
    one = (i >= P // 4) & (i < P // 4 + P // 2)
    return one[:, None] & one[None, :]


def mask_from_inliers(a, smooth_min, patch_min):
    """(c, w, D) from a [N,P,P] of 0 / 1: c = a | (3x3 count >= smooth_min), D_n = (sum c >= patch_min), w = c | (D & inner)"""
    a = np.asarray(a).astype(np.int64)
    P = a.shape[1]
    c = a | (neighbour_counts(a) >= smooth_min).astype(np.int64)
    D = c.reshape(a.shape[0], -1).sum(1) >= patch_min
    w = c | (D[:, None, None] & inner(P)[None]).astype(np.int64)
    return c, w, D


def fwd_bwd(x, y, rank=0, smooth_min=5, patch_min=1, kind="l1", mask_in=None, grad_scale=1.0):
    """every output of the call: loss, mse (float64), tau (float32), mask [N,P,P] uint8, stats (3 ints), d_x float32"""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    N, P, _, C = x.shape
    M = N * P * P
    if mask_in is None:
        e = residuals(x, y)
        tau = threshold(e, rank)
        a = (e <= tau).astype(np.int64)
        c, w, _ = mask_from_inliers(a, smooth_min, patch_min)
        stats = (int(a.sum()), int(c.sum()), int(w.sum()))
    else:
        w = (np.asarray(mask_in) != 0).astype(np.int64)
        tau, stats = np.float32(0.0), (0, 0, 0)
    d = x - y
    d64 = d.astype(np.float64)
    term = np.abs(d64) if kind == "l1" else d64 * d64
    loss = (term * w[..., None]).sum() / (C * M)
    mse = (d64 * d64).sum() / (C * M)
    # (grad_scale is a C float of the ABI: it is rounded to float32 before the division in double)
    g = np.float32(np.float64(np.float32(grad_scale)) / (C * M))
    wf = w[..., None].astype(np.float32)
    if kind == "l1":
        # sign(0) = 0 (and +0.0, whatever the sign of the zero)
        d_x = (wf * g) * ((d > 0).astype(np.float32) - (d < 0).astype(np.float32))
    else:
        d_x = (wf * (np.float32(2.0) * g)) * d
    assert d_x.dtype == np.float32
    return {"loss": loss, "mse": mse, "tau": np.float32(tau), "mask": w.astype(np.uint8), "stats": stats, "d_x": d_x}


def inputs(N, P, C, seed=0, outlier_patches=0.3):
    """x, y in [0, 1] with every non-zero |x - y| far above 2^-60: a smooth base, small noise everywhere, and blobs of large
    residuals (a square per some patches) so that the neighbourhood and patch rules all fire"""
    rng = np.random.default_rng(seed + 1000 * N + 10 * P + C)
    y = rng.uniform(0.0, 1.0, (N, P, P, C)).astype(np.float32)
    x = (y + rng.normal(0.0, 0.02, y.shape).astype(np.float32)).astype(np.float32)
    for n in range(N):
        if rng.uniform() < outlier_patches:
            s = int(rng.integers(1, P))
            r0, c0 = int(rng.integers(0, P - s + 1)), int(rng.integers(0, P - s + 1))
            x[n, r0:r0 + s, c0:c0 + s] = rng.uniform(0.0, 1.0, (s, s, C)).astype(np.float32)
    # isolated outliers and isolated inliers
    flip = rng.uniform(size=(N, P, P)) < 0.05
    x[flip] = (1.0 - y[flip]).astype(np.float32)
    d = x - y
    assert (np.abs(d[d != 0]) > 2.0 ** -60).all()
    return x, y
