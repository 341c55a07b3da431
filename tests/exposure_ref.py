"""float64 numpy restatement of voxe_exposure_fwd_bwd, voxe_exposure_apply_bwd and voxe_exposure_fit_sums (include/voxe.h,
DESIGN.md 4.21), and the inputs the host and GPU tests share.

Every output comes with the sum of the absolute values of the terms it is a sum of, which the tests' error bounds scale with.
The residual is expanded for that: e_c = sum_j A_cj x_j + b_c - y_c has the magnitude
    mag_c = sum_j |A_cj| |x_j| + |b_c| + |y_c|,
and wherever e enters a product (the L2 gradient 2 omega e, the squares of loss and mse) the terms are those of the expanded
product, so mag stands in for |e|: a float32 residual carries an error of a few 2^-24 mag_c however small e_c itself is."""
import numpy as np

U24 = 2.0 ** -24
FLIP_GUARD = 8.0 * U24          # L1: |e| below FLIP_GUARD * mag may round to the other sign in float32
FLIP_CAP = 1e-3                 # at most this share of the 3R residuals may be that close to 0


def affine(delta):
    """(A [N,3,3], b [N,3]) in float64 of delta [N,12]: the 1 + dA_cc of the kernel rounds in float32 and counts as a rounding"""
    d = np.asarray(delta, np.float64).reshape(-1, 12)
    return d[:, :9].reshape(-1, 3, 3) + np.eye(3), d[:, 9:]


def fwd_bwd(x, y, ids, delta, kind, w=None, grad_scale=1.0):
    """dict of (value, sum of |terms|) pairs under the names loss, mse, corrected, d_x, d_delta, plus `flip` [R,3] (the L1
    residuals too close to 0 to have a float32 sign), `count` [N] (rays per image) and `used` [N]"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    ids = np.asarray(ids).astype(np.int64)
    R, N = x.shape[0], np.asarray(delta).reshape(-1, 12).shape[0]
    ids = np.clip(ids, 0, N - 1)
    A, b = affine(delta)
    Ar, br = A[ids], b[ids]                                        # [R,3,3], [R,3]
    w = np.ones(R) if w is None else np.asarray(w, np.float64)
    corrected = np.einsum("rcj,rj->rc", Ar, x) + br
    corrected_abs = np.einsum("rcj,rj->rc", np.abs(Ar), np.abs(x)) + np.abs(br)
    mag = corrected_abs + np.abs(y)
    e = corrected - y
    n = 3.0 * max(R, 1)
    if kind == "l1":
        loss, loss_abs = (w[:, None] * np.abs(e)).sum() / n, (w[:, None] * mag).sum() / n
        g, g_abs = w[:, None] * np.sign(e), w[:, None] * np.ones_like(e)
    else:
        loss, loss_abs = (w[:, None] * e * e).sum() / n, (w[:, None] * mag * mag).sum() / n
        g, g_abs = 2.0 * w[:, None] * e, 2.0 * w[:, None] * mag
    mse, mse_abs = (e * e).sum() / n, (mag * mag).sum() / n
    gs = grad_scale / n
    out = {"loss": (loss, loss_abs), "mse": (mse, mse_abs), "corrected": (corrected, corrected_abs)}
    out["d_x"] = (gs * np.einsum("rcj,rc->rj", Ar, g), abs(gs) * np.einsum("rcj,rc->rj", np.abs(Ar), g_abs))
    out["d_delta"] = tuple(_segment(ids, N, gg, x if ab == 0 else np.abs(x), s) for ab, (gg, s) in enumerate(((g, gs), (g_abs, abs(gs)))))
    out["flip"] = (np.abs(e) < FLIP_GUARD * mag) if kind == "l1" else np.zeros_like(e, bool)
    out["count"] = np.bincount(ids, minlength=N)
    out["used"] = out["count"] > 0
    out["gs"] = gs
    return out


def _segment(ids, N, g, x, scale):
    """[N,12]: per image scale * sum over its rays of (g x^T row-major, g)"""
    terms = np.concatenate([(g[:, :, None] * x[:, None, :]).reshape(-1, 9), g], axis=1)
    out = np.zeros((N, 12))
    np.add.at(out, ids, terms)
    return scale * out


def apply_bwd(x, ids, delta, d_corrected):
    """{(d_x, |terms|), (d_delta, |terms|)} of the chain rule of c' = A x + b alone"""
    x, g = np.asarray(x, np.float64), np.asarray(d_corrected, np.float64)
    N = np.asarray(delta).reshape(-1, 12).shape[0]
    ids = np.clip(np.asarray(ids).astype(np.int64), 0, N - 1)
    A, _ = affine(delta)
    Ar = A[ids]
    return {"d_x": (np.einsum("rcj,rc->rj", Ar, g), np.einsum("rcj,rc->rj", np.abs(Ar), np.abs(g))),
            "d_delta": (_segment(ids, N, g, x, 1.0), _segment(ids, N, np.abs(g), np.abs(x), 1.0)),
            "count": np.bincount(ids, minlength=N)}


def delta_rows_with_flips(ids, N, flip):
    """bool [N,12]: the d_delta elements a near-zero L1 residual enters (channel c of a ray of image n: row n, columns 3c..3c+2
    and 9+c)"""
    ids = np.clip(np.asarray(ids).astype(np.int64), 0, N - 1)
    hit = np.zeros((N, 3), bool)
    np.logical_or.at(hit, ids, flip)
    return np.concatenate([np.repeat(hit, 3, axis=1), hit], axis=1)


FIT_UPPER = ((0, 0), (0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3))


def fit_sums(x, y):
    """(sums [N,25], sum of |terms| [N,25]) in float64, summed in extended precision: the upper triangle of sum u u^T, u = (x, 1),
    row-major; sum u y^T row-major [4,3]; sum y o y"""
    x, y = np.asarray(x, np.longdouble), np.asarray(y, np.longdouble)
    u = np.concatenate([x, np.ones(x.shape[:2] + (1,), np.longdouble)], axis=2)
    cols = [u[..., i] * u[..., j] for i, j in FIT_UPPER] + [u[..., i] * y[..., c] for i in range(4) for c in range(3)] \
        + [y[..., c] * y[..., c] for c in range(3)]
    t = np.stack(cols, axis=-1)                                    # [N,P,25]
    return t.sum(axis=1).astype(np.float64), np.abs(t).sum(axis=1).astype(np.float64)


def gram(sums):
    """(G [N,4,4], h [N,4,3]) of sums [N,25]"""
    s = np.asarray(sums, np.float64)
    G = np.zeros((s.shape[0], 4, 4))
    for k, (i, j) in enumerate(FIT_UPPER):
        G[:, i, j] = G[:, j, i] = s[:, k]
    return G, s[:, 10:22].reshape(-1, 4, 3)


# ---- inputs shared by tests/test_exposure_host.py and tests/test_exposure_gpu.py ---------------------------------------
RS = (1, 63, 64, 65, 257, 4099)
NS = (1, 3, 70)
KINDS = ("l1", "l2")
PATTERNS = ("one", "runs63", "runs64", "runs65", "shuffle", "unused")


def image_ids(pattern, R, N, rng):
    r = np.arange(R)
    if pattern == "one":
        return np.full(R, N - 1, np.int32)
    if pattern.startswith("runs"):
        # image 0 up to the ray named by the pattern (one short of, at, one past the end of the first wave), then sorted runs of
        # equal length over the other images
        first = int(pattern[4:])
        run = max(1, -(-(R - first) // max(N - 1, 1)))
        return np.where(r < first, 0, np.minimum(1 + (r - first) // run, N - 1)).astype(np.int32)
    if pattern == "shuffle":
        return rng.integers(0, N, R).astype(np.int32)
    # every `step`-th image only: the others stay unused
    step = 2 if N < 10 else 7
    return (rng.integers(0, -(-N // step), R) * step).astype(np.int32)


def inputs(R, N, pattern, weighted, seed=0):
    """(x [R,3], y [R,3], ids [R] int32, delta [N,12], w [R] or None) float32: colours uniform in [0,1], |dA|, |db| <= 0.3,
    weights in [0,2] with a fifth of them 0"""
    rng = np.random.default_rng([R, N, PATTERNS.index(pattern), int(weighted), seed])
    x, y = rng.uniform(0, 1, (R, 3)).astype(np.float32), rng.uniform(0, 1, (R, 3)).astype(np.float32)
    delta = rng.uniform(-0.3, 0.3, (N, 12)).astype(np.float32)
    w = (rng.uniform(0, 2, R) * (rng.uniform(size=R) > 0.2)).astype(np.float32) if weighted else None
    return x, y, image_ids(pattern, R, N, rng), delta, w


def cases():
    return [(R, N) for R in RS for N in NS]


def variants():
    return [(kind, weighted, pattern) for kind in KINDS for weighted in (False, True) for pattern in PATTERNS]
