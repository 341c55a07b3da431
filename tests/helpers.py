"""Shared helpers of the parity tests (oracle-side: numpy only)."""
import numpy as np

from voxe_hip import abi
from voxe_hip.desc import make_render_cfg

from oracle import voxe_oracle as vo

KINDS = {
    # kind -> (density_pre_act, density_post_act, expected_density_scale) as built by tools/gen_golden.py
    "softplus": (abi.ACT_IDENTITY, abi.ACT_SOFTPLUS, 100.0 / 3.0),
    "softplus_soft": (abi.ACT_IDENTITY, abi.ACT_SOFTPLUS, 2.0),
    "relu": (abi.ACT_IDENTITY, abi.ACT_RELU, 100.0 / 3.0),
    "abs": (abi.ACT_ABS, abi.ACT_IDENTITY, 1.0),
}


def grid_from_golden(g, prefix, kind, attn=False):
    pre, post, scale = KINDS[kind]
    aabb = [tuple(r) for r in g[prefix + "aabb"]]
    feats = g[prefix + ("attn" if attn else "features")]
    return vo.Grid(g[prefix + "densities"], feats, aabb, scale, pre, post,
                   abi.FEAT_ATTN if attn else abi.FEAT_SH)


def cfg_from_bounds(bounds, S, **kw):
    return make_render_cfg(S, float(bounds[0]), float(bounds[1]), **kw)


def rel_l2(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def psnr(a, b):
    mse = float(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2))
    return float("inf") if mse == 0 else -10.0 * np.log10(mse)


def nan_equal(a, b, rtol, atol):
    a, b = np.asarray(a), np.asarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb), "NaN pattern differs"
    np.testing.assert_allclose(a[~na], b[~nb], rtol=rtol, atol=atol)


def band_errors(got, ref, bands):
    """relative error of `got` per magnitude band of the reference: for every (lo, hi] in `bands` (fractions of max |ref|)
    that holds at least one element -> (count, median of |got - ref| / |ref|, 99th percentile)"""
    ref = np.asarray(ref, np.float64).ravel()
    err = np.abs(np.asarray(got, np.float64).ravel() - ref)
    mag = np.abs(ref)
    big = float(mag.max())
    out = {}
    for lo, hi in bands:
        m = (mag > lo * big) & (mag <= hi * big)
        if m.any():
            rel = err[m] / mag[m]
            out[(lo, hi)] = (int(m.sum()), float(np.median(rel)), float(np.quantile(rel, 0.99)))
    return out


# ---- the per-voxel error budget of the render backward (oracle/voxe_cpu.c: voxe_cpu_render_bwd_budget) ----------------------------
EPS32 = 2.0 ** -24
FLT_MIN = 1.1754943508222875e-38        # smallest normal float32
EXEMPT_FRACTION = 1e-20                 # of the tensor's largest `mag`
STRAY_FRACTION = 1e-12                  # of max |ref|, where the oracle deposits nothing (tests/test_hip_hygiene_r03.py's rule)


def per_voxel_report(got, ref, mag, budget, count, fixed_point_bits=None):
    """|got - ref| against the per-voxel bound, element by element:
      budget > 0:   bound = EPS32 * (budget + count * mag) + floor, floor = (count + 1) * FLT_MIN: every deposit and the stored
                    value may each be flushed to zero below the smallest normal float32;
      exempt:       mag < 1e-20 x the tensor's largest mag (voxels behind a transmittance in float32's denormal range): held
                    only to an absolute error of 1e-20 x that maximum (or to their bound where that is larger);
      fixed_point_bits = n (the deterministic backward): every deposit is truncated to 2^-n of the launch's largest contribution,
                    which is at most the largest mag: count * 2^-n * max(mag) on top;
      budget == 0:  nothing is deposited there: |got| <= 1e-12 x max |ref|.
    -> dict(ratio = |got - ref| / bound per element, flagged = ratio > 1, worst, where, touched, exempt, exempt_share)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    mag, budget, count = np.asarray(mag, np.float64), np.asarray(budget, np.float64), np.asarray(count, np.float64)
    assert got.shape == ref.shape == mag.shape == budget.shape == count.shape, (got.shape, ref.shape, mag.shape, budget.shape, count.shape)
    assert np.isfinite(got).all() and np.isfinite(budget).all() and np.isfinite(mag).all()
    touched = budget > 0
    top = float(mag.max(initial=0.0))
    exempt = touched & (mag < EXEMPT_FRACTION * top)
    bound = EPS32 * (budget + count * mag) + (count + 1.0) * FLT_MIN
    if fixed_point_bits is not None:
        bound += count * (2.0 ** -fixed_point_bits) * top
    bound[exempt] = np.maximum(bound[exempt], EXEMPT_FRACTION * top)
    bound[~touched] = STRAY_FRACTION * float(np.abs(ref).max(initial=0.0))
    err = np.abs(got - ref)
    ratio = np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))
    where = np.unravel_index(int(np.argmax(ratio)), ratio.shape) if ratio.size else ()
    n_touched = int(touched.sum())
    return dict(ratio=ratio, flagged=ratio > 1.0, worst=float(ratio.max(initial=0.0)), where=tuple(int(i) for i in where), touched=touched,
                exempt=exempt, exempt_share=float(exempt.sum()) / max(n_touched, 1), bound=bound)


def per_voxel_check(got, ref, mag, budget, count, what, fixed_point_bits=None):
    """asserts the bound of per_voxel_report at EVERY element, prints the largest ratio |got - ref| / bound and the voxel it occurs
    at, returns the exempt share of the touched voxels (the caller asserts its cap)"""
    rep = per_voxel_report(got, ref, mag, budget, count, fixed_point_bits)
    w = rep["where"]
    line = f"{what}: largest |got - ref| / bound {rep['worst']:.3g}"
    if w:
        line += (f" at {w} (got {float(np.asarray(got)[w]):.6e} ref {float(np.asarray(ref)[w]):.6e} bound {float(rep['bound'][w]):.3e} "
                 f"mag {float(np.asarray(mag)[w]):.3e} count {int(np.asarray(count)[w])}"
                 f"{' exempt' if rep['exempt'][w] else ''}{'' if rep['touched'][w] else ' untouched'})")
    print(line + f"; {int(rep['flagged'].sum())} of {int(rep['touched'].sum())} touched elements over; exempt {rep['exempt_share']:.2%}")
    assert not rep["flagged"].any(), line
    return rep["exempt_share"]
