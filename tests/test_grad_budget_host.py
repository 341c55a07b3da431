"""The per-voxel error budget of the render backward on the CPU: the budget twin of the oracle (oracle/voxe_cpu.c,
voxe_cpu_render_bwd_budget) and tests/helpers.py's per_voxel_check, before any kernel is held to them.

  sanity         mag >= |gradient| at every voxel (triangle inequality), budget >= A * mag, count == the deposits counted from the
                 sample probe;
  calibration    the reference's OWN float32 autograd gradients (tests/golden) lie within the budget of the oracle's gradient;
  bite           three corruptions of the oracle's gradient that tests/test_hip_fuzz.py's _close passes are flagged voxel by voxel --
                 fed through the GPU tests' own checking functions (the mutation check of tests/test_hip_grad_per_voxel.py);
  preconditions  of the GPU case table (tests/grad_budget_cases.py), in the manner of tests/test_degenerate_host.py.

Calibration, measured with A, B, C, Q, V = 16, 2, 2, 1 (2 where e >= 1/2), 8 -- largest |golden - oracle| / bound per golden file,
densities / features:
  render_sh0.npz (22 cases x 2 upstream sets)   0.026 / 0.46   (non-opaque kinds 0.026 / 0.20; opaque softplus 0.013 / 0.46, whose
                                                exempt share is 0.19 - 0.25 % of the touched feature values; nothing else is exempt)
  render_attn.npz                               0.036 / 0.50   (opaque softplus: one voxel with one deposit behind one grid step of alpha)
  render_shdeg.npz (degree 1-3, full, diffuse)  0.0037 / 0.12
  degenerate_rays.npz (24 cases)                0.012 / 0.086
With A, B, C alone (no Q: the 2^-24 grid of alpha = 1 - exp(-x), see the comment above the twin) the same run gives 1.08 on relu_jit and
3.1e3 - 7.4e3 on the opaque softplus features: the reference does not fit them, and Q is the rounding source that was missing, not a
rescaling.  Two terms are invisible to this calibration and come from the kernels' code, each after a GPU run had shown voxels with ONE
deposit just over the bound (1.5 - 1.9 x): V, the interpolations' absolute rounding (the reference interpolates in the oracle's order),
and the second grid step of alpha where e >= 1/2 (an ulp of e is a grid step there, and the kernels' exp is another faithful exp)."""
import numpy as np
import pytest

import degenerate_cases as dc
import grad_budget_cases as gb
from conftest import load_golden
from helpers import EPS32, KINDS, cfg_from_bounds, grid_from_golden, per_voxel_check, per_voxel_report
from test_hip_fuzz import _close
from test_oracle_vs_golden import _degenerate_names, _render_cases

from oracle import voxe_oracle as vo

NAMES = ("densities", "features")
OPAQUE = ("softplus",)            # KINDS whose transmittance reaches float32's denormal range: their exempt share is reported, not capped
EXEMPT_CAP = 0.01


def _calibrate(what, kind, grid, cfg, o, d, ups, golden, jitter=None):
    """-> largest ratio per tensor; asserts ratio <= 1 (per_voxel_check) and the exempt cap on the non-opaque kinds"""
    ref = vo.render_bwd(grid, cfg, o, d, *ups, jitter=jitter)
    bud = vo.render_bwd_budget(grid, cfg, o, d, *ups, jitter=jitter)
    worst = []
    for i, name in enumerate(NAMES):
        share = per_voxel_check(golden[i], ref[i], *bud[name], f"{what} {name}")
        if kind not in OPAQUE:
            assert share <= EXEMPT_CAP, (what, name, share)
        worst.append(per_voxel_report(golden[i], ref[i], *bud[name])["worst"])
    return worst


# ---- sanity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["soft", "dense", "sphere", "relu", "abs", "attn", "sh2", "sh2_diffuse", "dense_eps1e-2", "saturated"])
def test_mag_bounds_the_gradient_and_the_budget_bounds_mag(name):
    r = gb.reference(name)
    A = vo.budget_constants()[0]
    for which, up in r["sets"].items():
        for i, n in enumerate(NAMES):
            mag, budget, count = up["budget"][n]
            ref = np.abs(up["bwd"][i].astype(np.float64))
            # (the oracle's gradient is a double sum rounded to float32 once: half an ulp above the sum of magnitudes at most)
            assert (ref <= mag * (1 + 2 * EPS32) + 1e-45).all(), (name, which, n, float((ref - mag).max()))
            assert (budget >= A * mag).all(), (name, which, n)
            assert ((mag > 0) <= (budget > 0)).all() and ((budget > 0) <= (count > 0)).all()
    if name == "dense":             # the whole ray as one block (the plain scatter kernel's contract) is never tighter, and leaves mag alone
        up = r["sets"]["all"]
        whole = gb.whole_ray_budget("dense", "image", "all")
        np.testing.assert_allclose(whole["densities"][0], up["budget"]["densities"][0], rtol=1e-12)     # (the order of the double sums)
        assert (whole["densities"][1] >= up["budget"]["densities"][1] * (1 - 1e-12)).all()
        assert (whole["densities"][1] > 2 * up["budget"]["densities"][1]).mean() > 0.1
        np.testing.assert_allclose(whole["features"][1], up["budget"]["features"][1], rtol=1e-12)
    if name == "sh2_diffuse":       # only the constant coefficient of each colour is deposited
        per_colour = r["sets"]["colour"]["budget"]["features"][1].reshape(gb.SH_DIMS + (3, 9))
        assert not per_colour[..., 1:].any() and per_colour[..., 0].any()


@pytest.mark.parametrize("name", ["sh1", "odd", "dense_eps1e-2"])
def test_count_equals_the_deposits_of_the_sample_probe(name):
    """count[voxel] = number of (inside sample in front of the cut, in-bounds corner) pairs that address it"""
    r = gb.reference(name)
    grid, dims = r["grid"], r["grid"].densities.shape[:3]
    probe = vo.sample_probe(grid, r["cfg"], r["o"], r["d"], r["jit"])
    live = probe["inside"].copy()
    if r["cut"] is not None:
        live &= np.arange(r["case"].S)[None, :] < r["cut"][:, None]
    i0 = probe["idx"][live].astype(np.int64)
    want = np.zeros(dims, np.int64)
    for cx in (0, 1):
        for cy in (0, 1):
            for cz in (0, 1):
                p = i0 + np.array([cx, cy, cz])
                ok = ((p >= 0) & (p < np.array(dims))).all(1)
                np.add.at(want, tuple(p[ok].T), 1)
    count = r["sets"]["colour"]["budget"]["densities"][2][..., 0]
    assert np.array_equal(count, want) and want.max() > 8


def test_the_saturated_case_has_saturated_interior_samples():
    """om == 0 with e != 0 away from the closing interval: x = sigma * delta between 17.4 (1 - e rounds to 1) and 87 (e underflows),
    in front of which the transmittance is still above 1e-6 -- and the term the oracle keeps there is visible to the bound: an
    oracle gradient with the transmittance-weighted tail of those samples removed is what a `suffix / om` kernel computes"""
    r = gb.reference("saturated")
    probe = vo.sample_probe(r["grid"], r["cfg"], r["o"], r["d"], r["jit"])
    dnorm = np.linalg.norm(r["d"].astype(np.float64), axis=1)
    x = np.where(probe["inside"], probe["sigma"].astype(np.float64), 0.0)[:, :-1] * np.diff(probe["z"].astype(np.float64), axis=1) * dnorm[:, None]
    T = np.exp(-np.concatenate([np.zeros((x.shape[0], 1)), np.cumsum(x, axis=1)[:, :-1]], axis=1))
    sat = (x > 17.4) & (x < 87.0) & (T > 1e-6)
    print(f"saturated interior samples in sight: {int(sat.sum())} on {int(sat.any(1).sum())} of {x.shape[0]} rays")
    assert sat.any(1).sum() >= 128      # (more than a wave of rays, in more than one 8 x 8 pixel tile: 432 measured)


# ---- calibration against the reference's float32 autograd --------------------------------------------------------------------------
@pytest.mark.parametrize("tag", [t for t in _render_cases() if t + "grad_densities" in load_golden("render_sh0.npz").files])
def test_the_reference_s_sh0_gradients_lie_within_the_budget(tag):
    g = load_golden("render_sh0.npz")
    kind = next(k for k in sorted(KINDS, key=len, reverse=True) if tag.startswith(k + "_"))
    grid = grid_from_golden(g, kind + "_", kind)
    rest = tag[len(kind) + 1:]
    kw = {}
    if rest.startswith("S"):
        S = int(rest.split("_")[0][1:])
        kw["white_bkgd"] = rest.split("_")[1] == "w1"
    else:
        S = 64
        kw["white_bkgd"] = True
        if rest.startswith("jit"):
            kw["perturb"] = True
        elif rest.startswith("lindisp"):
            kw["linear_disparity"] = True
        elif rest.startswith("clipjit"):
            kw["aabb_clip"] = kw["perturb"] = True
        elif rest.startswith("clip"):
            kw["aabb_clip"] = True
    cfg = cfg_from_bounds(g["bounds"], S, **kw)
    jit = g[tag + "jitter"] if tag + "jitter" in g.files else None
    o, d = g["rays_o"], g["rays_d"]
    for pre, ups in (("grad_", (g[tag + "g_colour"], None, None)), ("grad2_", (g[tag + "g_colour"], g[tag + "g_depth"], g[tag + "g_acc"]))):
        _calibrate(tag + pre, kind, grid, cfg, o, d, ups, (g[tag + pre + "densities"], g[tag + pre + "features"]), jit)


@pytest.mark.parametrize("kind", ["softplus", "softplus_soft"])
@pytest.mark.parametrize("white", [0, 1])
def test_the_reference_s_attention_gradients_lie_within_the_budget(kind, white):
    g = load_golden("render_attn.npz")
    grid = grid_from_golden(g, kind + "_", kind, attn=True)
    tag = f"{kind}_w{white}_"
    cfg = cfg_from_bounds(g["bounds"], 48, white_bkgd=bool(white))
    _calibrate("attn " + tag, kind, grid, cfg, g["rays_o"], g["rays_d"], (g[tag + "g_colour"], None, None),
               (g[tag + "grad_densities"], g[tag + "grad_features"]))


@pytest.mark.parametrize("deg", [1, 2, 3])
@pytest.mark.parametrize("mode", ["full", "diffuse"])
def test_the_reference_s_view_dependent_gradients_lie_within_the_budget(deg, mode):
    g = load_golden("render_shdeg.npz")
    grid = grid_from_golden(g, f"deg{deg}_", "softplus_soft")
    tag = f"deg{deg}_{mode}_"
    cfg = cfg_from_bounds(g["bounds"], 32, white_bkgd=True, sh_degree=deg, render_diffuse=(mode == "diffuse"))
    _calibrate("shdeg " + tag, "softplus_soft", grid, cfg, g["rays_o"], g["rays_d"], (g[tag + "g_colour"], None, None),
               (g[tag + "grad_densities"], g[tag + "grad_features"]))


@pytest.mark.parametrize("name", _degenerate_names())
def test_the_reference_s_gradients_on_degenerate_rays_lie_within_the_budget(name):
    g = load_golden("degenerate_rays.npz")
    c = dc.case(name)
    c.grid = grid_from_golden(g, "", "softplus_soft")
    o, d = dc.rays(c)
    R = o.shape[0]
    tag = name + "/"
    jit = g[tag + "jitter"] if tag + "jitter" in g.files else None
    _calibrate("degenerate " + name, "softplus_soft", c.grid, c.cfg(), o, d, (g[f"R{R}/g_colour"], g[f"R{R}/g_depth"], g[f"R{R}/g_acc"]),
               (g[tag + "grad_densities"], g[tag + "grad_features"]), jit)


# ---- bite: what a global rel-L2 passes, the per-voxel bound flags ---------------------------------------------------------------------
def _passes(fn, *args):
    try:
        fn(*args)
    except AssertionError:
        return False
    return True


@pytest.mark.parametrize("name", ["sphere", "soft"])
def test_the_bound_flags_what_a_global_norm_passes(name):
    """the mutation check of tests/test_hip_grad_per_voxel.py: each corruption of the ORACLE's gradient goes through the GPU tests'
    checking functions in the kernel's place -- it passes the old check (global_check) and fails the new one (per_voxel).  On the
    sphere all three corruptions pass _close (rel-L2 1.9e-6 / 7.7e-5 / below 1e-4); on the soft random grid the gradient's energy is spread
    evenly, a zeroed face and 1.01 on 0.1 % of the voxels are visible to the norm (1.9e-1, 1.9e-4) and only the lost eighth passes it
    (7.4e-6 / 1.5e-5) -- there the other two must be flagged all the same."""
    r = gb.reference(name)
    up = r["sets"]["colour"]
    ref = up["bwd"]
    for i, n in enumerate(NAMES):
        for cname, (bad, changed) in gb.corruptions(ref[i]).items():
            got = [ref[0], ref[1]]
            got[i] = bad
            rep = per_voxel_report(bad, ref[i], *up["budget"][n])
            hit = int((rep["flagged"] & changed).sum())
            old = _passes(gb.global_check, r, "colour", got, cname)
            print(f"{name} {n} {cname}: {int(changed.sum())} changed, {hit} flagged, the global check {'passes' if old else 'fails'}")
            assert not rep["flagged"][~changed].any()
            assert not _passes(gb.per_voxel, r, "colour", got, cname), (name, n, cname)
            if name == "sphere" or cname == "lost_eighth":
                assert old, (name, n, cname)
                _close(n, bad, ref[i])
            if cname == "zeroed_face" and not (name == "sphere" and n == "features"):
                # (the sphere's 30 feature values on that face are one or two grid steps of alpha: the oracle itself does not know them better)
                assert hit == int(changed.sum()) and hit >= 800, (name, n, hit, int(changed.sum()))
            if cname == "lost_eighth":
                assert 2 * hit >= int(changed.sum()) and hit > 300, (name, n, hit, int(changed.sum()))
            if cname == "scaled_1.01":
                assert 2 * hit >= int(changed.sum()), (name, n, hit, int(changed.sum()))


# ---- preconditions of the GPU case table ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["image", "permuted"])
@pytest.mark.parametrize("name", gb.SCENES)
def test_scene_preconditions_hold_on_the_oracle(name, order):
    r = gb.reference(name, order)
    need = gb.NEED[name]
    for which, up in r["sets"].items():
        for i, n in enumerate(NAMES):
            ref = up["bwd"][i]
            rep = per_voxel_report(ref, ref, *up["budget"][n])
            touched = rep["touched"]
            tight = float(((rep["bound"] < 1e-2 * np.abs(ref)) & touched).sum()) / float(touched.sum())
            print(f"{name} {order} {which} {n}: touched {touched.mean():.1%}  exempt {rep['exempt_share']:.2%}  bound < 1e-2 |ref| on {tight:.1%}")
            assert touched.mean() >= need["touched"][i], (name, which, n, float(touched.mean()))
            assert rep["exempt_share"] <= need["exempt"][i], (name, which, n, rep["exempt_share"])
            assert tight >= need["tight"][i], (name, which, n, tight)
