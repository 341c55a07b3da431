"""Degenerate ray geometry through every render route, HIP vs the oracle: the case table of tests/degenerate_cases.py (axis-aligned
views with direction components exactly +-0, samples exactly on voxel planes and AABB faces, exact ties between two / three march
axes, eyes on a face and on a lattice point, launches in which no ray meets the grid, 1xN / Nx1 / 1x1 images, six axis views in one
launch).  Sample indices and masks bit for bit; renders, gradients and the bit-identity claims with the rules of
tests/test_hip_fuzz.py, tests/test_hip_r06.py and tests/test_hip_sched.py; the three ray-marching side kernels (normals, visibility,
distortion) against their float64 restatements with the bounds of their own `..._matches_the_restatement` tests.

The oracle is pinned to the reference on this geometry by tests/test_oracle_vs_golden.py (tests/golden/degenerate_rays.npz), the
table's preconditions are checked on the oracle alone by tests/test_degenerate_host.py."""
import functools

import numpy as np
import pytest
import torch

import degenerate_cases as dc
from helpers import per_voxel_check
from test_hip_fuzz import _close
from voxe_hip import abi

from oracle import voxe_oracle as vo

pytestmark = pytest.mark.gpu
DET_BITS = 37       # the deterministic backward truncates every deposit to 2^-37 of the launch's largest contribution (64-bit fixed point)

if torch.cuda.is_available():
    import gpu_helpers as gh
    from voxe_hip import ops

TILE = dict(tile_min_rays=-1)
# name -> (dispatch fields, ray order, voxe_render_route of the launch)
ROUTES = {
    "shipped": ({}, "image", abi.ROUTE_PACKED_SCATTER),                 # small image: line-dense scatter backward
    "plain_scatter": (dict(bwd_mode=1), "image", abi.ROUTE_SCATTER),
    "lean_tile": (dict(TILE), "image", abi.ROUTE_TILE),
    "general_tile": (dict(TILE, tile_lean=-1), "image", abi.ROUTE_TILE),
    "general_tile_kl10": (dict(TILE, tile_lean=-1, tile_kl=10), "image", abi.ROUTE_TILE),
    "precise": (dict(TILE, precise_grad=1), "image", abi.ROUTE_TILE),
    "cost_order": (dict(TILE, tile_map=4), "image", abi.ROUTE_TILE),
    "split_tiles_q1": (dict(TILE, tile_fit_lat=1.0, tile_qsplit=1), "image", abi.ROUTE_TILE),
    "split_tiles_q4": (dict(TILE, tile_fit_lat=1.0, tile_qsplit=4), "image", abi.ROUTE_TILE),
    "deterministic": (dict(TILE), "image", abi.ROUTE_DETERMINISTIC),
    "region_unordered": (dict(region_min_rays=1), "permuted", abi.ROUTE_REGION),
    "region_unordered_global_ranks": (dict(region_min_rays=1, region_lds_ranks=-1), "permuted", abi.ROUTE_REGION),
    "region_image": (dict(region_min_rays=1, region_image_ratio=-1.0), "image", abi.ROUTE_REGION),
}


def _seed_of(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name))


@functools.lru_cache(maxsize=None)
def _ref(name, order="image", deg=0, diffuse=False):
    """the oracle's probe, render and gradients of one case, computed once and shared (nobody writes into them); order
    "permuted": the same rays shuffled, as an unordered batch (the in-kernel jitter stream is indexed by the ray's position)"""
    c = dc.case(name)
    if deg:
        c.grid = dc.sh_grid(deg)
    cfg = c.cfg(sh_degree=deg, render_diffuse=diffuse)
    o, d = dc.rays(c)
    jit = dc.jitter_of(c)
    if not deg:
        dc.check_preconditions(c, o, d)
    rng = np.random.default_rng(_seed_of(name))
    R = o.shape[0]
    gc = rng.standard_normal((R, 3)).astype(np.float32)
    gdep = (0.2 * rng.standard_normal(R)).astype(np.float32) if not deg else None
    gacc = (0.2 * rng.standard_normal(R)).astype(np.float32) if not deg else None
    if order == "permuted":
        perm = rng.permutation(R)
        o, d, gc, gdep, gacc = (np.ascontiguousarray(a[perm]) for a in (o, d, gc, gdep, gacc))
        jit = None if jit is None else np.ascontiguousarray(jit[perm])
    out = dict(case=c, order=order, cfg=cfg, o=o, d=d, jit=jit, gc=gc, gdep=gdep, gacc=gacc, width=c.W if order == "image" else 0,
               over=dict(image_width=c.W, image_height=c.H if c.views > 1 else 0) if order == "image" else dict(image_width=0))
    out["probe"] = vo.sample_probe(c.grid, cfg, o, d, jit)
    out["fwd"] = vo.render_fwd(c.grid, cfg, o, d, jit)
    out["bwd"] = vo.render_bwd(c.grid, cfg, o, d, gc, d_depth=gdep, d_acc=gacc, jitter=jit)
    out["budget"] = vo.render_bwd_budget(c.grid, cfg, o, d, gc, d_depth=gdep, d_acc=gacc, jitter=jit)
    return out


@functools.lru_cache(maxsize=None)
def _whole_ray_budget(name, order):
    r = _ref(name, order)
    return vo.render_bwd_budget(r["case"].grid, r["cfg"], r["o"], r["d"], r["gc"], d_depth=r["gdep"], d_acc=r["gacc"], jitter=r["jit"],
                                segment=r["cfg"].num_samples)


def _check_forward(r, got):
    """tests/test_hip_fuzz.py's rule: 5e-6 x scale + 3e-8 x S (depth: both x max(1, far)), and the disparity's NaN pattern"""
    ref, cfg = r["fwd"], r["cfg"]
    for k in ("colour", "depth", "acc"):
        scale = max(1.0, float(np.abs(ref[k]).max())) * (max(1.0, float(cfg.far)) if k == "depth" else 1.0)
        atol = 5e-6 * scale + 3e-8 * cfg.num_samples * (max(1.0, float(cfg.far)) if k == "depth" else 1.0)
        err = float(np.abs(got[k] - ref[k].reshape(got[k].shape)).max())
        print(f"{r['case'].name} forward {k}: max|err| {err:.3e} (bound {atol:.3e})")
        np.testing.assert_allclose(got[k], ref[k].reshape(got[k].shape), rtol=0, atol=atol, err_msg=k)
    assert np.array_equal(np.isnan(got["disparity"]), np.isnan(ref["disparity"]))
    if r["case"].need.get("miss"):       # nothing was rendered: the background, exactly
        assert np.array_equal(got["acc"], ref["acc"]) and np.array_equal(got["colour"], ref["colour"]) and not got["acc"].any()


def _check_backward(r, got, route=""):
    """tests/test_hip_fuzz.py's _close (1e-4 rel-L2 + its absolute floor) and tests/helpers.py's per_voxel_check (the budget twin of
    the oracle); an exactly-zero oracle gradient: exactly zero"""
    for name, got_g, ref_g in (("densities", got[0], r["bwd"][0]), ("features", got[1], r["bwd"][1])):
        err = float(np.linalg.norm(got_g.astype(np.float64) - ref_g.astype(np.float64)))
        print(f"{r['case'].name} backward {name}: |err| {err:.3e}  |ref| {float(np.linalg.norm(ref_g)):.3e}")
        if not ref_g.any():
            assert np.array_equal(got_g, np.zeros_like(got_g)), name
        depth_grad = r["gdep"] is not None and np.any(r["gdep"] != 0.0)
        _close(name, got_g, ref_g, far=r["cfg"].far if (name == "densities" and depth_grad) else 1.0)
        # every voxel against its own float32 error budget: the 5e-5 floor above swallows these small gradients whole
        # (the plain scatter's suffix is `total - prefix` over the whole ray: the twin with one block per ray)
        budget = _whole_ray_budget(r["case"].name, r["order"]) if route == "plain_scatter" else r["budget"]
        exempt = per_voxel_check(got_g, ref_g, *budget[name], f"{r['case'].name} backward {name}",
                                 fixed_point_bits=DET_BITS if route == "deterministic" else None)
        # (voxels behind a transmittance below 1e-20: only the opaque ReLU x 100/3 lattice has more than 1 % of them)
        assert exempt <= 0.01 or r["case"].grid.density_scale >= 20.0, (name, exempt)


def _hip_route(r, **over):
    c = r["case"]
    params = gh.params_of(r["cfg"], **{**r["over"], **over})
    g, cf = ops._descs(gh.spec_of(c.grid), params, gh.t(c.grid.densities), gh.t(c.grid.features), c.rng[0], c.rng[1], False)
    return ops._route(g, cf, r["o"].shape[0])


# ---- index math: bit for bit, both ray orders ---------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["image", "permuted"])
@pytest.mark.parametrize("name", dc.NAMES)
def test_sample_probe_is_bit_exact(name, order):
    r = _ref(name, order)
    c = r["case"]
    got = gh.hip_probe(c.grid, r["cfg"], r["o"], r["d"], r["jit"], rng=c.rng, **r["over"])
    ref = r["probe"]
    assert np.array_equal(got["inside"].astype(bool), ref["inside"])
    assert np.array_equal(got["z"], ref["z"])
    m = ref["inside"]
    assert np.array_equal(got["idx"][m], ref["idx"][m])


# ---- every case through every route -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", dc.NAMES)
def test_case_through_route(name, route, disp):
    fields, order, want_route = ROUTES[route]
    r = _ref(name, order)
    c = r["case"]
    disp.set(**fields)
    det = dict(deterministic=True) if route == "deterministic" else {}
    assert _hip_route(r, **det) == want_route
    args = (c.grid, r["cfg"], r["o"], r["d"])
    _check_forward(r, gh.hip_forward(*args, r["jit"], rng=c.rng, **r["over"]))
    bwd = lambda: gh.hip_backward(*args, r["gc"], g_depth=r["gdep"], g_acc=r["gacc"], jitter=r["jit"], rng=c.rng, **r["over"], **det)  # noqa: E731
    got = bwd()
    _check_backward(r, got, route)
    if route == "deterministic":
        again = bwd()
        assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1])


# ---- bit-identity claims of the project, on this geometry ---------------------------------------------------------------------
def _forwards_equal(a, b):
    for k in ("colour", "depth", "acc", "disparity"):
        assert np.array_equal(np.isnan(a[k]), np.isnan(b[k])), k
        assert np.array_equal(a[k], b[k], equal_nan=True), k


@pytest.mark.parametrize("name,zdom", [(n, False) for n in dc.NAMES] + [("axis+z", True), ("axis-z", True)])
def test_window_forward_equals_the_ray_ordered_forward_bit_for_bit(name, zdom, disp):
    r = _ref(name)
    c = r["case"]
    fields = dict(TILE, fwd_zdom=-1.0) if zdom else dict(TILE)
    disp.set(fwd_window=-1, **fields)
    a = gh.hip_forward(c.grid, r["cfg"], r["o"], r["d"], r["jit"], rng=c.rng, **r["over"])
    disp.set(fwd_window=0, **fields)
    b = gh.hip_forward(c.grid, r["cfg"], r["o"], r["d"], r["jit"], rng=c.rng, **r["over"])
    _forwards_equal(a, b)
    _check_forward(r, b)


@pytest.mark.parametrize("name", dc.NAMES)
def test_cost_order_changes_no_forward_bit(name, disp):
    r = _ref(name)
    c = r["case"]
    disp.set(tile_map=3, **TILE)
    a = gh.hip_forward(c.grid, r["cfg"], r["o"], r["d"], r["jit"], rng=c.rng, **r["over"])
    disp.set(tile_map=4, **TILE)
    b = gh.hip_forward(c.grid, r["cfg"], r["o"], r["d"], r["jit"], rng=c.rng, **r["over"])
    _forwards_equal(a, b)


# ---- view-dependent grids: the SH basis at v = d / |d| with exact zero components ----------------------------------------------
@pytest.mark.parametrize("two_phase", [0, -1])
@pytest.mark.parametrize("deg", [1, 2, 3])
@pytest.mark.parametrize("name", dc.SH_CASES)
def test_view_dependent_grid(name, deg, two_phase, disp):
    _sh_check(name, deg, False, two_phase, disp)


def test_view_dependent_grid_rendered_diffuse(disp):
    _sh_check("axis-z", 2, True, 0, disp)


def _sh_check(name, deg, diffuse, two_phase, disp):
    r = _ref(name, "image", deg, diffuse)
    c = r["case"]
    args = (c.grid, r["cfg"], r["o"], r["d"])
    # the wide-window forward against the ray-ordered one (tests/test_hip_r06.py): every output bit
    disp.set(region_min_rays=-1, tile_two_phase=two_phase, fwd_window=-1, **TILE)
    a = gh.hip_forward(*args, **r["over"])
    disp.set(fwd_window=0)
    b = gh.hip_forward(*args, **r["over"])
    for k in ("colour", "depth", "acc"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert np.array_equal(np.isnan(a["disparity"]), np.isnan(b["disparity"]))
    err = float(np.abs(b["colour"] - r["fwd"]["colour"]).max())
    print(f"{name} deg {deg} forward colour: max|err| {err:.3e}")
    np.testing.assert_allclose(b["colour"], r["fwd"]["colour"], rtol=0, atol=5e-6)
    assert np.array_equal(np.isnan(b["disparity"]), np.isnan(r["fwd"]["disparity"]))
    _check_backward(r, gh.hip_backward(*args, r["gc"], **r["over"]))


# ---- the ray-marching side kernels (they share RayCtx with the render) ---------------------------------------------------------
def _side_inputs(name):
    r = _ref(name)
    c = r["case"]
    spec, params = gh.spec_of(c.grid), gh.params_of(r["cfg"], **r["over"])
    return r, c, spec, params, gh.t(c.grid.densities), gh.t(c.grid.features), gh.t(r["o"]), gh.t(r["d"])


@pytest.mark.parametrize("name", dc.SIDE_CASES)
def test_render_normals_match_the_restatement(name):
    import normals_ref

    r, c, spec, params, dens, feat, ro, rd = _side_inputs(name)
    N, depth, acc = ops.render_normals(spec, params, dens, ro, rd)
    rN, rdepth, racc = normals_ref.render_normals(spec, params, dens, feat, ro, rd)
    print(f"{name}: max|N - ref| {float((N.double() - rN).abs().max()):.3e}  max|acc - ref| {float((acc[:, 0].double() - racc).abs().max()):.3e}")
    assert float((N.double() - rN).abs().max()) <= 1e-4
    assert float((acc[:, 0].double() - racc).abs().max()) <= 1e-5
    assert bool((N.norm(dim=1) <= acc[:, 0] * (1 + 1e-5) + 1e-6).all())
    with torch.no_grad():
        _, fdepth, facc, _ = ops.render(spec, params, dens, feat, ro, rd)
    assert float((acc - facc).abs().max()) <= 2e-6
    assert float(((depth - fdepth).abs() / fdepth.abs().clamp_min(1e-3)).max()) <= 1e-5
    if c.need.get("miss"):      # acc = 0: the restatement's normals are exact zeros
        assert int(rN.count_nonzero()) == 0 and int(N.count_nonzero()) == 0 and int(acc.count_nonzero()) == 0
    else:
        assert float(acc.max()) > 0.5 and float(N.norm(dim=1).max()) > 0.1


@pytest.mark.parametrize("name", dc.SIDE_CASES)
def test_visibility_matches_the_restatement(name):
    import visibility_ref

    r, c, spec, params, dens, feat, ro, rd = _side_inputs(name)
    g = torch.Generator().manual_seed(4)
    shape = dens.shape[:3]
    miss = bool(c.need.get("miss"))
    # (a launch that sees nothing must leave a grid exactly as it was initialised: pre-filled buffers there)
    pre = [(torch.rand(shape, generator=g) * s).to(gh.DEV) if miss else torch.zeros(shape, device=gh.DEV) for s in (0.05, 1.0)]
    mw, mt = pre[0].clone(), pre[1].clone()
    ops.visibility_accumulate_(spec, params, dens, ro, rd, mw, mt)
    rw, rt = visibility_ref.visibility(spec, params, dens, feat, ro, rd)
    if miss:
        assert int(rw.count_nonzero()) == 0 and int(rt.count_nonzero()) == 0
        assert torch.equal(mw, pre[0]) and torch.equal(mt, pre[1])
        return
    err_w, err_t = float((mw.double() - rw).abs().max()), float((mt.double() - rt).abs().max())
    print(f"{name}: max|max_weight - ref| {err_w:.3e}  max|max_trans - ref| {err_t:.3e}")
    assert err_w <= 1e-5 and err_t <= 1e-5
    assert bool((mw[rw == 0] == 0).all()) and bool((mt[rt == 0] == 0).all())
    assert float(rw.max()) > 0.01 and float(mt.max()) == 1.0            # the first inside sample arrives with T = 1
    assert bool(torch.isfinite(mw).all()) and float(mw.min()) >= 0 and float(mw.max()) <= 1


@pytest.mark.parametrize("name", dc.SIDE_CASES)
def test_distortion_matches_the_restatement(name):
    import distortion_ref as DR

    r, c, spec, params, dens, feat, ro, rd = _side_inputs(name)
    L64, g64 = DR.loss_and_gradient(DR.distortion, spec, params, dens, feat, ro, rd)
    with torch.no_grad():
        L32 = DR.distortion(spec, params, dens, feat, ro, rd, dtype=torch.float32)
    yard_ray = float((L32.double() - L64).abs().max())
    yard_loss = abs(float(L32.mean()) - float(L64.mean()))
    bound_ray, bound_loss = max(4.0 * yard_ray, 1e-6), max(4.0 * yard_loss, 1e-6)
    miss = bool(c.need.get("miss"))
    assert miss == (float(L64.abs().max()) == 0.0) and miss == (float(g64.norm()) == 0.0)
    for lanes in (0, 1, 2, 4, 8):
        d = torch.full_like(dens, float("nan"))
        loss, ray = ops.distortion_fwd_bwd(spec, params, dens, ro, rd, None, (0, 0), grad_scale=1.0, want_loss=True, want_ray_loss=True,
                                           d_densities=d, accumulate=False, lanes=lanes)
        err_ray = float((ray.double() - L64).abs().max())
        err_loss = abs(float(loss) - float(L64.mean()))
        err_g = float((d.double() - g64).norm() / g64.norm()) if not miss else float(d.abs().max())
        print(f"{name} lanes {lanes}: ray_loss err {err_ray:.3e} (bound {bound_ray:.3e})  loss err {err_loss:.3e} (bound {bound_loss:.3e})  "
              f"grad rel_l2 {err_g:.3e}")
        assert err_ray <= bound_ray and err_loss <= bound_loss, (lanes, err_ray, err_loss)
        assert err_g < 1e-4, (lanes, err_g)
        assert bool((ray[L64 == 0] == 0).all()) and bool((d[g64 == 0] == 0).all())      # empty rays / untouched voxels: exact 0
        assert bool(torch.isfinite(ray).all()) and bool(torch.isfinite(d).all())
        if miss:
            assert float(loss) == 0.0 and int(ray.count_nonzero()) == 0 and int(d.count_nonzero()) == 0
