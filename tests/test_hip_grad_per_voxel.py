"""Every backward route voxel by voxel, HIP vs the oracle: the case table of tests/grad_budget_cases.py through tests/helpers.py's
per_voxel_check -- |got - ref| <= eps32 * (budget + count * mag) + floor at EVERY density voxel and EVERY feature value, with the
budget twin of the oracle (oracle/voxe_cpu.c: voxe_cpu_render_bwd_budget) saying how much float32 error is legitimate there.  The
global rel-L2 the suite had (tests/test_hip_fuzz.py's _close) is asserted beside it; what it does not see -- a lost grid face, a
dropped trilinear corner of the faint voxels, an unflushed part of a split tile, a skipped channel group -- the per-voxel bound
flags (shown on the oracle alone by tests/test_grad_budget_host.py, which also checks the table's preconditions and pins the
budget's constants against the reference's own float32 gradients; they are not fitted to a kernel).

Every test prints the largest ratio |got - ref| / bound per tensor and the voxel it occurs at (-s)."""
import numpy as np
import pytest
import torch

import grad_budget_cases as gb
from test_hip_degenerate_rays import ROUTES, TILE
from voxe_hip import abi

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import gpu_helpers as gh
    from voxe_hip import ops


def _hip_route(r, **over):
    c, grid = r["case"], r["grid"]
    params = gh.params_of(r["cfg"], **{**r["over"], **over})
    g, cf = ops._descs(gh.spec_of(grid), params, gh.t(grid.densities), gh.t(grid.features), c.rng[0], c.rng[1], False)
    return ops._route(g, cf, r["o"].shape[0])


def _backward(r, which, **over):
    c, up = r["case"], r["sets"][which]
    return gh.hip_backward(r["grid"], r["cfg"], r["o"], r["d"], up["gc"], g_depth=up["gdep"], g_acc=up["gacc"], jitter=r["jit"], rng=c.rng,
                           **{**r["over"], **over})


def _run(r, what, exempt_cap=(0.01, 0.01), **over):
    """both upstream sets of the case through the launch the caller has set up; the exempt share (densities, features) stays under
    the case's cap: 1 % unless the case table states another for the scene, with its cause (tests/grad_budget_cases.py).
    (`what` starts with the route's name: the plain scatter and the deterministic backward have a term of their own in the bound)"""
    for which in r["sets"]:
        shares = gb.check_gradients(r, which, _backward(r, which, **over), what, route=what.split(",")[0])
        assert shares[0] <= exempt_cap[0] and shares[1] <= exempt_cap[1], (what, which, shares)


# ---- SH-0 grids: every scene through every route ------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", gb.SCENES)
def test_scene_through_route(name, route, disp):
    fields, order, want_route = ROUTES[route]
    r = gb.reference(name, order)
    disp.set(**fields)
    det = dict(deterministic=True) if route == "deterministic" else {}
    assert _hip_route(r, **det) == want_route
    _run(r, route, gb.NEED[name]["exempt"], **det)


# ---- other fields and channel kinds -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["lean_tile", "region_unordered", "region_image", "shipped"])
@pytest.mark.parametrize("name", ["relu", "abs"])
def test_relu_and_abs_fields(name, route, disp):
    fields, order, want_route = ROUTES[route]
    r = gb.reference(name, order)
    disp.set(**fields)
    assert _hip_route(r) == want_route
    _run(r, route)


@pytest.mark.parametrize("route", ["general_tile", "deterministic"])
def test_attention_grid(route, disp):
    fields, order, want_route = ROUTES[route]
    r = gb.reference("attn", order)
    disp.set(**fields)
    det = dict(deterministic=True) if route == "deterministic" else {}
    assert _hip_route(r, **det) == want_route
    _run(r, route, **det)


def test_a_caller_s_jitter_tensor_on_the_tile_route(disp):
    """a jitter tensor selects the general tile kernel (the lean kernels draw the in-kernel stream)"""
    r = gb.reference("jitter_tensor")
    assert r["jit"] is not None
    disp.set(**TILE)
    assert _hip_route(r) == abi.ROUTE_TILE
    _run(r, "tile, jitter tensor")


@pytest.mark.parametrize("route", ["lean_tile", "region_image"])
def test_two_cameras_in_one_launch(route, disp):
    fields, order, want_route = ROUTES[route]
    r = gb.reference("two_views", order)
    c = r["case"]
    assert r["over"]["image_height"] == c.H and r["o"].shape[0] == 2 * c.H * c.W
    disp.set(**fields)
    assert _hip_route(r) == want_route
    _run(r, route)


@pytest.mark.parametrize("route", ["shipped", "plain_scatter"])
def test_saturated_interior_samples(route, disp):
    """S = 7 across an opaque field: samples with om == 0 and e != 0 in the middle of a ray.  The two kernels that march one ray per
    lane (the line-dense scatter and the plain scatter) re-march the rest of such a ray for the term `suffix / om` has lost
    (saturated_correction() in csrc/voxe_render_common.hpp).
    KNOWN: the tile kernels, the space-binned kernels and the deterministic backward still take tail = 0 at such a sample -- their
    lanes do not own a ray's whole march -- and are over the bound on this case (the missing deposit delta e tail is up to 1e-10 of
    the largest gradient and 1e4 x the bound of a voxel that holds nothing else); the case is therefore not a row of SCENES."""
    fields, order, want_route = ROUTES[route]
    r = gb.reference("saturated", order)
    disp.set(**fields)
    assert _hip_route(r) == want_route
    _run(r, route, exempt_cap=(0.04, 0.01))     # (opaque: 3.13 % of the touched densities lie behind T < 1e-20, 0.42 % of the features)


@pytest.mark.parametrize("route", ["lean_tile", "plain_scatter", "region_unordered"])
def test_truncated_gradient(route, disp):
    """term_eps = 1e-2 against the twin given the same cut (tests/term_eps_cases.py derives it; rays it cannot decide carry no
    upstream gradient).  The space-binned route refuses term_eps (tests/test_hip_term_eps.py): the planner sends that launch
    elsewhere and the gradient is truncated all the same."""
    fields, order, want_route = ROUTES[route]
    r = gb.reference("dense_eps1e-2", order)
    eps = r["case"].eps
    disp.set(**fields)
    if want_route == abi.ROUTE_REGION:
        assert _hip_route(r) == abi.ROUTE_REGION and _hip_route(r, term_eps=eps) != abi.ROUTE_REGION
    else:
        assert _hip_route(r, term_eps=eps) == want_route
    _run(r, f"{route}, term_eps {eps:g}", term_eps=eps)


# ---- view-dependent grids: every feature channel ------------------------------------------------------------------------------------------
SH_MODES = {
    # name -> (dispatch fields, ray order, route or None)
    "two_phase_lean": (dict(TILE, region_min_rays=-1), "image", abi.ROUTE_TILE),
    "two_phase_general": (dict(TILE, region_min_rays=-1, tile_lean=-1), "image", abi.ROUTE_TILE),
    "single_kernel": (dict(TILE, region_min_rays=-1, tile_two_phase=-1), "image", abi.ROUTE_TILE),
    "region": (dict(region_min_rays=1), "permuted", abi.ROUTE_REGION),
    "scatter_unordered": (dict(region_min_rays=-1), "permuted", None),
}


@pytest.mark.parametrize("mode", list(SH_MODES))
@pytest.mark.parametrize("name", gb.SH_CASES)
def test_view_dependent_grid(name, mode, disp):
    """degree 1, 2, 3 and degree 2 rendered diffuse: all 12 / 27 / 48 feature values of a voxel against their own bound -- a skipped
    4-channel group of a faint voxel fails"""
    fields, order, want_route = SH_MODES[mode]
    r = gb.reference(name, order)
    disp.set(**fields)
    route = _hip_route(r)
    if want_route is None:
        assert route not in (abi.ROUTE_REGION, abi.ROUTE_TILE), route
    else:
        assert route == want_route
    got = _backward(r, "colour")
    shares = gb.check_gradients(r, "colour", got, mode)
    assert max(shares) <= 0.01, (mode, shares)
    if r["case"].diffuse:       # only the constant coefficient of each colour receives gradient: exact zeros elsewhere
        per_colour = got[1].reshape(got[1].shape[:3] + (3, 9))
        assert not per_colour[..., 1:].any() and per_colour[..., 0].any()
