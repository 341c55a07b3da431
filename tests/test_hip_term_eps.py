"""Gradient truncation (VoxeRenderCfg::term_eps) through every backward that implements it, HIP vs the TRUNCATED oracle: the case
table of tests/term_eps_cases.py (dense fields, eps = 0.1 / 0.5 where moving a ray's cut by ONE sample changes the gradient by at
least 10 x the tolerance, and eps = 1e-3 as the realistic setting).  The rule (include/voxe.h): sample k of a ray receives its exact
gradient iff the transmittance in front of it is >= term_eps.  The reference is vo.render_bwd(..., cut=cut(eps)) with the cut
worked out from the oracle's probe in float64; rays whose cut depends on the last 1e-3 of the threshold carry no upstream gradient.

Tolerance: tests/test_hip_fuzz.py's _close (1e-4 rel-L2 + its absolute floor, x max(1, far) on the density gradient under a depth
gradient).  Every test prints its error, the reference's norm and the two off-by-one margins of its case, checks the case's
conditions again (tests/test_oracle_term_eps.py does so on the CPU) and asserts once that the forward does not see term_eps."""
import ctypes as C

import numpy as np
import pytest
import torch

import term_eps_cases as tc
from test_hip_degenerate_rays import ROUTES as ALL_ROUTES, TILE
from test_hip_fuzz import _close
from voxe_hip import abi

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import gpu_helpers as gh
    from voxe_hip import ops
    from voxe_hip.runtime import lib

# the rows of tests/test_hip_degenerate_rays.py's table that can take term_eps (the space-binned rows refuse it: see the region test)
ROUTES = {k: v for k, v in ALL_ROUTES.items() if not k.startswith("region")}
SH0_CASES = tc.ROUTE_CASES + ("attn_relu_s64_e0.1",)
UNORDERED_CASES = SH0_CASES + ("sp_s64_jitter_tensor_e0.1",)


def _hip_route(r, **over):
    c = r["case"]
    params = gh.params_of(r["cfg"], **{**r["over"], **over})
    g, cf = ops._descs(gh.spec_of(r["grid"]), params, gh.t(r["grid"].densities), gh.t(r["grid"].features), c.rng[0], c.rng[1], False)
    return ops._route(g, cf, r["o"].shape[0])


def _start(r):
    """the case's conditions on the oracle's figures, and the forward with and without term_eps: every output bit equal"""
    c = r["case"]
    tc.check_conditions(r)
    args = (r["grid"], r["cfg"], r["o"], r["d"])
    a = gh.hip_forward(*args, r["jit"], rng=c.rng, **r["over"])
    b = gh.hip_forward(*args, r["jit"], rng=c.rng, term_eps=c.eps, **r["over"])
    for k in ("colour", "depth", "acc", "disparity"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    return args


def _backward(r, **over):
    c = r["case"]
    return gh.hip_backward(r["grid"], r["cfg"], r["o"], r["d"], r["gc"], g_depth=r["gdep"], g_acc=r["gacc"], jitter=r["jit"],
                           rng=c.rng, **{**r["over"], "term_eps": c.eps, **over})


def _check(r, got, what=""):
    minus, plus = tc.margins(r)
    far = r["cfg"].far if r["gdep"] is not None else 1.0
    for i, name in enumerate(("densities", "features")):
        ref_g = r["bwd"][i]
        err = float(np.linalg.norm(got[i].astype(np.float64) - ref_g.astype(np.float64)))
        print(f"{r['case'].name} deg {r['deg']} {what} {name}: |err| {err:.3e}  |ref| {float(np.linalg.norm(ref_g)):.3e}  tol {r['tol'][i]:.3e}  "
              f"|G(cut)-G(cut-1)| {minus[i]:.3e}  |G(cut)-G(cut+1)| {plus[i]:.3e}")
    for i, name in enumerate(("densities", "features")):
        _close(name, got[i], r["bwd"][i], far=far if name == "densities" else 1.0)


# ---- SH-0 and attention grids: colour + depth + acc gradients through every image-ordered route ---------------------------------
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", SH0_CASES)
def test_truncated_gradient_through_route(name, route, disp):
    fields, order, want_route = ROUTES[route]
    r = tc.reference(name, order)
    disp.set(**fields)
    det = dict(deterministic=True) if route == "deterministic" else {}
    assert _hip_route(r, term_eps=r["case"].eps, **det) == want_route
    _start(r)
    got = _backward(r, **det)
    _check(r, got, route)
    if route == "deterministic":
        again = _backward(r, **det)
        assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1])


def _region_to_gradients(region, layout, grid):
    """the workspace's gradient region -> (d_densities, d_features), like tests/test_hip_fused_step.py: de-brick (2x2x2 bricks of
    [features, density] texels), split the channels, chain rule of the (identity) density pre-activation"""
    X, Y, Z = grid.densities.shape[:3]
    C = grid.features.shape[-1] + 1
    if layout == abi.GRAD_BRICKED:
        by, bz = (Y + 1) // 2, (Z + 1) // 2
        x, y, z = np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij")
        slot = ((((x // 2) * by + (y // 2)) * bz + (z // 2)) * 8) + (x % 2) * 4 + (y % 2) * 2 + (z % 2)
        g = region.reshape(-1, C)[slot.reshape(-1)].reshape(X, Y, Z, C)
    else:
        g = region[: X * Y * Z * C].reshape(X, Y, Z, C)
    return g[..., C - 1:] * np.float32(grid.density_scale), g[..., : C - 1]


@pytest.mark.parametrize("linear_grad", [False, True])
@pytest.mark.parametrize("name", UNORDERED_CASES)
def test_truncated_gradient_of_an_unordered_batch_in_both_gradient_layouts(name, linear_grad):
    """the same rays permuted, image_width = 0: the line-dense scatter (its segment-start skip and its in-march stop), leaving its
    gradient in the workspace in 2x2x2 bricks or, with linear_grad, in the linear layout"""
    r = tc.reference(name, "permuted")
    c, grid = r["case"], r["grid"]
    assert _hip_route(r, term_eps=c.eps) == abi.ROUTE_PACKED_SCATTER
    _start(r)
    spec, params = gh.spec_of(grid), gh.params_of(r["cfg"], term_eps=c.eps, image_width=0, linear_grad=linear_grad)
    td, tf, to, tdir = gh.t(grid.densities), gh.t(grid.features), gh.t(r["o"]), gh.t(r["d"])
    R = r["o"].shape[0]
    outs = [torch.empty((R, n), device=gh.DEV) for n in (grid.cout, 1, 1, 1)]
    ws = ops.Workspace()
    ops.render_fwd_into(spec, params, td, tf, to, tdir, gh.t(r["jit"]), *outs, ws, c.rng)
    layout = ops.render_bwd_acc(spec, params, td, tf, to, tdir, gh.t(r["jit"]), outs[0], outs[1], outs[2], gh.t(r["gc"]),
                                gh.t(r["gdep"].reshape(R, 1)), gh.t(r["gacc"].reshape(R, 1)), ws, c.rng)
    assert layout == (abi.GRAD_LINEAR if linear_grad else abi.GRAD_BRICKED)
    torch.cuda.synchronize()
    got = _region_to_gradients(gh.n(ops.workspace_grad_view(spec, td, tf, ws)), layout, grid)
    _check(r, got, "unordered " + ("linear" if linear_grad else "bricked"))
    if not linear_grad:     # and through the autograd binding (voxe_render_bwd: the same kernel + the un-pack)
        _check(r, _backward(r), "unordered")


# ---- view-dependent grids: colour gradients ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["two_phase", "single_kernel", "scatter_unordered"])
@pytest.mark.parametrize("deg", [1, 2, 3])
@pytest.mark.parametrize("name", tc.SH_CASES)
def test_truncated_gradient_of_view_dependent_grids(name, deg, mode, disp):
    """the two-phase window backward (its source pass goes `dead` and keeps writing zeros), the channel groups that re-march
    (tile_two_phase = -1) and the scatter on unordered rays"""
    r = tc.reference(name, "permuted" if mode == "scatter_unordered" else "image", deg)
    if mode != "scatter_unordered":
        disp.set(region_min_rays=-1, tile_two_phase=-1 if mode == "single_kernel" else 0, **TILE)
        assert _hip_route(r, term_eps=r["case"].eps) == abi.ROUTE_TILE
    _start(r)
    _check(r, _backward(r), mode)


def test_truncated_gradient_of_a_view_dependent_grid_rendered_diffuse(disp):
    r = tc.reference("sp_s64_e0.1", "image", 2, True)
    disp.set(region_min_rays=-1, **TILE)
    _start(r)
    got = _backward(r)
    _check(r, got, "diffuse")
    per_colour = got[1].reshape(got[1].shape[:3] + (3, 9))
    assert not per_colour[..., 1:].any() and per_colour[..., 0].any()


# ---- several views in one launch, and the 32-sample depth segments of launches above 20 000 rays --------------------------------------
@pytest.mark.parametrize("route", ["shipped", "lean_tile", "general_tile", "plain_scatter"])
def test_truncated_gradient_of_two_views_in_one_launch(route, disp):
    fields, _, want_route = ROUTES[route]
    r = tc.reference("two_views_s64_e0.5")
    assert r["over"]["image_height"] == r["case"].hw and r["o"].shape[0] == 2 * r["case"].hw ** 2
    disp.set(**fields)
    assert _hip_route(r, term_eps=r["case"].eps) == want_route
    _start(r)
    _check(r, _backward(r), route)


@pytest.mark.parametrize("route", ["shipped", "general_tile", "precise", "plain_scatter", "unordered"])
def test_truncated_gradient_with_32_sample_segments(route, disp):
    """144 x 144 rays: above VOXE_SEG16_MAX_RAYS the depth segments hold 32 samples (cuts at k % 32 = 0, 1, 31 are in the case)"""
    r = tc.reference("big_144_s64_e0.1", "permuted" if route == "unordered" else "image")
    assert r["case"].seg_len == 32 and r["o"].shape[0] > tc.SEG16_MAX_RAYS
    if route != "unordered":
        disp.set(**ROUTES[route][0])
    if route not in ("unordered", "shipped"):
        assert _hip_route(r, term_eps=r["case"].eps) == ROUTES[route][2]
    _start(r)
    _check(r, _backward(r), route)


@pytest.mark.parametrize("route", ["shipped", "lean_tile", "general_tile", "precise", "deterministic", "unordered"])
def test_truncated_gradient_with_a_caller_s_jitter_tensor(route, disp):
    """a jitter tensor instead of the in-kernel stream (the forward then keeps no double segment sums for the `precise` backward:
    its states come from another source)"""
    r = tc.reference("sp_s64_jitter_tensor_e0.1", "permuted" if route == "unordered" else "image")
    assert r["jit"] is not None
    det = dict(deterministic=True) if route == "deterministic" else {}
    if route != "unordered":
        disp.set(**ROUTES[route][0])
        assert _hip_route(r, term_eps=r["case"].eps, **det) == ROUTES[route][2]
    _start(r)
    _check(r, _backward(r, **det), route)


@pytest.mark.parametrize("frozen", ["features", "densities"])
@pytest.mark.parametrize("route", ["shipped", "lean_tile", "general_tile", "plain_scatter"])
def test_truncated_gradient_with_one_tensor_frozen(route, frozen, disp):
    """the kernels' density-only / features-only instantiations stop at the same sample"""
    r = tc.reference("relu_s64_e0.5")
    c, grid = r["case"], r["grid"]
    disp.set(**ROUTES[route][0])
    _start(r)
    dt, ft = gh.t(grid.densities, frozen != "densities"), gh.t(grid.features, frozen != "features")
    col, dep, acc, _ = ops.render(gh.spec_of(grid), gh.params_of(r["cfg"], term_eps=c.eps, **r["over"]), dt, ft, gh.t(r["o"]), gh.t(r["d"]),
                                  None, rng=c.rng)
    ((col * gh.t(r["gc"])).sum() + (dep[:, 0] * gh.t(r["gdep"])).sum() + (acc[:, 0] * gh.t(r["gacc"])).sum()).backward()
    torch.cuda.synchronize()
    i, live = (0, dt) if frozen == "features" else (1, ft)
    assert (ft if frozen == "features" else dt).grad is None
    err = float(np.linalg.norm(gh.n(live.grad).astype(np.float64) - r["bwd"][i]))
    print(f"{c.name} {route} {frozen} frozen: |err| {err:.3e}  |ref| {float(np.linalg.norm(r['bwd'][i])):.3e}  tol {r['tol'][i]:.3e}")
    _close(frozen + " frozen", gh.n(live.grad), r["bwd"][i], far=r["cfg"].far if i == 0 else 1.0)


# ---- the route planner: the space-binned route refuses term_eps > 0 ----------------------------------------------------------------
@pytest.mark.parametrize("row", ["region_unordered", "region_image"])
@pytest.mark.parametrize("name", ["sp_s64_e0.1", "relu_s97_clip_e0.5"])
def test_the_region_route_is_refused_and_the_gradient_still_truncated(name, row, disp):
    fields, order, want_route = ALL_ROUTES[row]
    r = tc.reference(name, order)
    disp.set(**fields)
    assert want_route == abi.ROUTE_REGION and _hip_route(r, term_eps=0.0) == abi.ROUTE_REGION
    assert _hip_route(r, term_eps=r["case"].eps) != abi.ROUTE_REGION
    _start(r)
    _check(r, _backward(r), row)


# ---- a backward that cannot reuse the forward's ray states ---------------------------------------------------------------------------
@pytest.mark.parametrize("deg", [0, 1])
@pytest.mark.parametrize("name", ["sp_s64_e0.1", "sp_s33_e0.5"])
def test_a_re_march_gives_the_same_truncated_gradient(name, deg, disp):
    """as tests/test_hip_configs.py's ray-state tests: an honest forward + backward, an inference forward followed by a backward
    whose caller claims ray_state_valid = 1 (the library checks the claim and re-marches), and a backward alone -- the segment-start
    skip then reads states the backward itself recomputed"""
    r = tc.reference(name, "image", deg)
    c, grid = r["case"], r["grid"]
    disp.set(region_min_rays=-1, **TILE)
    _start(r)
    spec, params = gh.spec_of(grid), gh.params_of(r["cfg"], term_eps=c.eps, **r["over"])
    td, tf, to, tdir, tg = gh.t(grid.densities), gh.t(grid.features), gh.t(r["o"]), gh.t(r["d"]), gh.t(r["gc"])
    R = r["o"].shape[0]
    tdep = None if r["gdep"] is None else gh.t(r["gdep"].reshape(R, 1))
    tacc = None if r["gacc"] is None else gh.t(r["gacc"].reshape(R, 1))
    outs = [torch.empty((R, n), device=gh.DEV) for n in (3, 1, 1, 1)]
    g_, c_ = ops._descs(spec, params, td, tf, c.rng[0], c.rng[1], False)
    nbytes = lib().voxe_workspace_bytes(C.byref(g_), C.byref(c_), R)       # the size a training caller allocates
    for mode in ("honest", "inference_forward", "backward_alone"):
        ws = ops.Workspace()
        ws.ensure(nbytes, td.device).fill_(0xFF)        # (NaN bit patterns wherever a kernel reads what nobody wrote)
        ops.render_fwd_into(spec, params, td, tf, to, tdir, None, *outs, ws, c.rng, keep_for_backward=(mode == "honest"))
        if mode == "inference_forward":
            assert ws.state_key is None
            ws.remember_states(ops._state_key(ops._pack_key(spec, td, tf), params, to, tdir, None, c.rng, ops._route(g_, c_, R)), to, tdir, None)
        elif mode == "backward_alone":
            ws.invalidate()
        d_d, d_f = torch.zeros_like(td), torch.zeros_like(tf)
        ops.render_bwd_into(spec, params, td, tf, to, tdir, None, outs[0], outs[1], outs[2], tg, tdep, tacc, d_d, d_f, ws, c.rng)
        torch.cuda.synchronize()
        _check(r, (gh.n(d_d), gh.n(d_f)), mode)
