"""Do the values of a grid that changed reach the kernels?  Every render, query and fused step first packs the grid into its
workspace and skips that pass when the workspace says it holds the grid already; the backward likewise takes the forward's ray
states.  A false hit raises nothing -- the kernels run correctly on the PREVIOUS grid -- so no comparison of one call against the
oracle sees it.  Here every row of tests/cache_cases.py runs through every entry point that asks the caches:

    call through a persistent workspace -> change -> the same call through the SAME workspace

and the second call must equal, bit for bit, the same call through a fresh Workspace() on the current values (gradients: bit for bit
under `deterministic` for SH-0 and attention grids; SH-1 to rel-L2 1e-5, the figure tests/test_hip_r06.py uses for two runs that
differ in the order of float atomics), the fresh call must match the CPU oracle on the current values, and the two calls must differ
by far more than any tolerance (max |delta| > 1e-2: a stale result would otherwise pass).  Then the library's own in-place writers,
the ray-state cache, and -- so that "never cache" is no way to pass -- the pack counts of the library's profiler.

Shapes: 20 x 24 x 28 grids (SH-0, SH-1 with its wide-texel pack, attention) in [-1.5, 1.5]^3, softplus field at scale 3, the 32 x 40
image of camera 38 of the synthetic set, S = 48 with in-kernel jitter, 777 query points."""
import copy
import dataclasses
import functools

import numpy as np
import pytest
import torch

import cache_cases as cc
from helpers import rel_l2
from synth import FAR, NEAR, RADIUS, focal_for, synth_pose_angles
from voxe_hip import abi
from voxe_hip.desc import make_render_cfg

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import gpu_helpers as gh
    from oracle import voxe_oracle as vo
    from thre3d_atom.utils.imaging_utils import pose_spherical
    from voxe_hip import ops
    from voxe_hip.runtime import f32c

    DEV = gh.DEV

H, W, S, CAM = 32, 40, 48, 38
R = H * W
RNG = (42, 7)
VISIBLE = 1e-2


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rays_np(cam=CAM):
    p = pose_spherical(*synth_pose_angles(cam, 100), RADIUS)
    return vo.cast_rays(H, W, focal_for(W), p.rotation.numpy(), p.translation.numpy())


def _rays(cam=CAM):
    o, d = _rays_np(cam)
    return {"rays_o": gh.t(o), "rays_d": gh.t(d), "jitter": None}


@functools.lru_cache(maxsize=None)
def _upstream(cout):
    g = torch.Generator().manual_seed(17 + cout)
    return (torch.randn((R, cout), generator=g).to(DEV), (0.2 * torch.randn((R, 1), generator=g)).to(DEV),
            (0.2 * torch.randn((R, 1), generator=g)).to(DEV))


@functools.lru_cache(maxsize=None)
def _points_np():
    rng = np.random.default_rng(300)
    lo, hi = np.full(3, -1.5), np.full(3, 1.5)
    pts = (lo + (hi - lo) * rng.uniform(-0.2, 1.2, (777, 3))).astype(np.float32)
    pts[:8] = np.array([[lo[0], lo[1], lo[2]], [hi[0], hi[1], hi[2]], [lo[0], hi[1], lo[2]], (lo + hi) / 2,
                        [lo[0], (lo[1] + hi[1]) / 2, hi[2]], lo - 1, hi + 1, [hi[0], lo[1], lo[2]]], np.float32)
    return pts


def _cout(o):
    return 1 if o.spec.feature_kind == abi.FEAT_ATTN else 3


def _params(o, **over):
    # (the fixed-point backward exists for SH-0 and attention grids: bit-reproducible gradients)
    return ops.RenderParams(num_samples=S, near=NEAR, far=FAR, perturb=True, white_bkgd=True, sh_degree=o.sh_degree, image_width=W,
                            deterministic=(o.sh_degree == 0), **over)


def _dense(o):
    return f32c(o.densities.detach()), f32c(o.features.detach())


# ---- the entry points: each returns {name: tensor} of one call through `ws` --------------------------------------------------------
def _render_forward(o, ws, r, detach=False):
    """forward alone.  `detach`: on plain tensors, as an inference caller holds them (a grid that requires grad is a
    differentiable forward to ops.render even under no_grad: it keeps its states, and a second one before any backward runs in
    the workspace's sibling)"""
    dens, feat = (o.densities.detach(), o.features.detach()) if detach else (o.densities, o.features)
    with torch.no_grad():
        c, d, a, _ = ops.render(o.spec, _params(o), dens, feat, r["rays_o"], r["rays_d"], r["jitter"], workspace=ws, rng=RNG)
    return {"colour": c, "depth": d, "acc": a}


def _render_forward_backward(o, ws, r):
    gc_, gd_, ga_ = _upstream(_cout(o))
    o.densities.grad = o.features.grad = None
    c, d, a, _ = ops.render(o.spec, _params(o), o.densities, o.features, r["rays_o"], r["rays_d"], r["jitter"], workspace=ws, rng=RNG)
    loss = (c * gc_).sum()
    if o.sh_degree == 0:        # (view-dependent grids: colour gradients only, as everywhere in the suite)
        loss = loss + (d * gd_).sum() + (a * ga_).sum()
    loss.backward()
    out = {"colour": c.detach(), "depth": d.detach(), "acc": a.detach(), "d_densities": o.densities.grad.float().clone(),
           "d_features": o.features.grad.float().clone()}
    o.densities.grad = o.features.grad = None
    return out


def _outs(o):
    return [torch.empty((R, n), dtype=torch.float32, device=DEV) for n in (_cout(o), 1, 1, 1)]


def _into(o, ws, r):
    """render_fwd_into + render_bwd_into, as a caller of the raw entry points holds its tensors: dense float32 copies of its own
    where the grid is not dense float32 (temporaries, gone after the call)"""
    dens, feat = _dense(o)
    p = _params(o)
    gc_, gd_, ga_ = _upstream(_cout(o))
    outs = _outs(o)
    ops.render_fwd_into(o.spec, p, dens, feat, r["rays_o"], r["rays_d"], r["jitter"], *outs, ws, RNG)
    dd, df = torch.empty_like(dens), torch.empty_like(feat)
    flat = o.sh_degree == 0
    ops.render_bwd_into(o.spec, p, dens, feat, r["rays_o"], r["rays_d"], r["jitter"], outs[0], outs[1], outs[2], gc_,
                        gd_ if flat else None, ga_ if flat else None, dd, df, ws, RNG)
    return {"colour": outs[0], "depth": outs[1], "acc": outs[2], "d_densities": dd, "d_features": df}


def _bwd_acc(o, ws, r):
    """render_fwd_into + render_bwd_acc: the gradient stays in the workspace (kernel layout)"""
    dens, feat = _dense(o)
    p = _params(o)
    gc_, gd_, ga_ = _upstream(_cout(o))
    outs = _outs(o)
    ops.render_fwd_into(o.spec, p, dens, feat, r["rays_o"], r["rays_d"], r["jitter"], *outs, ws, RNG)
    flat = o.sh_degree == 0
    layout = ops.render_bwd_acc(o.spec, p, dens, feat, r["rays_o"], r["rays_d"], r["jitter"], outs[0], outs[1], outs[2], gc_,
                                gd_ if flat else None, ga_ if flat else None, ws, RNG, zero_first=True)
    region = ops.workspace_grad_view(o.spec, dens, feat, ws).clone()
    return {"colour": outs[0], "depth": outs[1], "acc": outs[2], "d_region": region,
            "layout": torch.tensor([layout])}


def _query(o, ws, r=None):
    pts = gh.t(_points_np())
    o.densities.grad = o.features.grad = None
    out = ops.query_points(o.spec, o.densities, o.features, pts, workspace=ws)
    g = torch.Generator().manual_seed(23)
    (out * torch.randn(out.shape, generator=g).to(DEV)).sum().backward()
    res = {"query": out.detach(), "d_densities": o.densities.grad.float().clone(), "d_features": o.features.grad.float().clone()}
    o.densities.grad = o.features.grad = None
    return res


# ---- comparisons ------------------------------------------------------------------------------------------------------------------
def _same(got, want, exact_gradients, what):
    """the second call through the persistent workspace against the fresh one: forwards bit for bit, gradients bit for bit under
    the fixed-point backward, else to the float-atomics figure"""
    for k in want:
        a, b = got[k], want[k]
        assert a.shape == b.shape, (what, k, a.shape, b.shape)
        if k.startswith("d_") and not exact_gradients:
            rel = rel_l2(gh.n(a), gh.n(b))
            print(f"{what} {k}: rel-L2 to the fresh workspace {rel:.3e}")
            assert rel < 1e-5, (what, k, rel)
        else:
            assert torch.equal(a, b), (f"{what} {k}: {int((a != b).sum())} of {a.numel()} differ from the fresh workspace, "
                                       f"max {float((a.float() - b.float()).abs().max()):.3e}")


def _visible(first, second, what, keys=("colour", "query")):
    """the change shows in every one of `keys` the call returned: a stale second call would equal the first"""
    deltas = {k: float("inf") if first[k].shape != second[k].shape else float((first[k] - second[k]).abs().max())
              for k in keys if k in first}
    print(f"{what}: max |delta| between the two calls {deltas}")
    assert deltas and min(deltas.values()) > VISIBLE, (what, deltas)


def _oracle_grid(o):
    dens, feat = _dense(o)
    return vo.Grid(gh.n(dens), gh.n(feat), [tuple(a) for a in o.spec.aabb], o.spec.density_scale, o.spec.density_pre_act,
                   o.spec.density_post_act, o.spec.feature_kind)


def _check_forward_vs_oracle(o, out, r, rng=RNG):
    from test_hip_configs import _check_forward

    cfg = make_render_cfg(S, NEAR, FAR, perturb=True, white_bkgd=True, sh_degree=o.sh_degree, seed=rng[0], rng_offset=rng[1])
    ref = vo.render_fwd(_oracle_grid(o), cfg, gh.n(r["rays_o"]), gh.n(r["rays_d"]),
                        jitter=None if r["jitter"] is None else gh.n(r["jitter"]))
    _check_forward({"colour": gh.n(out["colour"]), "depth": gh.n(out["depth"])[:, 0], "acc": gh.n(out["acc"])[:, 0]}, ref)


def _check_query_vs_oracle(o, out):
    np.testing.assert_allclose(gh.n(out["query"]), vo.query_fwd(_oracle_grid(o), _points_np()), rtol=3e-6, atol=3e-6)


def _two_calls(call, name, kind, what, exact_gradients=True):
    """call -> change -> call through one workspace; the second call against a fresh workspace; returns (owner, fresh result)"""
    change = cc.BY_NAME[name]
    o = cc.make_owner(kind, change.source, DEV)
    r = _rays()
    ws = ops.Workspace()
    first = {k: v.clone() for k, v in call(o, ws, r).items()}
    change.apply(o)
    second = {k: v.clone() for k, v in call(o, ws, r).items()}
    fresh = call(o, ops.Workspace(), r)
    _same(second, fresh, exact_gradients and o.sh_degree == 0, f"{what} [{name}-{kind}]")
    _visible(first, second, f"{what} [{name}-{kind}]")
    return o, r, fresh


ROWS = cc.rows(gpu_only=True)


# ---- every row through every entry point ------------------------------------------------------------------------------------------
# (the LDS-window kernels are SH-0 kernels: the `tile` variants run the SH-0 rows)
ROUTED_ROWS = [(n, k, route) for n, k in ROWS for route in ("shipped", "tile") if route == "shipped" or k == "sh0"]


@pytest.mark.parametrize("name,kind,route", ROUTED_ROWS)
def test_render_sees_the_change(name, kind, route, disp):
    """ops.render, forward alone (no states kept) and forward + backward; `tile`: the LDS-window kernels instead of the scatter
    route a 1280-ray image takes as shipped"""
    if route == "tile":
        disp.set(tile_min_rays=-1)
    # (on plain tensors: a grid that requires grad would send the second forward to the workspace's sibling, which never held
    #  the old grid)
    o, r, fresh = _two_calls(functools.partial(_render_forward, detach=True), name, kind, "render forward")
    _check_forward_vs_oracle(o, fresh, r)
    _two_calls(_render_forward_backward, name, kind, "render forward + backward")


@pytest.mark.parametrize("name,kind", ROWS)
def test_render_into_sees_the_change(name, kind):
    o, r, fresh = _two_calls(_into, name, kind, "render_fwd_into + render_bwd_into")
    _check_forward_vs_oracle(o, fresh, r)


@pytest.mark.parametrize("name,kind", ROWS)
def test_render_bwd_acc_sees_the_change(name, kind):
    _two_calls(_bwd_acc, name, kind, "render_fwd_into + render_bwd_acc")


@pytest.mark.parametrize("name,kind", ROWS)
def test_query_sees_the_change(name, kind):
    # (the query's backward deposits with float atomics and has no fixed-point mode: its gradients to the float-atomics figure)
    o, _, fresh = _two_calls(_query, name, kind, "query_points forward + backward", exact_gradients=False)
    _check_query_vs_oracle(o, fresh)


@pytest.mark.parametrize("source", ["f64", "f16", "permuted"])
def test_converted_temporaries_land_on_one_address(source):
    """the hazard behind the converted-source rows, asserted where it happens: the dense float32 copy one call makes of the grid is
    freed when the call returns, and the caching allocator hands its block to the copy of the next call -- same data_ptr, version 0
    -- although the source changed in between"""
    o = cc.make_owner("sh1", source, DEV)

    def change():
        with torch.no_grad():
            o.features.add_(0.5)

    assert cc.converted_temporaries_collide(o.features, change)


# ---- VoxelGrid ----------------------------------------------------------------------------------------------------------------------
def _grid_calls(grid, r):
    from thre3d_atom.rendering.volumetric.render_interface import Rays
    from thre3d_atom.thre3d_reprs.renderers import SHVoxGridRenderConfig, render_sh_voxel_grid, render_sh_voxel_grid_attn

    cfg = SHVoxGridRenderConfig(num_samples_per_ray=S, camera_bounds=(NEAR, FAR), perturb_sampled_points=True, white_bkgd=True)
    rays = Rays(r["rays_o"], r["rays_d"], image_shape=(H, W))
    pts = gh.t(_points_np())
    out = {}
    with torch.no_grad():
        torch.manual_seed(5)        # (the renderers draw the in-kernel jitter stream from torch's CPU generator)
        sh = render_sh_voxel_grid(grid, rays, cfg)
        out["colour"], out["depth"] = sh.colour, sh.depth
        torch.manual_seed(5)
        out["attn"] = render_sh_voxel_grid_attn(grid, rays, cfg).attn
        torch.manual_seed(5)
        out["attn_orig"] = render_sh_voxel_grid_attn(grid, rays, cfg, orig_densities=True).attn
        out["query"] = grid.forward(pts)
        out["query_attn"] = grid.forward_attn(pts)
        out["query_attn_orig"] = grid.forward_attn(pts, orig_densities=True)
    return {k: v.clone() for k, v in out.items()}


class _AsOwner:
    """a VoxelGrid where the oracle helpers expect an Owner"""

    def __init__(self, grid):
        self.densities, self.features, self.spec = grid.densities, grid.features, grid.voxe_grid_spec()
        self.sh_degree = 0 if grid.features.shape[-1] == 3 else 1


GRID_ROWS = [(n, k) for n, k in cc.rows(gpu_only=True, grid_only=True) if k in ("sh0", "sh1")]


@pytest.mark.parametrize("name,kind", GRID_ROWS)
def test_voxel_grid_sees_the_change(name, kind):
    """render_sh_voxel_grid, render_sh_voxel_grid_attn, VoxelGrid.forward and forward_attn through the grid's OWN workspaces:
    calls -> change -> the same calls, before anything else touches the workspaces.  The outputs on the orig_densities snapshot
    must not move with the change; they move with update_orig_densities(), which is checked after it."""
    change = cc.BY_NAME[name]
    what = f"VoxelGrid [{name}-{kind}]"
    grid = cc.make_voxel_grid(kind, change.source, DEV)
    r = _rays()
    first = _grid_calls(grid, r)
    # (a tunable grid's render is a differentiable forward even under no_grad: the second one before any backward runs in the
    #  workspace's sibling.  Twice, so that both hold the old grid -- and twice after the change, so that both are asked)
    _same(_grid_calls(grid, r), first, True, what + " warm")
    change.apply(grid)
    second, third = _grid_calls(grid, r), _grid_calls(grid, r)
    fresh = _grid_calls(copy.deepcopy(grid), r)           # (a copy of a grid starts with empty workspaces)
    _same(second, fresh, True, what)
    _same(third, fresh, True, what + " again")
    changed_densities = name != "del_then_fresh_features"
    _visible(first, second, what + " sh", keys=("colour", "query"))
    if changed_densities:
        _visible(first, second, what + " attn", keys=("attn", "query_attn"))
    for k in ("attn_orig", "query_attn_orig"):            # the snapshot did not change, whatever the workspaces were told
        assert torch.equal(second[k], first[k]), (what, k)
    torch.manual_seed(5)
    rng = ops._next_rng()
    o = _AsOwner(grid)
    cfg = make_render_cfg(S, NEAR, FAR, perturb=True, white_bkgd=True, sh_degree=o.sh_degree, seed=rng[0], rng_offset=rng[1])
    ref = vo.render_fwd(_oracle_grid(o), cfg, *_rays_np())
    np.testing.assert_allclose(gh.n(fresh["colour"]), ref["colour"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(gh.n(fresh["depth"])[:, 0], ref["depth"], rtol=1e-5, atol=1e-5)
    # ---- the snapshot follows update_orig_densities()
    grid.update_orig_densities()
    after = _grid_calls(grid, r)
    _same(after, _grid_calls(copy.deepcopy(grid), r), True, what + " after update_orig_densities")
    for k in ("colour", "query", "attn", "query_attn"):
        assert torch.equal(after[k], second[k]), (what, k)
    if changed_densities:
        _visible(first, after, what + " snapshot", keys=("attn_orig", "query_attn_orig"))


def test_update_orig_densities_snapshot_at_an_old_address():
    """update_orig_densities() REPLACES the snapshot by a fresh clone -- version 0 like every clone, and soon at the address of
    the one before last (asserted).  forward_attn / the attention render with orig_densities=True must read the new snapshot."""
    grid = cc.make_voxel_grid("sh0", "f32", DEV)
    r = _rays()
    first = _grid_calls(grid, r)
    ptr, version = grid.orig_densities.data_ptr(), grid.orig_densities._version
    with torch.no_grad():
        grid.densities.add_(0.25)
    grid.update_orig_densities()                          # the first snapshot's block is free now
    held = []                                             # every free block the allocator prefers to it ...
    block = cc.alloc_at(ptr, lambda: torch.empty_like(grid.orig_densities), misses=held)
    del block                                             # ... is held, and it is free again
    with torch.no_grad():
        grid.densities.add_(0.25)
    grid.update_orig_densities()
    assert (grid.orig_densities.data_ptr(), grid.orig_densities._version) == (ptr, version), "hazard not built"
    del held
    second = _grid_calls(grid, r)
    fresh = _grid_calls(copy.deepcopy(grid), r)
    _same(second, fresh, True, "update_orig_densities")
    _visible(first, second, "update_orig_densities", keys=("attn_orig", "query_attn_orig"))


def test_invalidate_voxe_caches_after_a_write_torch_cannot_see():
    """the documented contract ("Writes torch cannot see"): a write through `.data` moves no version counter, the
    next render may show the old grid (printed, not asserted: that half is the contract, not a bug) -- and shows the new one after
    VoxelGrid.invalidate_voxe_caches()"""
    grid = cc.make_voxel_grid("sh0", "f32", DEV)
    r = _rays()
    first = _grid_calls(grid, r)
    version = grid.densities._version
    grid.densities.data.add_(0.5)
    assert grid.densities._version == version
    stale = _grid_calls(grid, r)
    fresh = _grid_calls(copy.deepcopy(grid), r)
    print(f"without the call: max |colour - current| {float((stale['colour'] - fresh['colour']).abs().max()):.3e}, "
          f"max |colour - previous| {float((stale['colour'] - first['colour']).abs().max()):.3e}")
    grid.invalidate_voxe_caches()
    second = _grid_calls(grid, r)
    _same(second, fresh, True, "after invalidate_voxe_caches")
    _visible(first, second, "after invalidate_voxe_caches", keys=("colour", "query", "attn"))


# ---- the library's own in-place writers ---------------------------------------------------------------------------------------------
class _Holders:
    """every kind of workspace one VoxelGrid keeps over the written tensors, as raw workspaces: the SH render, the point query, and
    two attention grids over the ONE density tensor; `check()` runs all of them against fresh workspaces"""

    def __init__(self, o):
        self.o = o
        vals = cc.grid_values("attn")[1]
        self.attn = [cc.Owner(o.densities.detach(), gh.t(vals) * s, cc.base_spec("attn"), 0) for s in (1.0, -0.5)]
        for a in self.attn:
            a._densities = o._densities          # (the same tensor object: one density tensor under three grids)
        self.r = _rays()
        self.ws = {"sh": ops.Workspace(), "query": ops.Workspace(), "attn0": ops.Workspace(), "attn1": ops.Workspace()}

    def _calls(self, ws):
        out = {}
        for k, v in _render_forward(self.o, ws["sh"], self.r, detach=True).items():
            out["sh_" + k] = v.clone()
        with torch.no_grad():
            out["query"] = ops.query_points(self.o.spec, self.o.densities, self.o.features, gh.t(_points_np()), workspace=ws["query"]).clone()
        for i, a in enumerate(self.attn):
            out[f"attn{i}"] = _render_forward(a, ws[f"attn{i}"], self.r, detach=True)["colour"].clone()
        return out

    def first(self):
        self.before = self._calls(self.ws)

    def check(self, what, densities_written=True, features_written=True):
        second = self._calls(self.ws)
        fresh = self._calls({k: ops.Workspace() for k in self.ws})
        _same(second, fresh, True, what)
        if densities_written:
            _visible(self.before, second, what + " (attention grids)", keys=("attn0", "attn1"))
        if features_written or densities_written:
            _visible(self.before, second, what + " (SH render, query)", keys=("sh_colour", "query"))
        _check_forward_vs_oracle(self.o, {"colour": fresh["sh_colour"], "depth": fresh["sh_depth"], "acc": fresh["sh_acc"]}, self.r)


def _adam_state(t):
    return (torch.zeros_like(t), torch.zeros_like(t))


def test_adam_step_writer():
    o = cc.make_owner("sh0", "f32", DEV)
    h = _Holders(o)
    h.first()
    for p in (o.densities, o.features):
        m, v = _adam_state(p)
        ops.adam_step_(p.detach(), torch.ones_like(p), m, v, 1, 0.5)
    h.check("adam_step_")


@pytest.mark.parametrize("mode", ["whole", "slab", "densities_frozen", "features_frozen"])
@pytest.mark.parametrize("kind", ["sh0", "sh1"])
def test_grid_adam_step_writer(mode, kind):
    """voxe_grid_adam_step writes the tensors through raw pointers and leaves the NEW grid packed in its own workspace; every other
    workspace that held a written tensor must pack again, and -- as the comment in grid_adam_step_ promises -- the workspaces over
    a FROZEN tensor alone keep their pack"""
    o = cc.make_owner(kind, "f32", DEV)
    h = _Holders(o)
    h.first()
    res = _bwd_acc(o, h.ws["sh"], h.r)                   # the gradient of one render, left in the workspace
    d, f = o.densities.detach(), o.features.detach()
    ops.grid_adam_step_(o.spec, d, f, int(res["layout"]), h.ws["sh"], 1, 0.5,
                        state_densities=None if mode == "densities_frozen" else _adam_state(d),
                        state_features=None if mode == "features_frozen" else _adam_state(f),
                        x_range=(4, 14) if mode == "slab" else None)      # (bricked gradients: an even first plane)
    if mode == "densities_frozen":
        # the two attention grids hold (densities, attn): nothing they hold was written
        ops.profile_enable(True)
        for i, a in enumerate(h.attn):
            _render_forward(a, h.ws[f"attn{i}"], h.r, detach=True)
        packs = ops.profile_read()["n_pack"]
        ops.profile_enable(False)
        assert packs == 0, packs
    h.check(f"grid_adam_step_ {mode}", densities_written=mode != "densities_frozen", features_written=mode != "features_frozen")


def test_recon_step_writer():
    o = cc.make_owner("sh0", "f32", DEV)
    h = _Holders(o)
    h.first()
    K, batch = 4, 1000
    poses = torch.stack([torch.cat([p.rotation, p.translation], dim=-1) for p in
                         (pose_spherical(*synth_pose_angles(i, 100), RADIUS) for i in (3, 38, 12, 58))]).float().to(DEV)
    images = torch.rand(K, 3, H, W, generator=torch.Generator().manual_seed(1)).to(DEV)
    d, f = o.densities.detach(), o.features.detach()
    losses = torch.zeros(4, device=DEV)
    p = ops.RenderParams(num_samples=S, near=NEAR, far=FAR, perturb=True, white_bkgd=True)
    ops.recon_step_(o.spec, p, d, f, h.ws["sh"], ops.Workspace(), H, W, focal_for(W), poses, torch.arange(K, device=DEV), images,
                    batch, False, _adam_state(d), _adam_state(f), 1, 1, 0.5, losses, (11, 0), zero_gradient_first=True)
    h.check("recon_step_")


def test_attn_refine_step_writer():
    o = cc.make_owner("sh0", "f32", DEV)
    h = _Holders(o)
    h.first()
    a = h.attn[0]
    amap = torch.rand(R, generator=torch.Generator().manual_seed(2)).to(DEV)
    attn = a.features.detach()
    p = dataclasses.replace(_params(a), deterministic=False)        # (the fused iteration has no fixed-point mode)
    ops.attn_refine_step_(a.spec, p, o.densities.detach(), attn, h.r["rays_o"], h.r["rays_d"], amap, h.ws["attn0"], 1, 0.5,
                          _adam_state(attn), 0.01, rng=RNG, zero_gradient_first=True)
    # (no `losses`: include/voxe.h allows NULL there, and the TV pass still runs for its gradient; the binding hands the library a
    #  scratch pair, since the pass stores its loss value unconditionally)
    second = h._calls(h.ws)
    fresh = h._calls({k: ops.Workspace() for k in h.ws})
    _same(second, fresh, True, "attn_refine_step_")
    _visible(h.before, second, "attn_refine_step_", keys=("attn0",))
    assert torch.equal(second["attn1"], h.before["attn1"]) and torch.equal(second["sh_colour"], h.before["sh_colour"])
    # ... and through a second workspace that held the attention grid before the step
    ws2 = ops.Workspace()
    b = cc.Owner(o.densities.detach(), gh.t(cc.grid_values("attn")[1]), cc.base_spec("attn"), 0)
    before = _render_forward(b, ws2, h.r)["colour"].clone()
    battn = b.features.detach()
    ops.attn_refine_step_(b.spec, p, b.densities.detach(), battn, h.r["rays_o"], h.r["rays_d"], amap, ops.Workspace(), 1, 0.5,
                          _adam_state(battn), 0.01, rng=RNG, zero_gradient_first=True)
    after = _render_forward(b, ws2, h.r)
    _same(after, _render_forward(b, ops.Workspace(), h.r), True, "attn_refine_step_, another workspace")
    _visible({"colour": before}, after, "attn_refine_step_, another workspace")


def _union_source(o):
    """a source grid for the CSG union: strictly denser than the destination in half of the box, other features"""
    d, f = cc.grid_values("sh0")
    d2 = d.copy()
    d2[: cc.DIMS[0] // 2] += 1.0
    d2[cc.DIMS[0] // 2:] -= 1.0
    return gh.t(d2), gh.t(np.ascontiguousarray(-f))


def test_grid_resample_union_writer():
    """UNION runs in place on the destination the caller hands in -- here the live grid tensors"""
    o = cc.make_owner("sh0", "f32", DEV)
    h = _Holders(o)
    h.first()
    sd, sf = _union_source(o)
    eye = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    xf = ops.make_resample(eye, [0.0, 0.0, 0.0], None, -1, abi.ACT_IDENTITY, 0.0, abi.RESAMPLE_UNION)
    _, _, taken = ops.grid_resample(sd, sf, xf, dst_densities=o.densities.detach(), dst_features=o.features.detach(), want_taken=True)
    assert 0.3 < float(taken.float().mean()) < 0.7
    h.check("grid_resample UNION")


def test_compose_voxel_grids_writer():
    from thre3d_atom.thre3d_reprs.transform import compose_voxel_grids_

    grid = cc.make_voxel_grid("sh0", "f32", DEV)
    src = cc.make_voxel_grid("sh0", "f32", DEV)
    sd, sf = _union_source(None)
    with torch.no_grad():
        src.densities.copy_(sd)
        src.features.copy_(sf)
        src.attn.mul_(-1.0)
    r = _rays()
    first = _grid_calls(grid, r)
    taken = compose_voxel_grids_(grid, src, [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    assert 0.2 < float(taken.float().mean()) < 0.7
    second = _grid_calls(grid, r)
    fresh = _grid_calls(copy.deepcopy(grid), r)
    _same(second, fresh, True, "compose_voxel_grids_")
    _visible(first, second, "compose_voxel_grids_", keys=("colour", "query"))
    _visible(first, second, "compose_voxel_grids_ (attention)", keys=("attn", "query_attn"))


# ---- the cache must still hit -------------------------------------------------------------------------------------------------------
def _packs(fn):
    ops.profile_enable(True)
    try:
        fn()
        return ops.profile_read()["n_pack"]
    finally:
        ops.profile_enable(False)


@pytest.mark.parametrize("kind", ["sh0", "sh1", "attn"])
@pytest.mark.parametrize("source", ["f32", "f64"])
def test_pack_counts(kind, source):
    """an unchanged grid rendered twice through one workspace is packed once, a changed grid twice, and a forward followed by its
    own backward once -- for a float64 grid too, whose dense copy is a new temporary in every call.  (bench.py's step relies on
    the hit: "never cache" must not pass this module.)"""
    o = cc.make_owner(kind, source, DEV)
    r = _rays()
    ws = ops.Workspace()
    fwd = functools.partial(_render_forward, o, r=r, detach=True)
    assert _packs(lambda: (fwd(ws), fwd(ws))) == 1
    assert _packs(lambda: fwd(ws)) == 0
    cc.BY_NAME["add_"].apply(o)
    assert _packs(lambda: (fwd(ws), fwd(ws))) == 1
    ws2 = ops.Workspace()
    assert _packs(lambda: (fwd(ws2), cc.BY_NAME["add_"].apply(o), fwd(ws2))) == 2
    # training: forward + backward, step after step through one workspace
    ws3 = ops.Workspace()
    assert _packs(lambda: _render_forward_backward(o, ws3, r)) == 1
    assert _packs(lambda: _render_forward_backward(o, ws3, r)) == 0
    cc.BY_NAME["add_"].apply(o)
    assert _packs(lambda: _render_forward_backward(o, ws3, r)) == 1
    assert _packs(lambda: _render_forward_backward(o, ops.Workspace(), r)) == 1
    # (the point query's pack pass is outside the profiler's phases: tests/test_cache_keys_host.py holds its decision)
    if source == "f32":
        assert _packs(lambda: _into(o, ops.Workspace(), r)) == 1
        assert _packs(lambda: _bwd_acc(o, ops.Workspace(), r)) == 1


def test_voxel_grid_pack_counts():
    """a training loop on a VoxelGrid: render_sh_voxel_grid + backward through the grid's own workspace packs once per change"""
    from thre3d_atom.rendering.volumetric.render_interface import Rays
    from thre3d_atom.thre3d_reprs.renderers import SHVoxGridRenderConfig, render_sh_voxel_grid

    grid = cc.make_voxel_grid("sh0", "f32", DEV)
    r = _rays()
    cfg = SHVoxGridRenderConfig(num_samples_per_ray=S, camera_bounds=(NEAR, FAR), perturb_sampled_points=True, white_bkgd=True)
    rays = Rays(r["rays_o"], r["rays_d"], image_shape=(H, W))

    def step():
        render_sh_voxel_grid(grid, rays, cfg).colour.sum().backward()

    assert _packs(step) == 1
    assert _packs(step) == 0
    with torch.no_grad():
        grid.densities.add_(0.5)
    assert _packs(step) == 1
    assert _packs(step) == 0
    grid.invalidate_voxe_caches()
    assert _packs(step) == 1


# ---- the ray-state cache --------------------------------------------------------------------------------------------------------------
class _LibSpy:
    """voxe_hip.ops.lib() with the backward entry points recording the VoxeRenderCfg::ray_state_valid they are handed"""

    def __init__(self, real):
        self._real, self.claims = real, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name not in ("voxe_render_bwd", "voxe_render_bwd_acc_into"):
            return fn

        def spy(g, c, *rest):
            self.claims.append(int(c._obj.ray_state_valid))
            return fn(g, c, *rest)
        return spy


def _ray_batch():
    """rays and a jitter tensor, each between two neighbours of its size (cache_cases.make_owner: the block a dropped tensor leaves
    stays a block of that size)"""
    o, d = _rays_np()
    jit = torch.rand((R, S), generator=torch.Generator().manual_seed(4)).numpy()
    r, guards = {}, []
    for k, a in (("rays_o", o), ("rays_d", d), ("jitter", jit)):
        guards.append(gh.t(a).clone())
        r[k] = gh.t(a)
        guards.append(gh.t(a).clone())
    r["guards"] = guards
    return r


def _fwd_then(o, ws, r, change, acc):
    """render_fwd_into -> change(r) -> the backward on whatever r holds then; the gradient"""
    dens, feat = _dense(o)
    p = _params(o)
    gc_, gd_, ga_ = _upstream(_cout(o))
    outs = _outs(o)
    ops.render_fwd_into(o.spec, p, dens, feat, r["rays_o"], r["rays_d"], r["jitter"], *outs, ws, RNG)
    if change is not None:
        change(r)
        # (a caller who moved its rays renders them again before it differentiates: the outputs are those of the new rays)
        ops.render_fwd_into(o.spec, p, dens, feat, r["rays_o"], r["rays_d"], r["jitter"], *outs, ops.Workspace(), RNG, keep_for_backward=False)
    flat = o.sh_degree == 0
    args = (o.spec, p, dens, feat, r["rays_o"], r["rays_d"], r["jitter"], outs[0], outs[1], outs[2], gc_, gd_ if flat else None,
            ga_ if flat else None)
    if acc:
        ops.render_bwd_acc(*args, ws, RNG, zero_first=True)
        return {"d_region": ops.workspace_grad_view(o.spec, dens, feat, ws).clone()}
    dd, df = torch.empty_like(dens), torch.empty_like(feat)
    ops.render_bwd_into(*args, dd, df, ws, RNG)
    return {"d_densities": dd, "d_features": df}


@pytest.mark.parametrize("acc", [False, True], ids=["bwd_into", "bwd_acc"])
@pytest.mark.parametrize("kind,route", [("sh0", "shipped"), ("sh0", "tile"), ("sh1", "shipped"), ("attn", "shipped")])
@pytest.mark.parametrize("name", sorted(cc.RAY_CHANGES))
def test_ray_states_follow_the_rays(name, kind, acc, route, disp, monkeypatch):
    """render_fwd_into -> the rays (or the jitter tensor) rewritten in place, or replaced at the same address -> backward: the
    gradient is that of a fresh forward + backward on the new rays, not that of the rays the forward marched; the untouched
    sequence still reaches the library with ray_state_valid = 1"""
    if route == "tile":
        disp.set(tile_min_rays=-1)
    o = cc.make_owner(kind, "f32", DEV)
    spy = _LibSpy(ops.lib())
    monkeypatch.setattr(ops, "lib", lambda: spy)
    untouched = _fwd_then(o, ops.Workspace(), _ray_batch(), None, acc)
    assert spy.claims == [1], spy.claims
    r = _ray_batch()
    got = _fwd_then(o, ops.Workspace(), r, cc.RAY_CHANGES[name], acc)
    assert spy.claims == [1, 0], spy.claims
    want = _fwd_then(o, ops.Workspace(), r, None, acc)
    assert spy.claims == [1, 0, 1], spy.claims
    _same(got, want, o.sh_degree == 0, f"{name} [{kind}]")
    for k in want:
        rel = rel_l2(gh.n(got[k]), gh.n(untouched[k]))
        print(f"{name} [{kind}] {k}: rel-L2 between the gradients on the new and on the old rays {rel:.3e}")
        assert rel > 1e-2, (name, k, rel)


def test_autograd_backward_takes_the_forward_states(monkeypatch):
    """ops.render: the backward sees the rays as autograd unpacked them (other Python objects over the same storages) and still
    claims the forward's states; a backward-less forward through the workspace in between ends the claim, and the gradient is
    the same"""
    o = cc.make_owner("sh0", "f32", DEV)
    spy = _LibSpy(ops.lib())
    monkeypatch.setattr(ops, "lib", lambda: spy)
    r = _rays()
    want = _render_forward_backward(o, ops.Workspace(), r)
    assert spy.claims == [1], spy.claims
    ws = ops.Workspace()
    gc_, gd_, ga_ = _upstream(3)
    c, d, a, _ = ops.render(o.spec, _params(o), o.densities, o.features, r["rays_o"], r["rays_d"], None, workspace=ws, rng=RNG)
    _render_forward(o, ws, _rays(3), detach=True)          # another camera, inference: it marches its own rays through `ws`
    ((c * gc_).sum() + (d * gd_).sum() + (a * ga_).sum()).backward()
    assert spy.claims == [1, 0], spy.claims
    _same({"d_densities": o.densities.grad, "d_features": o.features.grad}, {k: want[k] for k in ("d_densities", "d_features")}, True,
          "backward after another forward")
