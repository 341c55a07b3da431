"""The buffer contract of include/voxe.h, entry point by entry point: every buffer is caller-owned, nothing is allocated inside,
and the sizes come from the header's element counts, the voxe_*_scratch_bytes functions and voxe_workspace_bytes.

Every pointer of every call below comes from tests/arena.py: outputs of exactly the documented element count, scratch of exactly
what the matching size function returns, the workspace of exactly voxe_workspace_bytes (also at the ray_state_valid = -1 size for
forward-only calls, and with voxe_tile_plan_bytes added where a plan exists), each between two 64 KiB guard bands, the rear one
starting at the very next byte.  tests/contract.py holds what every case asserts:

  (a) nothing outside: the bands are clean after the call and a synchronisation;
  (b) inputs are inputs: every `const` buffer is bit-identical afterwards (documented in-place arguments: bounds only);
  (c) overwrite means every element: outputs poisoned with 0xFF come back without a NaN / -1 (the disparity of rays with
      acc = 0 is NaN in the oracle too: that mask comes from the oracle);
  (d) nothing unwritten is read: the call runs with everything poisoned 0xFF and again 0x00; outputs free of atomics must have
      equal bits, outputs built with float atomics must be finite and within the tolerance the entry point's parity test uses
      (those constants are imported from the modules that own them);
  (e) a size argument one byte short of the smallest size the header lets the call accept gives VOXE_ERR_WORKSPACE, and a
      count of 0 gives VOXE_OK, both with the whole arena untouched.  The buffer is never actually short.

On (e) for the render calls: the header gives the workspace tiers ("the forward needs only the packed grid, and the backward
needs everything but the last region"), so voxe_render_fwd / voxe_sample_probe / voxe_query_fwd are refused below
voxe_workspace_grad_offset (the packed grid), voxe_render_bwd below the ray_state_valid = -1 size -- and one byte below
voxe_workspace_bytes they must run on the smaller tier and still keep (a) to (d): the "one_short" tier.  The smaller tiers
also run in buffers that END there: "total" (forward + backward in exactly the ray_state_valid = -1 size) and "packed_only"
(the forward, the probe and the point query in exactly the packed grid), so a kernel that still touched the states, the
two-phase sources or the binning scratch of the larger tier would land in a band.

Shapes are ragged on purpose (voxel counts that are no multiple of 4, 64 or 256, R = 1499, 37 x 29 and 21 x 13 images) next to
one aligned grid; no shape is the workload's, every call takes well under a second."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import background_ref as BR
import camera_ref as CR
import distortion_ref as DR
from contract import DEV, P, rel_l2, run_contract, run_empty, run_short
from test_background_gpu import GRAD_REL_L2 as BACKGROUND_GRAD_REL_L2
from test_distortion_gpu import GRAD_REL_L2 as DISTORTION_GRAD_REL_L2
from test_hip_fused_step import LR
from test_hip_fuzz import _close as query_grad_close
from test_workspace_tiers_gpu import FWD_ATOL, GRAD_REL_L2
from voxe_hip import abi
from voxe_hip.desc import make_grid_desc, make_render_cfg

from oracle import voxe_oracle as vo

pytestmark = pytest.mark.gpu

AABB = ((-1.5, 1.5),) * 3
NEAR, FAR = 1.8, 6.6
SCALE = 2.0
GRIDS = {"odd": (17, 9, 13), "tiny": (5, 6, 7), "aligned": (8, 8, 16)}
F32, I32, I64, U8 = torch.float32, torch.int32, torch.int64, torch.uint8


def _lib():
    from voxe_hip.runtime import lib

    return lib()


def _stream():
    from voxe_hip.runtime import stream_ptr

    return stream_ptr(DEV)


# ---- scenes: host arrays, built once ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _grid(dims, F, seed=1):
    rng = np.random.default_rng(seed + 7 * F + sum(dims))
    return (rng.uniform(-1, 1, (*dims, 1)).astype(np.float32), rng.uniform(-1, 1, (*dims, F)).astype(np.float32))


def _pose(i):
    from thre3d_atom.utils.imaging_utils import pose_spherical

    p = pose_spherical(40.0 + 97.0 * i, 35.0 - 11.0 * i, 4.0311)
    return p.rotation.numpy().astype(np.float32), p.translation.numpy().astype(np.float32).reshape(3)


def _focal(W):
    return float(0.5 * W / np.tan(0.5 * 0.6911112))


@functools.lru_cache(maxsize=None)
def _image_rays(W, H, K=1):
    o, d = zip(*(vo.cast_rays(H, W, _focal(W), *_pose(i)) for i in range(K)))
    return np.concatenate(o).astype(np.float32), np.concatenate(d).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _random_rays(R, seed=7):
    gen = torch.Generator().manual_seed(seed)
    o = torch.randn(R, 3, generator=gen)
    o = 4.0311 * o / o.norm(dim=1, keepdim=True)
    d = torch.empty(R, 3).uniform_(-1.2, 1.2, generator=gen) - o
    return o.numpy().copy(), (d / d.norm(dim=1, keepdim=True)).numpy().copy()


def _poses(K):
    return np.stack([np.concatenate([r, t[:, None]], axis=1) for r, t in (_pose(i) for i in range(K))]).astype(np.float32)


class Scene:
    """one render configuration: grid, rays, cfg and the dispatch that forces its route"""

    def __init__(self, grid="odd", deg=0, attn=False, rays="image", S=33, disp=None, cfg=None, route=None):
        self.dims, self.deg, self.attn, self.S = GRIDS[grid], deg, attn, S
        self.F = 1 if attn else 3 * (deg + 1) ** 2
        self.cout = 1 if attn else 3
        self.kind = abi.FEAT_ATTN if attn else abi.FEAT_SH
        self.dens, self.feat = _grid(self.dims, self.F)
        self.W, self.H = {"image": (37, 29), "views": (21, 13), "random": (0, 0)}[rays]
        self.ro, self.rd = {"image": lambda: _image_rays(37, 29), "views": lambda: _image_rays(21, 13, 3),
                            "random": lambda: _random_rays(1499)}[rays]()
        self.R = self.ro.shape[0]
        self.disp_fields, self.cfg_fields, self.route = dict(disp or {}), dict(cfg or {}), route
        self.nvox = int(np.prod(self.dims))

    def desc(self, dens_ptr, feat_ptr):
        return make_grid_desc(dens_ptr, feat_ptr, self.dims, self.F, AABB, SCALE, abi.ACT_IDENTITY, abi.ACT_SOFTPLUS, self.kind)

    def cfg(self, **over):
        disp = abi.VoxeDispatch()
        for key, v in self.disp_fields.items():
            setattr(disp, key, v)
        kw = dict(perturb=True, white_bkgd=not self.attn, sh_degree=self.deg, seed=5, rng_offset=3, image_width=self.W,
                  image_height=self.H if self.W and self.R > self.W * self.H else 0, dispatch=disp)
        kw.update(self.cfg_fields)
        kw.update(over)
        return make_render_cfg(self.S, NEAR, FAR, **kw)

    @functools.lru_cache(maxsize=None)
    def upstream(self):
        rng = np.random.default_rng(9)
        return (rng.standard_normal((self.R, self.cout)).astype(np.float32), (0.2 * rng.standard_normal(self.R)).astype(np.float32),
                (0.1 * rng.standard_normal(self.R)).astype(np.float32))

    @functools.lru_cache(maxsize=None)
    def oracle(self):
        """the CPU oracle's forward and gradients of this scene, computed once and shared"""
        grid = vo.Grid(self.dens, self.feat, AABB, SCALE, abi.ACT_IDENTITY, abi.ACT_SOFTPLUS, self.kind)
        cfg = make_render_cfg(self.S, NEAR, FAR, perturb=True, white_bkgd=not self.attn, sh_degree=self.deg, seed=5, rng_offset=3,
                              **{k: v for k, v in self.cfg_fields.items() if k in ("aabb_clip", "linear_disparity", "render_diffuse")})
        fwd = vo.render_fwd(grid, cfg, self.ro, self.rd)
        gc, gdep, gacc = self.upstream()
        gd, gf = vo.render_bwd(grid, cfg, self.ro, self.rd, gc, d_depth=gdep, d_acc=gacc)
        return fwd, gd, gf


TILE = dict(tile_min_rays=-1)
RENDERS = {
    # the routes of RENDERS in tests/test_workspace_tiers_gpu.py, forced through VoxeDispatch at ragged sizes
    "tile_segmented": dict(S=96, disp=TILE, route=abi.ROUTE_TILE),
    "tile_s33": dict(S=33, disp=TILE, route=abi.ROUTE_TILE),
    "tile_one_segment": dict(S=16, disp=TILE, route=abi.ROUTE_TILE),
    "tile_two_phase": dict(deg=1, S=96, disp=TILE, route=abi.ROUTE_TILE),
    "region": dict(rays="random", disp=dict(region_min_rays=1), route=abi.ROUTE_REGION),
    "packed_scatter": dict(rays="random", disp=dict(region_min_rays=-1), route=abi.ROUTE_PACKED_SCATTER),
    # ... and the ones that file does not have
    "scatter": dict(rays="random", disp=dict(bwd_mode=1), route=abi.ROUTE_SCATTER),
    "deterministic": dict(cfg=dict(deterministic=True), route=abi.ROUTE_DETERMINISTIC),
    "precise_grad": dict(S=96, disp=dict(tile_min_rays=-1, precise_grad=1), route=abi.ROUTE_TILE),
    "tile_planned": dict(S=96, disp=dict(tile_min_rays=-1, tile_map=4), route=abi.ROUTE_TILE),
    "views_tile": dict(rays="views", S=96, disp=TILE, route=abi.ROUTE_TILE),
    "views_shipped": dict(rays="views", route=abi.ROUTE_PACKED_SCATTER),
    "image_shipped_clip": dict(cfg=dict(aabb_clip=True), route=abi.ROUTE_PACKED_SCATTER),
    "region_sh1": dict(deg=1, rays="random", disp=dict(region_min_rays=1), route=abi.ROUTE_REGION),
    "tile_sh2_tiny": dict(grid="tiny", deg=2, disp=TILE, route=abi.ROUTE_TILE),
    "tile_sh3_views": dict(deg=3, rays="views", disp=TILE, route=abi.ROUTE_TILE),
    "scatter_sh3_tiny": dict(grid="tiny", deg=3, rays="random", disp=dict(region_min_rays=-1), route=None),
    "tile_attn": dict(attn=True, disp=TILE, route=abi.ROUTE_TILE),
    "scatter_attn_aligned": dict(grid="aligned", attn=True, rays="random", disp=dict(region_min_rays=-1), route=None),
    "tile_tiny": dict(grid="tiny", S=96, disp=TILE, route=abi.ROUTE_TILE),
    "tile_aligned": dict(grid="aligned", S=96, disp=TILE, route=abi.ROUTE_TILE),
    "region_aligned": dict(grid="aligned", rays="random", disp=dict(region_min_rays=1), route=abi.ROUTE_REGION),
    "packed_scatter_tiny": dict(grid="tiny", rays="random", disp=dict(region_min_rays=-1), route=abi.ROUTE_PACKED_SCATTER),
}


@functools.lru_cache(maxsize=None)
def scene(name):
    return Scene(**RENDERS[name])


def _ws_sizes(sc, g, c, R=None):
    """(packed grid alone, ray_state_valid = -1 size, voxe_workspace_bytes, plan bytes) of a render"""
    L, R = _lib(), sc.R if R is None else R
    gp, cp = C.byref(g), C.byref(c)
    keep = c.ray_state_valid
    c.ray_state_valid = -1
    inference = L.voxe_workspace_bytes(gp, cp, R)
    c.ray_state_valid = 0
    full, plan = L.voxe_workspace_bytes(gp, cp, R), L.voxe_tile_plan_bytes(gp, cp, R)
    c.ray_state_valid = keep
    return L.voxe_workspace_grad_offset(gp), inference, full, plan


def test_arena_reports_a_write_on_the_device():
    """the bite of the checks on the device the cases run on (tests/test_arena_host.py has the CPU's)"""
    from contract import K

    k = K(0xFF)
    out, src = k.out("out", 1499), k.inp("src", np.arange(7, dtype=np.float32))
    k.begin()
    assert k.a.check() == [] and k.a.unchanged() == []
    k.a.mem[out.ptr - k.a.base + out.nbytes] = 0          # the byte right behind a ragged buffer
    src.t[3] = -3.0
    assert k.a.check() == ["out: rear band dirty at offset 0, 1 dirty bytes of 65536"]
    assert k.a.unchanged() == ["src: input changed at byte 15, 1 bytes differ"]


# ---- render forward + backward ------------------------------------------------------------------------------------------------
def render_case(k, name, tier):
    """voxe_render_fwd, then voxe_render_bwd (overwrite, then accumulate on top) in one workspace of the tier's exact size"""
    L, sc, st = _lib(), scene(name), _stream()
    R, cout = sc.R, sc.cout
    dens, feat = k.inp("densities", sc.dens), k.inp("features", sc.feat)
    ro, rd = k.inp("rays_o", sc.ro), k.inp("rays_d", sc.rd)
    g, c = sc.desc(dens.ptr, feat.ptr), sc.cfg()
    gp, cp = C.byref(g), C.byref(c)
    packed, inference, full, plan = _ws_sizes(sc, g, c)
    if sc.route is not None:
        assert L.voxe_render_route(gp, cp, R) == sc.route
    if tier == "plan":
        assert plan > 0, "this configuration builds no per-tile plan"
    det = bool(c.deterministic)
    # "total": the smallest workspace a backward accepts (no two-phase sources, no region scratch: the call takes the smaller
    # tier); "packed_only": the smallest a forward accepts (no states, no segment partials)
    ws = k.scratch("workspace", {"full": full, "one_short": full, "plan": full + plan, "inference": inference, "total": inference,
                                 "packed_only": packed}[tier])
    given = ws.nbytes - 1 if tier == "one_short" else ws.nbytes
    colour, depth, acc, disp = (k.out(n, R * m) for n, m in (("colour", cout), ("depth", 1), ("acc", 1), ("disparity", 1)))
    backward = tier not in ("inference", "packed_only")
    if backward:
        gc, gdep, gacc = (k.inp(n, a) for n, a in zip(("d_colour", "d_depth", "d_acc"), sc.upstream()))
        d_dens, d_feat = k.out("d_densities", sc.nvox), k.out("d_features", sc.nvox * sc.F)
    k.begin()
    ref, ref_d, ref_f = sc.oracle()
    c.ray_state_valid = -1 if tier == "inference" else 0
    k.call(L.voxe_render_fwd, gp, cp, ro.ptr, rd.ptr, k.count(R, "fwd"), None, colour.ptr, depth.ptr, acc.ptr, disp.ptr, ws.ptr,
           min(given, k.size(ws, "fwd", minimum=packed)), st)
    for b in (colour, depth, acc):
        k.bits(b)
    k.bits(disp, nan_ok=np.isnan(ref["disparity"]))
    np.testing.assert_allclose(colour.cpu().numpy().reshape(R, cout), ref["colour"].reshape(R, cout), rtol=0, atol=FWD_ATOL)
    np.testing.assert_allclose(acc.cpu().numpy(), ref["acc"].reshape(-1), rtol=0, atol=FWD_ATOL)
    assert float(ref["acc"].max()) > 0.5                          # (the rays do hit the volume)
    if not backward:
        return
    c.ray_state_valid = 0
    frozen = [(b, b.t.clone()) for b in (colour, depth, acc, disp)]
    # the deterministic backward has no smaller tier: it needs the whole of voxe_workspace_bytes
    refused = det and tier == "one_short"
    for accumulate in (0, 1):
        k.call(L.voxe_render_bwd, gp, cp, ro.ptr, rd.ptr, R, None, colour.ptr, depth.ptr, acc.ptr, gc.ptr, gdep.ptr, gacc.ptr,
               d_dens.ptr, d_feat.ptr, accumulate, ws.ptr, min(given, k.size(ws, "bwd", minimum=full if det else inference)), st,
               expect=abi.ERR_WORKSPACE if refused else abi.OK)
        for b, was in frozen:
            assert torch.equal(b.t.view(I32), was.view(I32)), f"{b.name}: a const argument of the backward changed"
        if refused:
            assert k.a.poisoned("d_densities") == d_dens.nbytes and k.a.poisoned("d_features") == d_feat.nbytes
            return
        tag = "+=" if accumulate else "="
        for b, want in ((d_dens, ref_d), (d_feat, ref_f)):
            if det:
                k.bits(b, f"{b.name} {tag}")
                assert rel_l2(b.cpu().numpy(), (1 + accumulate) * want.reshape(-1)) < GRAD_REL_L2
            else:
                k.tol(b, (1 + accumulate) * want, GRAD_REL_L2, f"{b.name} {tag}")


RENDER_TIERS = ([(n, "full") for n in RENDERS] + [(n, "inference") for n in RENDERS] + [(n, "packed_only") for n in RENDERS]
                + [(n, "total") for n in RENDERS if n != "deterministic"]
                + [(n, "one_short") for n in ("tile_two_phase", "region", "region_sh1", "deterministic", "tile_sh3_views")]
                + [("tile_planned", "plan")])


@pytest.mark.parametrize("name,tier", RENDER_TIERS, ids=[f"{n}-{t}" for n, t in RENDER_TIERS])
def test_render_fwd_bwd(name, tier):
    run_contract(render_case, name, tier)


@pytest.mark.parametrize("tag", ["fwd", "bwd"])
@pytest.mark.parametrize("name", ["tile_segmented", "tile_two_phase", "region", "packed_scatter", "scatter", "deterministic", "tile_attn"])
def test_render_refuses_a_short_workspace(name, tag):
    run_short(render_case, tag, name, "full")


# ---- gradient left in the workspace + fused grid step ----------------------------------------------------------------------------
STEPS = {
    # name: (render, linear_grad, x range or None, into a second workspace, regulariser, extra gradients)
    "bricked_whole": ("packed_scatter", False, None, False, None, False),
    "bricked_slab": ("packed_scatter", False, (4, 11), False, None, True),
    "linear_whole": ("packed_scatter", True, None, False, None, True),
    "linear_slab_odd": ("tile_segmented", False, (3, 12), False, None, False),
    "into_second_workspace": ("tile_segmented", False, None, True, None, False),
    "dcl": ("tile_segmented", False, None, False, "dcl", False),
    "l2_slab": ("packed_scatter", True, (5, 17), False, "l2", False),
    "l1": ("packed_scatter", False, None, False, "l1", False),
    "feature_correlation": ("tile_s33", False, None, False, "feat", False),
    "sh1_linear": ("tile_two_phase", False, None, False, None, False),
    "sh3_tiny_bricked": ("scatter_sh3_tiny", False, (2, 5), False, None, False),
    "attn_aligned": ("scatter_attn_aligned", False, None, False, "feat", False),
    "tiny_bricked": ("packed_scatter_tiny", False, None, False, "dcl", True),
}
BETA1 = 0.9


def _well_above_noise(exp_avg):
    """the elements tests/test_hip_fused_step.py compares parameters on: gradient above 1e-3 of its maximum"""
    m = exp_avg.cpu().numpy()
    return np.abs(m) > 1e-3 * np.abs(m).max()


def step_case(k, name):
    """voxe_render_fwd -> voxe_render_bwd_acc(_into) -> voxe_grid_adam_step: parameters and moments in place, the step's
    workspace of exactly packed grid + gradient region when the gradient went into a second one"""
    L, st = _lib(), _stream()
    render, linear, xr, into, regkind, extras = STEPS[name]
    sc = scene(render)
    R, cout, dims, F, nvox = sc.R, sc.cout, sc.dims, sc.F, sc.nvox
    rng = np.random.default_rng(3)
    dens, feat = k.inout("densities", sc.dens), k.inout("features", sc.feat)
    ro, rd = k.inp("rays_o", sc.ro), k.inp("rays_d", sc.rd)
    gc, gdep, gacc = (k.inp(n, a) for n, a in zip(("d_colour", "d_depth", "d_acc"), sc.upstream()))
    g, c = sc.desc(dens.ptr, feat.ptr), sc.cfg(linear_grad=linear)
    gp, cp = C.byref(g), C.byref(c)
    _, _, full, _ = _ws_sizes(sc, g, c)
    grid_bytes = L.voxe_workspace_grad_offset(gp) + L.voxe_workspace_grad_bytes(gp)
    ws = k.scratch("workspace", full)
    ws2 = k.scratch("grad_workspace", grid_bytes) if into else None
    colour, depth, acc = (k.out(n, R * m) for n, m in (("colour", cout), ("depth", 1), ("acc", 1)))
    zeros_d, zeros_f = np.zeros(nvox, np.float32), np.zeros(nvox * F, np.float32)
    m_d, v_d = k.inout("exp_avg_densities", zeros_d), k.inout("exp_avg_sq_densities", zeros_d)
    m_f, v_f = k.inout("exp_avg_features", zeros_f), k.inout("exp_avg_sq_features", zeros_f)
    ex_d = k.inp("extra_d_densities", 1e-3 * rng.standard_normal(nvox).astype(np.float32)) if extras else None
    ex_f = k.inp("extra_d_features", 1e-3 * rng.standard_normal(nvox * F).astype(np.float32)) if extras else None
    reg = None
    if regkind:
        reg = abi.VoxeGridRegularisers()
        sc_reg = k.scratch("regulariser scratch", L.voxe_dcl_scratch_bytes(nvox))
        if regkind == "feat":
            fref, floss = k.inp("feat_reference", _grid(dims, F, seed=4)[1]), k.out("feat_loss", 1)
            reg.feat_reference, reg.feat_weight, reg.feat_loss = fref.ptr, 0.3, floss.ptr
        else:
            dref, dloss = k.inp("dcl_reference", _grid(dims, F, seed=4)[0]), k.out("dcl_loss", 1)
            reg.dcl_reference, reg.dcl_weight, reg.dcl_loss = dref.ptr, 200.0, dloss.ptr
            reg.density_kind = {"dcl": abi.DREG_CORRELATION, "l2": abi.DREG_L2, "l1": abi.DREG_L1}[regkind]
    k.begin()
    step_ws = ws2 if into else ws
    k.call(L.voxe_render_fwd, gp, cp, ro.ptr, rd.ptr, R, None, colour.ptr, depth.ptr, acc.ptr, None, ws.ptr, ws.nbytes, st)
    layout = C.c_int32(abi.GRAD_ANY)
    args = (gp, cp, ro.ptr, rd.ptr, R, None, colour.ptr, depth.ptr, acc.ptr, gc.ptr, gdep.ptr, gacc.ptr, 1, 1, 1, C.byref(layout),
            ws.ptr, k.size(ws, "bwd_acc", minimum=_ws_sizes(sc, g, c)[1]))
    if into:
        k.call(L.voxe_render_bwd_acc_into, *args, ws2.ptr, k.size(ws2, "grad_workspace"), st)
    else:
        k.call(L.voxe_render_bwd_acc, *args, st)
    assert layout.value == L.voxe_render_bwd_layout(gp, cp, R)
    if sc.route is not None:
        assert layout.value == (abi.GRAD_BRICKED if sc.route == abi.ROUTE_PACKED_SCATTER and not linear else abi.GRAD_LINEAR)
    x0, x1 = xr or (0, dims[0])
    before = {b.name: b.cpu() for b in (dens, feat, m_d, v_d, m_f, v_f)}
    if reg is not None:
        reg.scratch, reg.scratch_bytes = sc_reg.ptr, k.size(sc_reg, "regulariser")
    k.call(L.voxe_grid_adam_step, gp, layout.value, x0, x1, P(ex_d), P(ex_f), m_d.ptr, v_d.ptr, m_f.ptr, v_f.ptr, LR, BETA1, 0.999, 1e-8,
           1, 0, None if reg is None else C.byref(reg), step_ws.ptr, k.size(step_ws, "step", minimum=grid_bytes), st)
    plane = dims[1] * dims[2]
    ref_d, ref_f = sc.oracle()[1:]
    for b, per, ref, extra in ((dens, 1, None, None), (feat, F, None, None), (m_d, 1, ref_d, ex_d), (v_d, 1, None, None),
                               (m_f, F, ref_f, ex_f), (v_f, F, None, None)):
        now, was = b.cpu(), before[b.name]
        lo, hi = x0 * plane * per, x1 * plane * per
        assert torch.equal(now[:lo], was[:lo]) and torch.equal(now[hi:], was[hi:]), f"{b.name}: written outside the slab"
        assert bool(torch.isfinite(now).all()), b.name
        assert not torch.equal(now[lo:hi], was[lo:hi]), f"{b.name}: the step did nothing"
        if ref is not None and regkind is None:
            # exp_avg after the first step = (1 - beta1) x gradient: the render gradient against the oracle
            want = ref.reshape(-1) + (extra.cpu().numpy() if extra is not None else 0.0)
            err = rel_l2(now.numpy()[lo:hi] / np.float32(1 - BETA1), want[lo:hi])
            print(f"{name} {b.name}: rel-L2 {err:.2e}")
            assert err < GRAD_REL_L2, (b.name, err)
        # between the two fills: the moments within twice the gradient bound, the parameters as tests/test_hip_fused_step.py
        # holds them to the oracle (Adam's first step is lr * sign(g): only where g is far above the atomics' noise)
        if b in (dens, feat):
            k.pair_abs(b, _well_above_noise(m_d if b is dens else m_f), 2 * 1e-3 * LR)
        else:
            k.pair(b, 2 * GRAD_REL_L2)
    if reg is not None:
        k.bits(floss if regkind == "feat" else dloss)
    # the step leaves a zeroed gradient region behind (the header's promise to the next render_bwd_acc with zero_first = 0)
    off, nb = L.voxe_workspace_grad_offset(gp), L.voxe_workspace_grad_bytes(gp)
    if xr is None:
        assert not bool(step_ws.t[off:off + nb].any()), "the gradient region is not cleared after the step"


@pytest.mark.parametrize("name", sorted(STEPS))
def test_bwd_acc_and_grid_adam_step(name):
    run_contract(step_case, name)


@pytest.mark.parametrize("name,tag", [("bricked_whole", "bwd_acc"), ("bricked_whole", "step"), ("into_second_workspace", "grad_workspace"),
                                      ("into_second_workspace", "step"), ("dcl", "regulariser"), ("l1", "regulariser"),
                                      ("feature_correlation", "regulariser")])
def test_bwd_acc_and_grid_adam_step_refuse_short_sizes(name, tag):
    run_short(step_case, tag, name)


# ---- ray casting and sampling ------------------------------------------------------------------------------------------------
def cast_rays_case(k):
    L, st = _lib(), _stream()
    H, W = 29, 37
    rot, trans = _pose(0)
    ro, rd = k.out("rays_o", H * W * 3), k.out("rays_d", H * W * 3)
    k.begin()
    k.call(L.voxe_cast_rays, H, W, _focal(W), rot.reshape(-1).ctypes.data_as(C.POINTER(C.c_float)),
           trans.ctypes.data_as(C.POINTER(C.c_float)), ro.ptr, rd.ptr, st)
    k.bits(ro), k.bits(rd)
    want_o, want_d = vo.cast_rays(H, W, _focal(W), rot, trans)
    assert np.array_equal(ro.cpu().numpy(), want_o.reshape(-1)) and np.array_equal(rd.cpu().numpy(), want_d.reshape(-1))


@functools.lru_cache(maxsize=None)
def _flat_index(K, H, W, B=1499):
    rng = np.random.default_rng(B)
    idx = rng.integers(0, K * H * W, size=B).astype(np.int64)
    idx[:2] = (0, K * H * W - 1)
    return idx


def cast_rays_indexed_case(k, camera):
    L, st = _lib(), _stream()
    H, W, K = 29, 37, 3
    idx_np = _flat_index(K, H, W)
    B = idx_np.shape[0]
    poses, idx = k.inp("poses", _poses(K)), k.inp("flat_index", idx_np)
    ro, rd = k.out("rays_o", B * 3), k.out("rays_d", B * 3)
    k.begin()
    if camera:
        cam = abi.VoxeCamera(H, W, 52.0, 47.5, 17.3, 15.1, -0.12, 0.03, 0.002, -0.001, 0.0)
        k.call(L.voxe_cast_rays_camera, C.byref(cam), poses.ptr, K, idx.ptr, k.count(B), ro.ptr, rd.ptr, st)
    else:
        k.call(L.voxe_cast_rays_indexed, H, W, _focal(W), poses.ptr, K, idx.ptr, k.count(B), ro.ptr, rd.ptr, st)
        want_o, want_d = vo.cast_rays_indexed(H, W, _focal(W), _poses(K), idx_np)
        assert np.array_equal(rd.cpu().numpy(), want_d.reshape(-1)) and np.array_equal(ro.cpu().numpy(), want_o.reshape(-1))
    k.bits(ro), k.bits(rd)


def cast_rays_camera_whole_case(k):
    """flat_index NULL: K whole images"""
    L, st = _lib(), _stream()
    H, W, K = 13, 21, 3
    poses = k.inp("poses", _poses(K))
    ro, rd = k.out("rays_o", K * H * W * 3), k.out("rays_d", K * H * W * 3)
    k.begin()
    cam = abi.VoxeCamera(H, W, 30.0, 28.5, 10.3, 6.1, -0.12, 0.03, 0.002, -0.001, 0.001)
    k.call(L.voxe_cast_rays_camera, C.byref(cam), poses.ptr, K, None, K * H * W, ro.ptr, rd.ptr, st)
    k.bits(ro), k.bits(rd)


def cast_rays_bwd_case(k, camera, whole):
    """the cameras, poses and batch of tests/test_camera_gpu.py, whose bounds these are"""
    L, st = _lib(), _stream()
    K = 3
    cam = CR.CAM_C if camera else CR.CAM_A
    poses_np = CR.random_poses(K)
    idx_np = None if whole else CR.indexed_batch(CR.CAM_C, K)
    B = K * cam.H * cam.W if whole else idx_np.shape[0]
    g_o, g_d = CR.upstream(B)
    poses = k.inp("poses", poses_np)
    idx = None if whole else k.inp("flat_index", idx_np)
    d_o, d_d = k.inp("d_rays_o", g_o), k.inp("d_rays_d", g_d)
    d_poses = k.out("d_poses", K * 12)
    want = CR.cast_rays_bwd(cam, poses_np, idx_np, g_o, g_d)
    if camera:
        d_intr, d_dist = k.out("d_intrinsics", 4), k.out("d_distortion", 5)
        sc = k.scratch("scratch", L.voxe_cast_rays_camera_bwd_scratch_bytes(K))
        k.begin()
        s = abi.VoxeCamera(cam.H, cam.W, cam.fx, cam.fy, cam.cx, cam.cy, *cam.dist)
        k.call(L.voxe_cast_rays_camera_bwd, C.byref(s), poses.ptr, K, P(idx), B, d_o.ptr, d_d.ptr, d_poses.ptr, d_intr.ptr, d_dist.ptr,
               0, sc.ptr, k.size(sc, "scratch"), st)
        for b, w in ((d_intr, want[1]), (d_dist, want[2])):
            k.written(b)
            got = b.cpu().numpy().astype(np.float64)
            assert np.all(np.abs(got - w) <= CR.LENS_GRAD_BOUND * np.abs(w)), (b.name, got, w)
            k.pair_out[b.name] = (b.cpu(), 2 * CR.LENS_GRAD_BOUND)
    else:
        d_focal = k.out("d_focal", 1)
        sc = k.scratch("scratch", L.voxe_cast_rays_bwd_scratch_bytes(K))
        k.begin()
        k.call(L.voxe_cast_rays_bwd, cam.H, cam.W, CR.LEGACY_FOCAL, poses.ptr, K, P(idx), B, d_o.ptr, d_d.ptr, d_poses.ptr, d_focal.ptr,
               0, sc.ptr, k.size(sc, "scratch"), st)
        k.tol(d_focal, [want[1][0] + want[1][1]], CR.POSE_GRAD_REL_L2)
    k.tol(d_poses, want[0], CR.POSE_GRAD_REL_L2)


def random_subset_case(k, n, count):
    L, st = _lib(), _stream()
    out = k.out("out", count, I64)
    k.begin()
    k.call(L.voxe_random_subset, n, count, 11, 5, out.ptr, st)
    k.bits(out)
    assert np.array_equal(out.cpu().numpy(), vo.random_subset(n, count, 11, 5))


def sample_probe_case(k, name, packed_only=False):
    L, sc, st = _lib(), scene(name), _stream()
    R, S = sc.R, sc.S
    dens, feat = k.inp("densities", sc.dens), k.inp("features", sc.feat)
    ro, rd = k.inp("rays_o", sc.ro), k.inp("rays_d", sc.rd)
    g, c = sc.desc(dens.ptr, feat.ptr), sc.cfg()
    packed, _, full, _ = _ws_sizes(sc, g, c)
    ws = k.scratch("workspace", packed if packed_only else full)
    idx, inside = k.out("idx", R * S * 3, I32), k.out("inside", R * S, U8)
    z, sigma, rad = k.out("zvals", R * S), k.out("sigma", R * S), k.out("rad", R * S * sc.cout)
    k.begin()
    k.call(L.voxe_sample_probe, C.byref(g), C.byref(c), ro.ptr, rd.ptr, R, None, idx.ptr, inside.ptr, z.ptr, sigma.ptr, rad.ptr,
           ws.ptr, k.size(ws, "workspace", minimum=packed), st)
    k.bits(idx, minus_one_ok=True)              # (the low corner of a sample just outside the grid IS -1)
    for b in (inside, z, sigma, rad):
        k.bits(b)


CASTS = {
    "cast_rays": (cast_rays_case,),
    "cast_rays_indexed": (cast_rays_indexed_case, False),
    "cast_rays_camera": (cast_rays_indexed_case, True),
    "cast_rays_camera_whole_images": (cast_rays_camera_whole_case,),
    "cast_rays_bwd": (cast_rays_bwd_case, False, False),
    "cast_rays_bwd_whole_images": (cast_rays_bwd_case, False, True),
    "cast_rays_camera_bwd": (cast_rays_bwd_case, True, False),
    "cast_rays_camera_bwd_whole_images": (cast_rays_bwd_case, True, True),
    "random_subset_1": (random_subset_case, 1, 1),
    "random_subset_ragged": (random_subset_case, 3 * 29 * 37, 1499),
    "random_subset_all": (random_subset_case, 1025, 1025),
    "sample_probe": (sample_probe_case, "packed_scatter"),
    "sample_probe_sh3_views": (sample_probe_case, "tile_sh3_views"),
    "sample_probe_attn": (sample_probe_case, "tile_attn"),
    "sample_probe_packed_grid_only": (sample_probe_case, "packed_scatter", True),
}


@pytest.mark.parametrize("name", sorted(CASTS))
def test_ray_casting_and_sampling(name):
    run_contract(*CASTS[name])


@pytest.mark.parametrize("name,tag", [("cast_rays_bwd", "scratch"), ("cast_rays_camera_bwd", "scratch"), ("sample_probe", "workspace")])
def test_ray_casting_refuses_short_sizes(name, tag):
    run_short(CASTS[name][0], tag, *CASTS[name][1:])


@pytest.mark.parametrize("name", ["cast_rays_indexed", "cast_rays_camera"])
def test_ray_casting_of_no_rays_touches_nothing(name):
    run_empty(*CASTS[name])


# ---- per-ray and per-point passes without a workspace of their own, and the point query ---------------------------------------------
@functools.lru_cache(maxsize=None)
def _points(N=1499):
    rng = np.random.default_rng(N)
    pts = rng.uniform(-1.8, 1.8, (N, 3)).astype(np.float32)
    pts[:4] = ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5), (0, 0, 0), (1.5, -1.5, 0.3))
    return pts


def query_case(k, name, packed_only=False):
    L, sc, st = _lib(), scene(name), _stream()
    N, C1 = 1499, sc.F + 1
    dens, feat, pts = k.inp("densities", sc.dens), k.inp("features", sc.feat), k.inp("points", _points())
    rng = np.random.default_rng(2)
    g_out = k.inp("d_out", rng.standard_normal((N, C1)).astype(np.float32))
    g = sc.desc(dens.ptr, feat.ptr)
    gp = C.byref(g)
    ws = k.scratch("workspace", L.voxe_workspace_grad_offset(gp) if packed_only else L.voxe_workspace_bytes(gp, None, 0))
    assert packed_only or ws.nbytes == L.voxe_workspace_grad_offset(gp) + L.voxe_workspace_grad_bytes(gp)
    out, d_dens, d_feat = k.out("out", N * C1), k.out("d_densities", sc.nvox), k.out("d_features", sc.nvox * sc.F)
    k.begin()
    k.call(L.voxe_query_fwd, gp, pts.ptr, k.count(N, "fwd"), out.ptr, 0, ws.ptr, k.size(ws, "fwd", minimum=L.voxe_workspace_grad_offset(gp)), st)
    k.bits(out)
    grid = vo.Grid(sc.dens, sc.feat, AABB, SCALE, abi.ACT_IDENTITY, abi.ACT_SOFTPLUS, sc.kind)
    np.testing.assert_allclose(out.cpu().numpy().reshape(N, C1), vo.query_fwd(grid, _points()), rtol=3e-6, atol=3e-6)
    if packed_only:
        return                                   # (the forward alone, in a workspace that holds the packed grid and nothing else)
    rd_, rf_ = vo.query_bwd(grid, _points(), g_out.cpu().numpy().reshape(N, C1))
    for accumulate in (0, 1):
        k.call(L.voxe_query_bwd, gp, pts.ptr, N, g_out.ptr, d_dens.ptr, d_feat.ptr, accumulate, 0, ws.ptr, k.size(ws, "bwd"), st)
        for b, want in ((d_dens, rd_), (d_feat, rf_)):
            query_grad_close(b.name, b.cpu().numpy(), (1 + accumulate) * want.reshape(-1))
            k.pair(b, 2 * GRAD_REL_L2, f"{b.name} {'+=' if accumulate else '='}")


def normals_case(k, which, name):
    L, sc, st = _lib(), scene(name), _stream()
    dens = k.inp("densities", sc.dens)
    g = sc.desc(dens.ptr, None)                 # (features are not read: NULL is documented)
    if which == "query":
        N = 1499
        pts, out = k.inp("points", _points()), k.out("normals", N * 3)
        k.begin()
        k.call(L.voxe_query_normals, C.byref(g), pts.ptr, k.count(N), out.ptr, st)
        k.bits(out)
        return
    R = sc.R
    ro, rd = k.inp("rays_o", sc.ro), k.inp("rays_d", sc.rd)
    c = sc.cfg()
    normals, depth, acc = k.out("normals", R * 3), k.out("depth", R), k.out("acc", R)
    k.begin()
    k.call(L.voxe_render_normals, C.byref(g), C.byref(c), ro.ptr, rd.ptr, k.count(R), None, normals.ptr, depth.ptr, acc.ptr, st)
    for b in (normals, depth, acc):
        k.bits(b)
    np.testing.assert_allclose(acc.cpu().numpy(), sc.oracle()[0]["acc"].reshape(-1), rtol=0, atol=FWD_ATOL)


def visibility_case(k, name):
    L, sc, st = _lib(), scene(name), _stream()
    R = sc.R
    dens, ro, rd = k.inp("densities", sc.dens), k.inp("rays_o", sc.ro), k.inp("rays_d", sc.rd)
    g, c = sc.desc(dens.ptr, None), sc.cfg()
    zeros = np.zeros(sc.nvox, np.float32)
    mw, mt = k.inout("max_weight", zeros), k.inout("max_trans", zeros)      # accumulators: the caller zeroes them
    k.begin()
    k.call(L.voxe_visibility_accumulate, C.byref(g), C.byref(c), ro.ptr, rd.ptr, k.count(R), None, mw.ptr, mt.ptr, st)
    k.bits(mw), k.bits(mt)
    assert float(mw.t.max()) > 0 and float(mt.t.max()) == 1.0 and float(mw.t.min()) >= 0


def visibility_mask_case(k, dims, dilate):
    L, st = _lib(), _stream()
    rng = np.random.default_rng(dilate)
    vis = rng.uniform(0, 1, dims).astype(np.float32) * (rng.uniform(0, 1, dims) < 0.1)
    vis[0, 0, 0] = np.nan
    src, mask = k.inp("vis", vis.astype(np.float32)), k.out("mask", int(np.prod(dims)), U8)
    k.begin()
    k.call(L.voxe_visibility_mask, src.ptr, *dims, 0.05, dilate, mask.ptr, st)
    k.bits(mask)
    assert set(np.unique(mask.cpu().numpy())) <= {0, 1}


def lift_case(k, name, channels):
    L, sc, st = _lib(), scene(name), _stream()
    R = sc.R
    dens, ro, rd = k.inp("densities", sc.dens), k.inp("rays_o", sc.ro), k.inp("rays_d", sc.rd)
    g, c = sc.desc(dens.ptr, None), sc.cfg()
    rng = np.random.default_rng(channels)
    values = k.inp("values", rng.uniform(-1, 1, (R, channels)).astype(np.float32)) if channels else None
    wv = k.inout("sum_wv", np.zeros(sc.nvox * channels, np.int64)) if channels else None
    w = k.inout("sum_w", np.zeros(sc.nvox, np.int64))
    k.begin()
    k.call(L.voxe_lift_accumulate, C.byref(g), C.byref(c), ro.ptr, rd.ptr, k.count(R), None, P(values), channels, P(wv), w.ptr, st)
    k.bits(w)
    if channels:
        k.bits(wv)
    assert int(w.t.max()) > 0


def distortion_case(k, name, with_loss):
    L, sc, st = _lib(), scene(name), _stream()
    R = sc.R
    dens, ro, rd = k.inp("densities", sc.dens), k.inp("rays_o", sc.ro), k.inp("rays_d", sc.rd)
    g, c = sc.desc(dens.ptr, None), sc.cfg()
    loss = k.out("loss", 1) if with_loss else None
    ray_loss, d_dens = k.out("ray_loss", R), k.out("d_densities", sc.nvox)
    scr = k.scratch("scratch", L.voxe_distortion_scratch_bytes(R)) if with_loss else None
    k.begin()
    k.call(L.voxe_distortion_fwd_bwd, C.byref(g), C.byref(c), ro.ptr, rd.ptr, R, None, 0.7, P(loss), ray_loss.ptr, d_dens.ptr, 0,
           P(scr), k.size(scr, "scratch") if scr else 0, st)
    k.bits(ray_loss)
    if with_loss:
        k.bits(loss)
    k.tol(d_dens, 0.7 * _distortion_reference(name), DISTORTION_GRAD_REL_L2)


@functools.lru_cache(maxsize=None)
def _distortion_reference(name):
    from voxe_hip import ops

    sc = scene(name)
    spec = ops.GridSpec(aabb=AABB, density_scale=SCALE, density_pre_act=abi.ACT_IDENTITY, density_post_act=abi.ACT_SOFTPLUS,
                        feature_kind=sc.kind)
    params = ops.RenderParams(num_samples=sc.S, near=NEAR, far=FAR, perturb=True)
    t = torch.from_numpy
    _, g64 = DR.loss_and_gradient(DR.distortion_host, spec, params, t(sc.dens), t(sc.feat), t(sc.ro), t(sc.rd), None, (5, 3))
    return g64.numpy().reshape(-1)


def distortion_empty_case(k):
    """R == 0 with only the loss outputs: VOXE_OK, no launch (with a d_densities the header has it zeroed: not this case)"""
    L, sc, st = _lib(), scene("packed_scatter"), _stream()
    dens, ro, rd = k.inp("densities", sc.dens), k.inp("rays_o", sc.ro), k.inp("rays_d", sc.rd)
    g, c = sc.desc(dens.ptr, None), sc.cfg()
    loss, ray_loss = k.out("loss", 1), k.out("ray_loss", sc.R)
    scr = k.scratch("scratch", L.voxe_distortion_scratch_bytes(sc.R))
    k.begin()
    k.call(L.voxe_distortion_fwd_bwd, C.byref(g), C.byref(c), ro.ptr, rd.ptr, k.count(sc.R), None, 1.0, loss.ptr, ray_loss.ptr, None, 0,
           scr.ptr, scr.nbytes, st)
    raise AssertionError("only run_empty() runs this case")


def render_bwd_rays_case(k, name):
    L, sc, st = _lib(), scene(name), _stream()
    R = sc.R
    dens, feat = k.inp("densities", sc.dens), k.inp("features", sc.feat)
    ro, rd = k.inp("rays_o", sc.ro), k.inp("rays_d", sc.rd)
    gc, gdep, gacc = (k.inp(n, a) for n, a in zip(("d_colour", "d_depth", "d_acc"), sc.upstream()))
    g, c = sc.desc(dens.ptr, feat.ptr), sc.cfg()
    d_o, d_d = k.out("d_rays_o", R * 3), k.out("d_rays_d", R * 3)
    k.begin()
    for accumulate in (0, 1):
        k.call(L.voxe_render_bwd_rays, C.byref(g), C.byref(c), ro.ptr, rd.ptr, k.count(R), None, gc.ptr, gdep.ptr, gacc.ptr, d_o.ptr,
               d_d.ptr, accumulate, st)
        k.bits(d_o, f"d_rays_o {accumulate}"), k.bits(d_d, f"d_rays_d {accumulate}")
    assert float(d_d.t.abs().max()) > 0


def background_case(k, He, We, R):
    L, st = _lib(), _stream()
    texels, d, colour, acc, g, _, _ = BR.agreement_case(He, We, R)
    tex, rd = k.inp("texels", texels.numpy()), k.inp("rays_d", d.numpy())
    cin, a, gout = k.inp("colour_in", colour.numpy()), k.inp("acc", acc.numpy()), k.inp("d_colour_out", g.numpy())
    cout, d_acc, d_tex, d_rd = k.out("colour_out", R * 3), k.out("d_acc", R), k.out("d_texels", He * We * 3), k.out("d_rays_d", R * 3)
    k.begin()
    env = abi.VoxeEnvMap(tex.ptr, He, We)
    k.call(L.voxe_background_fwd, C.byref(env), rd.ptr, k.count(R, "fwd"), cin.ptr, a.ptr, cout.ptr, st)
    k.bits(cout)
    r_acc, r_tex, r_d, _ = BR.analytic_gradients(acc, d, texels, g)
    for accumulate in (0, 1):
        k.call(L.voxe_background_bwd, C.byref(env), rd.ptr, k.count(R, "bwd"), a.ptr, gout.ptr, d_acc.ptr, d_tex.ptr, d_rd.ptr, accumulate, st)
        k.bits(d_acc, f"d_acc {accumulate}"), k.bits(d_rd, f"d_rays_d {accumulate}")
        k.tol(d_tex, (1 + accumulate) * r_tex.numpy(), BACKGROUND_GRAD_REL_L2, f"d_texels {accumulate}")
    assert BR.rel_l2(d_acc.cpu().reshape(-1), 2 * r_acc) < BACKGROUND_GRAD_REL_L2


def disparity_bwd_case(k, with_inputs):
    L, sc, st = _lib(), scene("packed_scatter"), _stream()
    R = sc.R
    ref = sc.oracle()[0]
    rng = np.random.default_rng(R)
    depth, acc = k.inp("depth", ref["depth"].reshape(-1)), k.inp("acc", ref["acc"].reshape(-1))
    gdisp = k.inp("d_disparity", rng.standard_normal(R).astype(np.float32))
    din = k.inp("d_depth_in", rng.standard_normal(R).astype(np.float32)) if with_inputs else None
    ain = k.inp("d_acc_in", rng.standard_normal(R).astype(np.float32)) if with_inputs else None
    dout, aout = k.out("d_depth_out", R), k.out("d_acc_out", R)
    k.begin()
    k.call(L.voxe_disparity_bwd, depth.ptr, acc.ptr, gdisp.ptr, P(din), P(ain), dout.ptr, aout.ptr, R, st)
    k.bits(dout), k.bits(aout)
    assert bool(torch.isfinite(dout.t).all()) and bool(torch.isfinite(aout.t).all())


PASSES = {
    "query_fwd_bwd_odd": (query_case, "packed_scatter"),
    "query_fwd_bwd_sh3_tiny": (query_case, "scatter_sh3_tiny"),
    "query_fwd_bwd_sh1": (query_case, "tile_two_phase"),
    "query_fwd_bwd_attn_aligned": (query_case, "scatter_attn_aligned"),
    "query_fwd_packed_grid_only": (query_case, "packed_scatter", True),
    "query_normals": (normals_case, "query", "packed_scatter"),
    "query_normals_tiny": (normals_case, "query", "packed_scatter_tiny"),
    "render_normals_image": (normals_case, "render", "tile_s33"),
    "render_normals_views": (normals_case, "render", "views_tile"),
    "render_normals_random": (normals_case, "render", "packed_scatter"),
    "visibility_accumulate_image": (visibility_case, "tile_s33"),
    "visibility_accumulate_views": (visibility_case, "views_tile"),
    "visibility_accumulate_random_tiny": (visibility_case, "packed_scatter_tiny"),
    "visibility_mask_dilate0": (visibility_mask_case, (17, 9, 13), 0),
    "visibility_mask_dilate1": (visibility_mask_case, (17, 9, 13), 1),
    "visibility_mask_dilate1_tiny": (visibility_mask_case, (5, 6, 7), 1),
    "lift_accumulate_coverage": (lift_case, "packed_scatter", 0),
    "lift_accumulate_1": (lift_case, "tile_s33", 1),
    "lift_accumulate_3_views": (lift_case, "views_tile", 3),
    "lift_accumulate_8_tiny": (lift_case, "packed_scatter_tiny", 8),
    "distortion_fwd_bwd": (distortion_case, "packed_scatter", True),
    "distortion_fwd_bwd_no_loss": (distortion_case, "tile_s33", False),
    "distortion_fwd_bwd_views_96": (distortion_case, "views_tile", True),
    "render_bwd_rays": (render_bwd_rays_case, "packed_scatter"),
    "render_bwd_rays_sh2_tiny": (render_bwd_rays_case, "tile_sh2_tiny"),
    "render_bwd_rays_sh3_views": (render_bwd_rays_case, "tile_sh3_views"),
    "background_fwd_bwd_5x7": (background_case, 5, 7, 1499),
    "background_fwd_bwd_2x2": (background_case, 2, 2, 65),
    "disparity_bwd": (disparity_bwd_case, True),
    "disparity_bwd_no_inputs": (disparity_bwd_case, False),
}


@pytest.mark.parametrize("name", sorted(PASSES))
def test_per_ray_and_per_point_passes(name):
    run_contract(*PASSES[name])


@pytest.mark.parametrize("name,tag", [("query_fwd_bwd_odd", "fwd"), ("query_fwd_bwd_odd", "bwd"), ("distortion_fwd_bwd", "scratch")])
def test_per_ray_passes_refuse_short_sizes(name, tag):
    run_short(PASSES[name][0], tag, *PASSES[name][1:])


EMPTY = [("query_normals", "count"), ("render_normals_random", "count"), ("visibility_accumulate_image", "count"),
         ("lift_accumulate_3_views", "count"), ("render_bwd_rays", "count"), ("background_fwd_bwd_5x7", "fwd"),
         ("background_fwd_bwd_5x7", "bwd")]


@pytest.mark.parametrize("name,tag", EMPTY)
def test_per_ray_passes_of_no_rays_touch_nothing(name, tag):
    run_empty(*PASSES[name], tag=tag)


def test_distortion_of_no_rays_touches_nothing():
    run_empty(distortion_empty_case)


# ---- whole-grid passes -----------------------------------------------------------------------------------------------------------
def _pair(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)


def dcl_case(k, n):
    L, st = _lib(), _stream()
    a_np, b_np = _pair(n, n)
    a, b = k.inp("a", a_np), k.inp("b", b_np)
    loss, d_a = k.out("loss", 1), k.out("d_a", n)
    sc = k.scratch("scratch", L.voxe_dcl_scratch_bytes(n))
    k.begin()
    for accumulate in (0, 1):
        k.call(L.voxe_dcl_fwd_bwd, a.ptr, b.ptr, n, 0.7, loss.ptr, d_a.ptr, accumulate, sc.ptr, k.size(sc, "scratch"), st)
        k.bits(loss, f"loss {accumulate}"), k.bits(d_a, f"d_a {accumulate}")
    ref_loss, ref_g = vo.dcl_fwd_bwd(a_np, b_np, 0.7)
    assert abs(float(loss.t) - ref_loss) < 1e-5 * max(1.0, abs(ref_loss)) and rel_l2(d_a.cpu().numpy(), 2 * ref_g) < GRAD_REL_L2


def density_diff_case(k, n, kind, with_loss):
    L, st = _lib(), _stream()
    a_np, b_np = _pair(n, n + kind)
    b_np[::5] = a_np[::5]                        # exact ties: sign(0) = 0
    a, b = k.inp("a", a_np), k.inp("b", b_np)
    loss = k.out("loss", 1) if with_loss else None
    d_a = k.out("d_a", n)
    sc = k.scratch("scratch", L.voxe_dcl_scratch_bytes(n))
    k.begin()
    k.call(L.voxe_density_diff_fwd_bwd, a.ptr, b.ptr, n, kind, 0.7, P(loss), d_a.ptr, 0, sc.ptr,
           k.size(sc, "scratch") if with_loss else sc.nbytes, st)
    k.bits(d_a)
    if with_loss:
        k.bits(loss)
    ref_loss, ref_g = vo.density_diff_fwd_bwd(a_np, b_np, kind, 0.7)
    assert rel_l2(d_a.cpu().numpy(), ref_g) < GRAD_REL_L2
    if with_loss:
        assert abs(float(loss.t) - ref_loss) < 1e-5 * max(1.0, abs(ref_loss))


def feature_correlation_case(k, nvox, F):
    L, st = _lib(), _stream()
    f_np, r_np = _pair(nvox * F, F)
    f, r = k.inp("f", f_np), k.inp("r", r_np)
    loss, d_f = k.out("loss", 1), k.out("d_f", nvox * F)
    sc = k.scratch("scratch", L.voxe_dcl_scratch_bytes(nvox))
    k.begin()
    k.call(L.voxe_feature_correlation_fwd_bwd, f.ptr, r.ptr, nvox, F, 0.7, loss.ptr, d_f.ptr, 0, sc.ptr, k.size(sc, "scratch"), st)
    k.bits(loss), k.bits(d_f)
    ref_loss, ref_g = vo.feature_correlation_fwd_bwd(f_np.reshape(nvox, F), r_np.reshape(nvox, F), 0.7)
    assert rel_l2(d_f.cpu().numpy(), ref_g.reshape(-1)) < GRAD_REL_L2 and abs(float(loss.t) - ref_loss) < 1e-4 * abs(ref_loss)


def tv_case(k, dims, channels):
    L, st = _lib(), _stream()
    rng = np.random.default_rng(sum(dims) + channels)
    grid_np = rng.standard_normal((*dims, channels)).astype(np.float32)
    grid_np[1:3, 2:5] = grid_np[0:1, 2:5]
    grid = k.inp("grid", grid_np)
    loss, d_grid = k.out("loss", 1), k.out("d_grid", grid_np.size)
    sc = k.scratch("scratch", L.voxe_tv_scratch_bytes(*dims, channels))
    k.begin()
    for accumulate in (0, 1):
        k.call(L.voxe_tv_fwd_bwd, grid.ptr, *dims, channels, 0.7, loss.ptr, d_grid.ptr, accumulate, sc.ptr, k.size(sc, "scratch"), st)
        k.bits(loss, f"loss {accumulate}"), k.bits(d_grid, f"d_grid {accumulate}")
    ref_loss, ref_g = vo.tv_fwd_bwd(grid_np, 0.7)
    assert rel_l2(d_grid.cpu().numpy(), 2 * ref_g.reshape(-1)) < GRAD_REL_L2 and abs(float(loss.t) - ref_loss) < 1e-5 * max(1.0, abs(ref_loss))


def adam_case(k, n):
    L, st = _lib(), _stream()
    rng = np.random.default_rng(n)
    p0, g0 = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    m0, v0 = (0.1 * rng.standard_normal(n)).astype(np.float32), (0.01 * rng.uniform(0, 1, n)).astype(np.float32)
    p, m, v = k.inout("param", p0), k.inout("exp_avg", m0), k.inout("exp_avg_sq", v0)
    g = k.inp("grad", g0)
    k.begin()
    k.call(L.voxe_adam_step, p.ptr, g.ptr, m.ptr, v.ptr, n, 1e-2, 0.9, 0.999, 1e-8, 3, st)
    k.bits(p), k.bits(m), k.bits(v)
    vo.adam_step(p0, g0, m0, v0, 1e-2, 0.9, 0.999, 1e-8, 3)
    np.testing.assert_allclose(p.cpu().numpy(), p0, rtol=2e-6, atol=1e-7)


def upsample_case(k, src_dims, dst_dims, channels):
    L, st = _lib(), _stream()
    rng = np.random.default_rng(sum(src_dims) + channels)
    src_np = rng.standard_normal((*src_dims, channels)).astype(np.float32)
    src, dst = k.inp("src", src_np), k.out("dst", int(np.prod(dst_dims)) * channels)
    k.begin()
    k.call(L.voxe_upsample_trilinear, src.ptr, *src_dims, channels, dst.ptr, *dst_dims, st)
    k.bits(dst)
    assert np.array_equal(dst.cpu().numpy(), vo.upsample_trilinear(src_np, dst_dims).reshape(-1))


def resample_case(k, mode, degree, with_taken):
    """a rotated, shifted copy of (17, 9, 13) on an (11, 15, 10) lattice; UNION merges into an existing destination"""
    import transform_ref as TR
    from voxe_hip import ops

    L, st = _lib(), _stream()
    src_dims, dst_dims = (17, 9, 13), (11, 15, 10)
    channels = 5 if degree < 0 else 3 * (degree + 1) ** 2
    n_dst = int(np.prod(dst_dims))
    sd, sf = _grid(src_dims, channels, seed=2)
    rot = TR.random_orthogonal(5, 1.0)
    A, b = TR.index_map(src_dims, (-1.5,) * 3, tuple(3.0 / n for n in src_dims), dst_dims, (-1.2,) * 3, tuple(2.6 / n for n in dst_dims),
                        rot, (0.1, -0.05, 0.2), 1.1)
    blocks = None
    if degree >= 0:
        from thre3d_atom.thre3d_reprs.transform import sh_rotation_matrices

        blocks = sh_rotation_matrices(rot, degree)
    xf = ops.make_resample(A, b, blocks, degree, abi.ACT_ABS, 0.25, mode)
    src_d, src_f = k.inp("src_densities", sd), k.inp("src_features", sf)
    if mode == abi.RESAMPLE_UNION:
        dd, df = _grid(dst_dims, channels, seed=3)
        dst_d, dst_f = k.inout("dst_densities", 0.3 * dd), k.inout("dst_features", df)
    else:
        dst_d, dst_f = k.out("dst_densities", n_dst), k.out("dst_features", n_dst * channels)
    taken = k.out("taken", n_dst, U8) if with_taken else None
    k.begin()
    k.call(L.voxe_grid_resample, src_d.ptr, src_f.ptr, *src_dims, channels, dst_d.ptr, dst_f.ptr, *dst_dims, C.byref(xf), P(taken), st)
    k.bits(dst_d), k.bits(dst_f)
    if with_taken:
        k.bits(taken)
        assert 0 < int(taken.t.sum()) < n_dst


GRID_PASSES = {
    **{f"dcl_{n}": (dcl_case, n) for n in (17 * 9 * 13, 5 * 6 * 7, 8 * 8 * 16)},
    **{f"density_diff_{'l2' if kind == 1 else 'l1'}_{'loss' if wl else 'no_loss'}": (density_diff_case, 17 * 9 * 13, kind, wl)
       for kind in (abi.DREG_L2, abi.DREG_L1) for wl in (True, False)},
    "feature_correlation_F3": (feature_correlation_case, 17 * 9 * 13, 3),
    "feature_correlation_F64": (feature_correlation_case, 5 * 6 * 7, 64),
    "tv_C1": (tv_case, (17, 9, 13), 1),
    "tv_C3": (tv_case, (5, 6, 7), 3),
    "tv_C4": (tv_case, (17, 9, 13), 4),
    "tv_C1_aligned": (tv_case, (8, 8, 16), 1),
    **{f"adam_step_{n}": (adam_case, n) for n in (1, 255, 1025)},
    "upsample_odd_to_odd_C1": (upsample_case, (5, 6, 7), (17, 9, 13), 1),
    "upsample_odd_to_odd_C3": (upsample_case, (5, 7, 3), (9, 11, 13), 3),
    **{f"resample_replace_deg{d}": (resample_case, abi.RESAMPLE_REPLACE, d, d % 2 == 0) for d in (-1, 0, 1, 2, 3)},
    **{f"resample_union_deg{d}": (resample_case, abi.RESAMPLE_UNION, d, d % 2 != 0) for d in (-1, 0, 1, 2, 3)},
}


@pytest.mark.parametrize("name", sorted(GRID_PASSES))
def test_whole_grid_passes(name):
    run_contract(*GRID_PASSES[name])


@pytest.mark.parametrize("name", ["dcl_1989", "density_diff_l2_loss", "density_diff_l1_loss", "feature_correlation_F3", "feature_correlation_F64",
                                  "tv_C1", "tv_C3", "tv_C4"])
def test_whole_grid_passes_refuse_a_short_scratch(name):
    run_short(GRID_PASSES[name][0], "scratch", *GRID_PASSES[name][1:])


# ---- refinement, mesh, image loss -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _graph(dims, F=3):
    rng = np.random.default_rng(sum(dims))
    dens = (rng.uniform(0, 1, dims) * (rng.uniform(0, 1, dims) < 0.6)).astype(np.float32)
    feat = rng.uniform(0, 1, (*dims, F)).astype(np.float32)
    return dens, feat


def graph_build_case(k, dims, dilate):
    L, st = _lib(), _stream()
    dens_np, feat_np = _graph(dims)
    n = int(np.prod(dims))
    dens, feat = k.inp("density_grid", dens_np), k.inp("feature_grid", feat_np)
    mask, cap = k.out("node_mask", n, U8), k.out("cap", 6 * n, I32)
    k.begin()
    k.call(L.voxe_graph_build, dens.ptr, feat.ptr, *dims, 3, 0.1, dilate, mask.ptr, cap.ptr, st)
    k.bits(mask), k.bits(cap)
    ref_mask, ref_cap = vo.graph_build(dens_np, feat_np, 0.1, bool(dilate))
    assert np.array_equal(mask.cpu().numpy(), ref_mask.reshape(-1)) and np.array_equal(cap.cpu().numpy(), ref_cap.reshape(-1))


def graphcut_case(k, dims):
    L, st = _lib(), _stream()
    dens_np, feat_np = _graph(dims)
    n = int(np.prod(dims))
    mask_np, cap_np = vo.graph_build(dens_np, feat_np, 0.1, True)
    rng = np.random.default_rng(n)
    term_np = np.zeros(dims, np.int8)
    nodes = np.argwhere(mask_np.reshape(dims) > 0)
    for sign, rows in ((1, nodes[rng.choice(len(nodes), 5, replace=False)]), (-1, nodes[rng.choice(len(nodes), 5, replace=False)])):
        for r in rows:
            term_np[tuple(r)] = sign
    mask, term = k.inp("node_mask", mask_np.astype(np.uint8)), k.inp("terminal", term_np)
    cap = k.inout("cap", cap_np.astype(np.int32))                      # consumed: holds the residual capacities on return
    seg, flow = k.out("segment", n, U8), k.out("flow", 1, I64)
    sc = k.scratch("scratch", L.voxe_graphcut_scratch_bytes(*dims))
    k.begin()
    k.call(L.voxe_graphcut, mask.ptr, term.ptr, cap.ptr, *dims, seg.ptr, flow.ptr, sc.ptr, k.size(sc, "scratch"), st)
    k.bits(seg), k.bits(flow)
    ref_seg, ref_flow, _ = vo.graphcut(mask_np, term_np, cap_np)
    assert np.array_equal(seg.cpu().numpy(), ref_seg.reshape(-1)) and int(flow.t) == int(ref_flow)


def cc_case(k, dims, kk):
    L, st = _lib(), _stream()
    rng = np.random.default_rng(sum(dims) + kk)
    mask_np = (rng.uniform(0, 1, dims) < 0.22).astype(np.uint8) * 7
    n = int(np.prod(dims))
    mask = k.inp("mask", mask_np)
    labels, num = k.out("labels", n, I32), k.out("num_components", 1, I32)
    sc = k.scratch("scratch", L.voxe_cc_scratch_bytes(*dims, kk))
    k.begin()
    k.call(L.voxe_cc_largest_k, mask.ptr, *dims, kk, labels.ptr, num.ptr, sc.ptr, k.size(sc, "scratch"), st)
    k.bits(labels), k.bits(num)
    ref_labels, ref_num = vo.cc_largest_k(mask_np, kk)
    assert np.array_equal(labels.cpu().numpy(), ref_labels.reshape(-1)) and int(num.t) == int(ref_num)


def attn_masked_l1_case(k, n):
    L, st = _lib(), _stream()
    rng = np.random.default_rng(n)
    render_np = (rng.uniform(-0.3, 1.0, n)).astype(np.float32)
    render, amap = k.inp("render", render_np), k.inp("attn_map", rng.uniform(0, 1, n).astype(np.float32))
    d_render, loss = k.out("d_render", n), k.out("loss", 1)
    sc = k.scratch("scratch", L.voxe_attn_masked_l1_scratch_bytes())
    k.begin()
    k.call(L.voxe_attn_masked_l1, render.ptr, amap.ptr, n, d_render.ptr, loss.ptr, sc.ptr, k.size(sc, "scratch"), st)
    k.bits(d_render), k.bits(loss)
    assert bool((d_render.t[render.t <= 0] == 0).all()) and float(loss.t) > 0


def attn_refine_case(k, name, tv_weight):
    """voxe_attn_refine_step: render -> masked L1 -> backward -> TV -> Adam of the attention tensor, densities frozen"""
    L, sc, st = _lib(), scene(name), _stream()
    R, nvox = sc.R, sc.nvox
    rng = np.random.default_rng(R)
    dens = k.inp("densities", sc.dens)                     # frozen: a const input of this call
    attn = k.inout("attn", sc.feat)
    ro, rd = k.inp("rays_o", sc.ro), k.inp("rays_d", sc.rd)
    amap = k.inp("attn_map", rng.uniform(0, 1, R).astype(np.float32))
    zeros = np.zeros(nvox, np.float32)
    m, v = k.inout("exp_avg", zeros), k.inout("exp_avg_sq", zeros)
    losses, image = k.out("losses", 2), k.out("attn_render", R)
    g, c = sc.desc(dens.ptr, attn.ptr), sc.cfg()
    _, inference, full, _ = _ws_sizes(sc, g, c)
    ws = k.scratch("workspace", full)
    scr = k.scratch("scratch", L.voxe_attn_refine_scratch_bytes(C.byref(g), R))
    k.begin()
    rs = abi.VoxeAttnRefineStep()
    rs.attn_map, rs.tv_weight, rs.tv_loss_always = amap.ptr, tv_weight, 1
    rs.lr, rs.beta1, rs.beta2, rs.eps, rs.step = LR, BETA1, 0.999, 1e-8, 1
    rs.exp_avg, rs.exp_avg_sq, rs.losses, rs.attn_render, rs.zero_gradient_first = m.ptr, v.ptr, losses.ptr, image.ptr, 1
    before = attn.cpu()
    k.call(L.voxe_attn_refine_step, C.byref(g), C.byref(c), C.byref(rs), ro.ptr, rd.ptr, R, ws.ptr, k.size(ws, "workspace", minimum=inference),
           scr.ptr, k.size(scr, "scratch"), st)
    k.bits(image), k.bits(losses)
    assert not torch.equal(attn.cpu(), before)
    k.pair(m, 2 * GRAD_REL_L2), k.pair(v, 2 * GRAD_REL_L2), k.pair_abs(attn, _well_above_noise(m), 2 * 1e-3 * LR)


def recon_case(k, name, diffuse):
    """voxe_recon_step without a hint: batch assembly -> render(s) -> losses -> backward -> grid step, in exact-size workspaces"""
    L, sc, st = _lib(), scene(name), _stream()
    H, W, K, batch = 29, 37, 3, 1499
    rng = np.random.default_rng(batch)
    dens, feat = k.inout("densities", sc.dens), k.inout("features", sc.feat)
    poses = k.inp("poses", _poses(K))
    rows = k.inp("image_rows", np.array([2, 0, 3], np.int64))
    images = k.inp("images", rng.uniform(0, 1, (4, 3, H, W)).astype(np.float32))
    zeros_d, zeros_f = np.zeros(sc.nvox, np.float32), np.zeros(sc.nvox * sc.F, np.float32)
    m_d, v_d = k.inout("exp_avg_densities", zeros_d), k.inout("exp_avg_sq_densities", zeros_d)
    m_f, v_f = k.inout("exp_avg_features", zeros_f), k.inout("exp_avg_sq_features", zeros_f)
    losses = k.out("losses", 4)
    g = sc.desc(dens.ptr, feat.ptr)
    c = sc.cfg(linear_grad=True, image_width=0, image_height=0)
    gp, cp = C.byref(g), C.byref(c)
    nbytes = L.voxe_workspace_bytes(gp, cp, batch)
    if diffuse and sc.deg == 0:
        nbytes = max(nbytes, L.voxe_workspace_bytes(gp, cp, 2 * batch))
    ws = k.scratch("workspace", nbytes)
    least = _ws_sizes(sc, g, c, batch)[1]          # (below the paired launch's size the step takes two renders: not an error)
    ws2, least2 = None, 0
    if diffuse:
        c2 = sc.cfg(linear_grad=True, image_width=0, image_height=0, render_diffuse=True)
        ws2 = k.scratch("workspace2", max(nbytes, L.voxe_workspace_bytes(gp, C.byref(c2), batch)))
        least2 = _ws_sizes(sc, g, c2, batch)[1]
    scr = k.scratch("scratch", L.voxe_recon_scratch_bytes(batch))
    k.begin()
    rs = abi.VoxeReconStep()
    rs.H, rs.W, rs.focal, rs.poses, rs.image_rows, rs.images, rs.num_images = H, W, _focal(W), poses.ptr, rows.ptr, images.ptr, 4
    rs.K, rs.batch, rs.diffuse_regularisation = K, batch, int(diffuse)
    rs.lr, rs.beta1, rs.beta2, rs.eps, rs.step_densities, rs.step_features = LR, BETA1, 0.999, 1e-8, 1, 1
    rs.exp_avg_densities, rs.exp_avg_sq_densities, rs.exp_avg_features, rs.exp_avg_sq_features = m_d.ptr, v_d.ptr, m_f.ptr, v_f.ptr
    rs.losses, rs.zero_gradient_first = losses.ptr, 1
    before = dens.cpu()
    k.call(L.voxe_recon_step, gp, cp, C.byref(rs), ws.ptr, k.size(ws, "workspace", minimum=least), P(ws2),
           k.size(ws2, "workspace2", minimum=least2) if ws2 else 0, scr.ptr, k.size(scr, "scratch"), st)
    assert not torch.equal(dens.cpu(), before)
    # (without the diffuse render its two loss values are not written: the header says so)
    live = 4 if diffuse else 2
    got = losses.cpu()
    assert bool(torch.isfinite(got[:live]).all()) and float(got[0]) > 0 and float(got[1]) > 0
    assert bool((losses.t[live:].view(U8) == k.pattern).all())
    k.pair_abs(losses, np.arange(4) < live, 1e-5)
    for b in (m_d, m_f, v_d, v_f):
        k.pair(b, 2 * GRAD_REL_L2)
    k.pair_abs(dens, _well_above_noise(m_d), 2 * 1e-3 * LR), k.pair_abs(feat, _well_above_noise(m_f), 2 * 1e-3 * LR)


@functools.lru_cache(maxsize=None)
def _blob(dims):
    x, y, z = (np.linspace(-1, 1, n, dtype=np.float32) for n in dims)
    r = np.sqrt(x[:, None, None] ** 2 + (1.3 * y[None, :, None]) ** 2 + z[None, None, :] ** 2)
    return (1.2 - 2.0 * r).astype(np.float32)[..., None]


def _mesh_calls(k, dims, with_mask, capacity):
    """declare the buffers of count + emit; -> a function that runs both after k.begin()"""
    L, st = _lib(), _stream()
    dens = k.inp("densities", _blob(dims))
    mask_np = np.ones(dims, np.uint8)
    mask_np[: dims[0] // 3] = 0
    mask = k.inp("mask", mask_np) if with_mask else None
    totals = k.out("totals", 2, I64)
    sc = k.scratch("scratch", L.voxe_mesh_scratch_bytes(*dims))
    verts = k.out("vertices", 3 * capacity[0]) if capacity else None
    faces = k.out("faces", 3 * capacity[1], I32) if capacity else None

    def run():
        g = make_grid_desc(dens.ptr, None, dims, 3, AABB, 1.0, abi.ACT_IDENTITY, abi.ACT_RELU, abi.FEAT_SH)
        k.call(L.voxe_mesh_count, C.byref(g), 0.2, P(mask), totals.ptr, sc.ptr, k.size(sc, "count"), st)
        k.bits(totals)
        if capacity:
            k.call(L.voxe_mesh_emit, C.byref(g), 0.2, P(mask), verts.ptr, capacity[0], faces.ptr, capacity[1], sc.ptr, k.size(sc, "emit"), st)
            k.bits(verts), k.bits(faces, minus_one_ok=False)
        return tuple(int(x) for x in totals.cpu())

    return run


@functools.lru_cache(maxsize=None)
def _mesh_totals(dims, with_mask):
    from contract import K

    k = K(0x00)
    run = _mesh_calls(k, dims, with_mask, None)
    k.begin()
    return run()


def mesh_case(k, dims, with_mask):
    """voxe_mesh_count / voxe_mesh_emit with vertices and faces of exactly the counted capacity"""
    V, T = _mesh_totals(dims, with_mask)
    assert V > 8 and T > 8
    run = _mesh_calls(k, dims, with_mask, (V, T))
    k.begin()
    assert run() == (V, T)


def ssim_case(k, N, H, W, channels, with_grad):
    import ssim_ref as SR

    L, st = _lib(), _stream()
    x_t, y_t = SR.noise(3, N, H, W, channels)
    x, y = k.inp("x", x_t.numpy()), k.inp("y", y_t.numpy())
    mean, per_image = k.out("mean", 1), k.out("per_image", N)
    smap = k.out("ssim_map", N * (H - 10) * (W - 10) * channels)
    d_x = k.out("d_x", N * H * W * channels) if with_grad else None
    sc = k.scratch("scratch", L.voxe_ssim_scratch_bytes(N, H, W, channels, int(with_grad)))
    k.begin()
    for accumulate in ((0, 1) if with_grad else (0,)):
        k.call(L.voxe_ssim_fwd_bwd, x.ptr, y.ptr, N, H, W, channels, 1.0, 0.7, mean.ptr, per_image.ptr, smap.ptr, P(d_x), accumulate,
               sc.ptr, k.size(sc, "scratch"), st)
        for b in (mean, per_image, smap) + ((d_x,) if with_grad else ()):
            k.bits(b, f"{b.name} {accumulate}")
    ref_mean = float(SR.ssim64(x_t.double(), y_t.double())[0])
    assert abs(float(mean.t) - ref_mean) < 1e-5


REFINE = {
    "graph_build_dilate": (graph_build_case, (17, 9, 13), 1),
    "graph_build_plain_tiny": (graph_build_case, (5, 6, 7), 0),
    "graphcut": (graphcut_case, (17, 9, 13)),
    "graphcut_aligned": (graphcut_case, (8, 8, 16)),
    **{f"cc_largest_k_{'x'.join(map(str, d))}_k{kk}": (cc_case, d, kk) for d in ((1, 9, 40), (20, 33, 17)) for kk in (1, 10)},
    "attn_masked_l1": (attn_masked_l1_case, 37 * 29),
    "attn_masked_l1_1": (attn_masked_l1_case, 1),
    "attn_refine_step_tv": (attn_refine_case, "tile_attn", 0.05),
    "attn_refine_step_no_tv_aligned": (attn_refine_case, "scatter_attn_aligned", 0.0),
    "recon_step_paired": (recon_case, "packed_scatter", True),
    "recon_step_single": (recon_case, "packed_scatter_tiny", False),
    "recon_step_sh1_two_renders": (recon_case, "region_sh1", True),
    "mesh_count_emit": (mesh_case, (17, 9, 13), False),
    "mesh_count_emit_masked_tiny": (mesh_case, (5, 6, 7), True),
    "mesh_count_emit_aligned": (mesh_case, (8, 8, 16), True),
    "ssim_2x27x43x3_grad": (ssim_case, 2, 27, 43, 3, True),
    "ssim_2x27x43x3": (ssim_case, 2, 27, 43, 3, False),
    "ssim_one_window_grad": (ssim_case, 1, 11, 11, 1, True),
    "ssim_one_window": (ssim_case, 1, 11, 11, 1, False),
}


@pytest.mark.parametrize("name", sorted(REFINE))
def test_refinement_mesh_and_image_loss(name):
    run_contract(*REFINE[name])


@pytest.mark.parametrize("name,tag", [("graphcut", "scratch"), ("cc_largest_k_20x33x17_k10", "scratch"), ("attn_masked_l1", "scratch"),
                                      ("attn_refine_step_tv", "workspace"), ("attn_refine_step_tv", "scratch"), ("recon_step_paired", "scratch"),
                                      ("recon_step_single", "workspace"), ("recon_step_sh1_two_renders", "workspace2"),
                                      ("mesh_count_emit", "count"), ("mesh_count_emit", "emit"), ("ssim_2x27x43x3_grad", "scratch"),
                                      ("ssim_one_window", "scratch")])
def test_refinement_mesh_and_image_loss_refuse_short_sizes(name, tag):
    run_short(REFINE[name][0], tag, *REFINE[name][1:])
