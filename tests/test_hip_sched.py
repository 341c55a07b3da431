"""Cost-ordered block list of the lean SH-0 tile kernels: the list the library builds in front of the lean
forward against a numpy restatement, the forward with the order on = the forward with it off bit for bit, the backward on / off
against the oracle and against each other, and the list never outliving the forward it belongs to.

Switch: VoxeDispatch::tile_map 0 (auto) = cost order where a launch is large enough, 1 = the static interleaved map (off),
4 = cost order at every launch size.  Bounds: gradients vs the oracle rel-L2 < 1e-4 (tests/test_hip_configs.py), two HIP
backwards of one render that differ in the order of their float atomics rel-L2 < 2e-6 (tests/test_hip_r05.py: lean vs general
kernel)."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import rel_l2
from synth import FAR, NEAR, RADIUS, focal_for, random_grid, synth_pose_angles
from voxe_hip import abi
from voxe_hip.desc import make_render_cfg

from oracle import voxe_oracle as vo

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import gpu_helpers as gh
    from thre3d_atom.utils.imaging_utils import pose_spherical

AABB = [(-1.5, 1.5)] * 3
S = 256
GRAD_TOL = 1e-4      # vs the oracle
ORDER_TOL = 2e-6     # two summation orders of the same float atomics
BUCKET = 4           # VOXE_SCHED_BUCKET of the shipped build
EMPTY = 0x80000000


def _rays(hw, cam, rows=None):
    yaw, pitch = synth_pose_angles(cam, 100)
    pose = pose_spherical(yaw, pitch, RADIUS)
    o, d = vo.cast_rays(hw, hw, focal_for(hw), pose.rotation.numpy(), pose.translation.numpy())
    if rows is not None:      # a strong-scaling rank's band of image rows
        o, d = o[rows[0] * hw:rows[1] * hw], d[rows[0] * hw:rows[1] * hw]
    return np.ascontiguousarray(o, dtype=np.float32), np.ascontiguousarray(d, dtype=np.float32)


def _grid(side):
    dens, feat = random_grid(side)
    return vo.Grid(dens.numpy(), feat.numpy(), AABB, 100.0 / 3.0, abi.ACT_IDENTITY, abi.ACT_SOFTPLUS)


def _params(cfg, width, height=0, **disp):
    from voxe_hip.dispatch import Dispatch
    return gh.params_of(cfg, image_width=width, image_height=height, dispatch=Dispatch(**disp))


def _layout(spec, params, td, tf, R, rng):
    from voxe_hip import ops
    from voxe_hip.runtime import lib
    fn = lib().voxe_tile_sched_debug_layout
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    g, c = ops._descs(spec, params, td, tf, rng[0], rng[1], False)
    out = (C.c_int64 * 4)()
    assert fn(C.byref(g), C.byref(c), R, out) == 0
    return [int(v) for v in out]


def _forward(spec, params, td, tf, to, tdir, ws, rng):
    from voxe_hip import ops
    outs = [torch.empty((to.shape[0], n), device="cuda") for n in (3, 1, 1, 1)]
    ops.render_fwd_into(spec, params, td, tf, to, tdir, None, *outs, ws, rng)
    torch.cuda.synchronize()
    return outs


def _backward(spec, params, td, tf, to, tdir, outs, grads, ws, rng):
    from voxe_hip import ops
    d_d, d_f = torch.zeros_like(td), torch.zeros_like(tf)
    ops.render_bwd_into(spec, params, td, tf, to, tdir, None, outs[0], outs[1], outs[2], grads[0], grads[1], grads[2], d_d, d_f, ws, rng)
    torch.cuda.synchronize()
    return gh.n(d_d), gh.n(d_f)


def _table(ws, layout):
    applies, off, nb, _ = layout
    assert applies == 1
    buf = ws.buf[off:off + 5 * nb].cpu().numpy()
    return buf[:4 * nb].view(np.int32).view(np.uint32).copy(), buf[4 * nb:].copy()


def _restated_table(o, d, width, height, seg_len):
    """inside_range (voxe_device.hpp) in float32, the tile -> ray map of the lean kernels, the stable bucket sort"""
    f = np.float32
    lo, hi = f(AABB[0][0]), f(AABB[0][1])
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = f(1.0) / d
        t0, t1 = (lo - o) * inv, (hi - o) * inv
    par = d == 0
    tmin = np.where(par, f(-3.0e38), np.minimum(t0, t1))
    tmax = np.where(par, f(3.0e38), np.maximum(t0, t1))
    t_in = np.maximum(f(-3.0e38), tmin.max(-1))
    t_out = np.minimum(f(3.0e38), tmax.min(-1))
    outside = (par & ~((o > lo) & (o < hi))).any(-1)
    invz = f(1.0) / (f(FAR) - f(NEAR))
    sm1 = f(S - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.floor(((t_in - f(NEAR)) * invz) * sm1) - f(2.0)
        b = np.ceil(((t_out - f(NEAR)) * invz) * sm1) + f(2.0)
    a, b = np.maximum(a, f(0.0)), np.minimum(b, sm1)
    miss = outside | (t_in > t_out) | (a > b)
    k_lo = np.where(miss, 1, a.astype(np.int64))
    k_hi = np.where(miss, 0, b.astype(np.int64))
    ntx, nty = (width + 7) // 8, (height + 7) // 8
    ntp = (ntx * nty + 7) // 8 * 8
    nseg = (S + seg_len - 1) // seg_len
    pad = lambda v, fill: np.pad(v.reshape(height, width), ((0, nty * 8 - height), (0, ntx * 8 - width)), constant_values=fill)
    k_lo, k_hi = pad(k_lo, 1), pad(k_hi, 0)
    cost = np.zeros((nseg, ntp), np.int64)
    for seg in range(nseg):
        ks, ke = seg * seg_len, min(S, (seg + 1) * seg_len) - 1
        lo_s, hi_s = np.maximum(k_lo, ks), np.minimum(k_hi, ke)
        has = lo_s <= hi_s
        kmin = np.where(has, lo_s, 1 << 30).reshape(nty, 8, ntx, 8).min((1, 3))
        kmax = np.where(has, hi_s, -1).reshape(nty, 8, ntx, 8).max((1, 3))
        cost[seg, :ntx * nty] = np.where(kmin <= kmax, kmax - kmin + 1, 0).reshape(-1)
    cost = cost.reshape(-1)
    nbk = (seg_len + BUCKET - 1) // BUCKET + 1
    rank = np.where(cost == 0, nbk - 1, nbk - 1 - np.minimum((cost + BUCKET - 1) // BUCKET, nbk - 1))
    order = np.argsort(rank, kind="stable").astype(np.uint32)
    return np.where(cost[order] == 0, order | np.uint32(EMPTY), order), cost


@pytest.mark.parametrize("hw,cam,rows,tile_map", [(400, 3, None, 0), (400, 38, None, 0), (400, 88, None, 0), (100, 3, None, 4),
                                                   (400, 3, (96, 296), 4)])
def test_block_list_equals_its_restatement_and_is_reproducible(hw, cam, rows, tile_map):
    """every block of the launch appears exactly once, the ones with samples longest bucket first in launch order inside a
    bucket, the empty ones behind them and marked; costs and order equal the restatement (a pure function of rays and
    configuration); a second build is bit-identical.  The list does not depend on the grid's values: a small grid."""
    from voxe_hip import ops
    grid = _grid(32)
    o, d = _rays(hw, cam, rows)
    height = hw if rows is None else rows[1] - rows[0]
    cfg = make_render_cfg(S, NEAR, FAR, perturb=True, white_bkgd=True, seed=42, rng_offset=7)
    params = _params(cfg, hw, 0 if rows is None else height, tile_map=tile_map)
    spec, td, tf, to, tdir = gh.spec_of(grid), gh.t(grid.densities), gh.t(grid.features), gh.t(o), gh.t(d)
    layout = _layout(spec, params, td, tf, o.shape[0], (42, 7))
    seg_len = 16 if o.shape[0] <= 20000 else 32
    want, want_cost = _restated_table(o, d, hw, height, seg_len)
    assert layout[2] == want.size
    ws = ops.Workspace()
    _forward(spec, params, td, tf, to, tdir, ws, (42, 7))
    got, got_cost = _table(ws, layout)
    assert np.array_equal(np.sort(got & np.uint32(EMPTY - 1)), np.arange(want.size, dtype=np.uint32))
    assert np.array_equal(got_cost, want_cost.astype(np.uint8))
    assert (want_cost > 0).sum() > want.size // 3        # (a camera that sees the volume)
    assert np.array_equal((got & np.uint32(EMPTY)) != 0, got_cost[got & np.uint32(EMPTY - 1)] == 0)
    assert np.array_equal(got, want)
    ws.buf[layout[1]:layout[1] + 5 * layout[2]].fill_(0xFF)
    ws.invalidate()
    _forward(spec, params, td, tf, to, tdir, ws, (42, 7))
    again, _ = _table(ws, layout)
    assert np.array_equal(again, got)
    # the static maps build no list; small launches of the default dispatch do not either
    assert _layout(spec, _params(cfg, hw, 0 if rows is None else height, tile_map=1), td, tf, o.shape[0], (42, 7))[0] == 0
    if tile_map == 4:
        assert _layout(spec, _params(cfg, hw, 0 if rows is None else height), td, tf, o.shape[0], (42, 7))[0] == 0


@pytest.mark.parametrize("hw,cam,oracle", [(400, 3, True), (400, 38, True), (400, 88, False), (100, 7, False)])
def test_cost_order_changes_no_forward_bit_and_only_the_backwards_summation_order(hw, cam, oracle):
    """forward on == forward off, all four outputs, NaN pattern of the disparity included; backward on / off each against the
    oracle (cameras 3 and 38: the bench camera and an oblique one) and against each other"""
    from voxe_hip import ops
    grid = _grid(160 if hw == 400 else 64)
    o, d = _rays(hw, cam)
    cfg = make_render_cfg(S, NEAR, FAR, perturb=True, white_bkgd=True, seed=42, rng_offset=7)
    spec, td, tf, to, tdir = gh.spec_of(grid), gh.t(grid.densities), gh.t(grid.features), gh.t(o), gh.t(d)
    r = np.random.default_rng(100 + cam)
    gc = r.standard_normal((o.shape[0], 3)).astype(np.float32)
    gdep = (0.1 * r.standard_normal((o.shape[0], 1))).astype(np.float32)
    gacc = (0.1 * r.standard_normal((o.shape[0], 1))).astype(np.float32)
    grads = [gh.t(gc), gh.t(gdep), gh.t(gacc)]
    got = {}
    for name, tile_map in (("on", 0 if hw == 400 else 4), ("off", 1)):
        params = _params(cfg, hw, tile_map=tile_map, tile_qsplit=1 if hw != 400 else 0)
        assert _layout(spec, params, td, tf, o.shape[0], (42, 7))[0] == (1 if name == "on" else 0)
        ws = ops.Workspace()
        outs = _forward(spec, params, td, tf, to, tdir, ws, (42, 7))
        got[name] = [gh.n(x) for x in outs] + list(_backward(spec, params, td, tf, to, tdir, outs, grads, ws, (42, 7)))
    for a, b in zip(got["on"][:4], got["off"][:4]):
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a, b, equal_nan=True)
    err = (rel_l2(got["on"][4], got["off"][4]), rel_l2(got["on"][5], got["off"][5]))
    print("on vs off", hw, cam, err)
    assert err[0] < ORDER_TOL and err[1] < ORDER_TOL, err
    if oracle:
        rd, rf = vo.render_bwd(grid, cfg, o, d, gc, d_depth=gdep[:, 0], d_acc=gacc[:, 0])
        for name in ("on", "off"):
            e = (rel_l2(got[name][4], rd), rel_l2(got[name][5], rf))
            print(name, "vs oracle", hw, cam, e)
            assert e[0] < GRAD_TOL and e[1] < GRAD_TOL, (name, e)


@pytest.mark.parametrize("case", ["other_rays_through_the_general_kernel", "smaller_image_in_the_same_workspace"])
def test_a_block_list_never_outlives_its_forward(case):
    """the list is valid exactly as long as the depth-segment states next to it: a forward of other rays through another kernel
    (VoxeDispatch::tile_lean = -1), or of a smaller image, in the same workspace, then a backward whose caller claims the states
    are its own -- the library re-marches (and rebuilds what that forward builds); the gradient equals the switch-off one"""
    from voxe_hip import ops
    grid = _grid(64)
    cfg = make_render_cfg(S, NEAR, FAR, perturb=True, white_bkgd=True, seed=4, rng_offset=6)
    spec, td, tf = gh.spec_of(grid), gh.t(grid.densities), gh.t(grid.features)
    oa, da = _rays(400, 3)
    hw_b = 400 if case == "other_rays_through_the_general_kernel" else 100
    ob, db = _rays(hw_b, 38)
    toa, tda, tob, tdb = gh.t(oa), gh.t(da), gh.t(ob), gh.t(db)
    r = np.random.default_rng(8)
    grads = [gh.t(r.standard_normal((ob.shape[0], 3)).astype(np.float32)), None, None]
    on_b = _params(cfg, hw_b, tile_map=0 if hw_b == 400 else 4, tile_qsplit=1)
    got = {}
    for name in ("stale", "off"):
        ws = ops.Workspace()
        if name == "stale":
            _forward(spec, _params(cfg, 400), td, tf, toa, tda, ws, (4, 6))          # rays A: cost order, list built
            assert _layout(spec, _params(cfg, 400), td, tf, oa.shape[0], (4, 6))[0] == 1
            mid = _params(cfg, hw_b, tile_lean=-1, tile_qsplit=1) if hw_b == 400 else on_b
            outs = _forward(spec, mid, td, tf, tob, tdb, ws, (4, 6))                 # rays B
            params = on_b
            # a careless caller's claim: "the workspace holds the forward of exactly this backward"
            g_, c_ = ops._descs(spec, params, td, tf, 4, 6, False)
            ws.remember_states(ops._state_key(ops._pack_key(spec, td, tf), params, tob, tdb, None, (4, 6), ops._route(g_, c_, ob.shape[0])), tob, tdb, None)
        else:
            params = _params(cfg, hw_b, tile_map=1, tile_qsplit=1)
            outs = _forward(spec, params, td, tf, tob, tdb, ws, (4, 6))
        got[name] = _backward(spec, params, td, tf, tob, tdb, outs, grads, ws, (4, 6))
        assert np.isfinite(got[name][0]).all() and np.isfinite(got[name][1]).all()
    err = (rel_l2(got["stale"][0], got["off"][0]), rel_l2(got["stale"][1], got["off"][1]))
    assert err[0] < ORDER_TOL and err[1] < ORDER_TOL, err
