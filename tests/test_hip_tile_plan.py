"""Per-tile plan of the lean SH-0 tile kernels: the schedule pass takes the decisions of the render kernels'
prologues once per (tile slot, depth segment) -- which rays, lanes along the rows or down the columns, how the tile splits,
the forward's route -- and the planned instantiations read them from an 8-byte record instead of deriving them again.

What is checked, at the smallest shapes at which every branch of that is taken (partial tiles on both image edges, a partial
last segment, tiles that split, tiles that turn their lanes, empty tiles and empty segments, two images in one launch):
  * the records against the block list next to them and against a float32 restatement of the orientation and split decisions
    (tile_lanes_down_columns / tile_split_decision of voxe_render_tile4.hip);
  * VoxeDispatch::tile_map = 4 (list and plan) against tile_map = 1 (static map: no list, no plan, the unplanned kernels):
    forward outputs bit for bit, gradients rel-L2 <= 2e-6 (two summation orders of the same float atomics: the bound of
    tests/test_hip_sched.py for order on / off);
  * both against the CPU oracle with the bounds of the small-image tests (tests/test_hip_configs.py: colour / acc 1e-5
    absolute, depth 1e-5 relative + 1e-5, gradients rel-L2 < 1e-4);
  * the planned kernels really ran where a plan was built (launch counts of the library), and a workspace without room for the
    plan runs the unplanned kernels with the list alone;
  * a backward never reads the plan of another render into the same workspace: after the re-march the records are those of its
    own rays.

Which tiles split and which turn (restatement, asserted below): see CASES."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import rel_l2
from synth import FAR, NEAR, RADIUS, focal_for
from voxe_hip import abi
from voxe_hip.desc import make_render_cfg

from oracle import voxe_oracle as vo

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import gpu_helpers as gh
    from thre3d_atom.utils.imaging_utils import pose_spherical

AABB = [(-1.5, 1.5)] * 3
GRAD_TOL = 1e-4      # vs the oracle (tests/test_hip_configs.py)
FWD_ATOL = 1e-5
ORDER_TOL = 2e-6     # two summation orders of the same float atomics (tests/test_hip_sched.py)
EMPTY = 0x80000000
SEG_LEN = 16         # launches of <= 20 000 rays
RNG = (42, 7)

# name -> (grid dims, (width, height), S, [(yaw, pitch, sideways shift of the ray origins, roll)], what the restatement must find)
# A pinhole camera's un-normalised ray directions differ by the same vector from pixel to pixel, so all tiles of one camera lie
# the same way; how a tile splits depends on its own direction and on the depth of the segment.
#   axis:    camera on the x axis, looking down it: lanes along the rows; whole tiles, quadrants in the last segment
#   oblique: 37x29 px on the anisotropic grid, from above at 63 degrees, rolled by 20: every tile turns its lanes down the columns;
#            whole in segment 0, halves behind it (some tiles from segment 1, the others from segment 2)
#   past:    that camera moved sideways until part of the image looks past the volume: empty tiles, empty segments of live tiles
#   two:     two cameras in one launch (image_height = 40 of 80 rows): the tiles of the first along the rows, of the second down
#            the columns; whole tiles, halves of either kind and quadrants
CASES = {
    "axis": ((24, 24, 24), (48, 40), 96, [(0.0, 0.0, 0.0, 0.0)], dict(turn="none", split=True)),
    "oblique": ((20, 24, 28), (37, 29), 40, [(40.0, 63.0, 0.0, 20.0)], dict(turn="all", split=True)),
    "past": ((24, 24, 24), (37, 29), 96, [(40.0, 63.0, 2.0, 20.0)], dict(turn="all", split=True, empty=True)),
    "two": ((24, 24, 24), (48, 40), 96, [(0.0, 0.0, 0.0, 0.0), (130.0, 50.0, 0.0, 0.0)], dict(turn="mixed", split=True)),
}


def _rays(case):
    _, (w, h), _, cams, _ = CASES[case]
    os_, ds_ = [], []
    for yaw, pitch, shift, roll in cams:
        pose = pose_spherical(yaw, pitch, RADIUS)
        cr, sr = np.cos(np.radians(roll)), np.sin(np.radians(roll))
        rot = pose.rotation.numpy() @ np.array([[cr, -sr, 0.0], [sr, cr, 0.0], [0.0, 0.0, 1.0]], dtype=np.float32)   # rolled about the view axis
        # (the focal length of the wider image: the 37 px images see the volume with rays further apart)
        o, d = vo.cast_rays(h, w, focal_for(48), rot, pose.translation.numpy())
        o = o + shift * rot[:, 0][None, :].astype(o.dtype)     # along the camera's x axis
        os_.append(o); ds_.append(d)
    return (np.ascontiguousarray(np.concatenate(os_), dtype=np.float32), np.ascontiguousarray(np.concatenate(ds_), dtype=np.float32))


def _grid(dims, seed=3):
    g = torch.Generator().manual_seed(seed)
    dens = torch.empty((*dims, 1)).uniform_(-1.0, 1.0, generator=g)
    feat = torch.empty((*dims, 3)).uniform_(-1.0, 1.0, generator=g)
    return vo.Grid(dens.numpy(), feat.numpy(), AABB, 100.0 / 3.0, abi.ACT_IDENTITY, abi.ACT_SOFTPLUS)


def _params(cfg, width, height, **disp):
    from voxe_hip.dispatch import Dispatch
    base = dict(tile_min_rays=-1, tile_qsplit=1, tile_kl=8)      # the LDS-window backward, one block per (tile, segment), 8-wide
    base.update(disp)
    return gh.params_of(cfg, image_width=width, image_height=height, dispatch=Dispatch(**base))


def _offsets(spec, params, td, tf, R):
    """(applies, byte offset of the list, blocks, tile slots), grid descriptor"""
    from voxe_hip import ops
    from voxe_hip.runtime import lib
    g, c = ops._descs(spec, params, td, tf, RNG[0], RNG[1], False)
    fn = lib().voxe_tile_sched_debug_layout
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    out = (C.c_int64 * 4)()
    assert fn(C.byref(g), C.byref(c), R, out) == 0
    return [int(v) for v in out], g


def _plan_records(spec, params, td, tf, R, ws, nb):
    """the plan the last forward into `ws` wrote: uint32 [blocks, 2] in list order, or None when launches of this configuration
    build none or the workspace has no room for it (it lives behind everything voxe_workspace_bytes asks for)"""
    from voxe_hip import ops
    from voxe_hip.runtime import lib
    g, c = ops._descs(spec, params, td, tf, RNG[0], RNG[1], False)
    fp = lib().voxe_tile_plan_debug_offset
    fp.restype = C.c_int
    fp.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    off = C.c_int64(0)
    assert fp(C.byref(g), C.byref(c), R, C.byref(off)) == 0
    if off.value < 0 or ws.buf.numel() < off.value + 16 * nb:
        return None
    return ws.buf[off.value:off.value + 8 * nb].cpu().numpy().view(np.uint32).reshape(nb, 2).copy()


def _planned_launches():
    """(forward, backward) launches of the planned kernels by this process so far: a launch that fell back to the unplanned
    kernels would give the same results, only the count tells"""
    from voxe_hip.runtime import lib
    fn = lib().voxe_tile_plan_debug_launches
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(C.c_int64)]
    out = (C.c_int64 * 2)()
    assert fn(out) == 0
    return int(out[0]), int(out[1])


def _forward(spec, params, td, tf, to, tdir, ws):
    from voxe_hip import ops
    outs = [torch.empty((to.shape[0], n), device="cuda") for n in (3, 1, 1, 1)]
    ops.render_fwd_into(spec, params, td, tf, to, tdir, None, *outs, ws, RNG)
    torch.cuda.synchronize()
    return outs


def _backward(spec, params, td, tf, to, tdir, outs, grads, ws):
    from voxe_hip import ops
    d_d, d_f = torch.zeros_like(td), torch.zeros_like(tf)
    ops.render_bwd_into(spec, params, td, tf, to, tdir, None, outs[0], outs[1], outs[2], grads[0], grads[1], grads[2], d_d, d_f, ws, RNG)
    torch.cuda.synchronize()
    return gh.n(d_d), gh.n(d_f)


def _zlin(k, S):
    """DepthGen::zlin (voxe_device.hpp) in float32; the fmaf of tval() through float64 (exact product and sum, one rounding)"""
    f = np.float32
    step = f(1.0) / f(S - 1)
    t = step * f(k) if k < S // 2 else f(np.float64(-step) * np.float64(S - 1 - k) + 1.0)
    return f(NEAR) * (f(1.0) - t) + f(FAR) * t


def _restated_decisions(d, dims, scale, width, height, nimg, S):
    """-> {(tile, segment): (lanes down the columns, split code)} for the tiles whose pixels (0, 0), (1, 0), (0, 1) are inside
    the image: tile_lanes_down_columns and tile_split_decision<8> (fit_lat 5.5, fit_m 4.5: launches of <= 16 000 tile-segments)
    in float32, operation for operation"""
    f = np.float32
    ntx, per = (width + 7) // 8, (height + 7) // 8
    nseg = (S + SEG_LEN - 1) // SEG_LEN
    N = [f(v) for v in dims]
    sc = [f(v) for v in scale]
    out = {}
    for tile in range(ntx * per * nimg):
        ty, tx = divmod(tile, ntx)
        img, tyi = divmod(ty, per)
        if width - 8 * tx < 2 or height - 8 * tyi < 2:
            continue
        ray = lambda i, j: d[(img * height + 8 * tyi + i) * width + 8 * tx + j]     # noqa: E731
        d0, dx, dy = ray(0, 0), ray(0, 1), ray(1, 0)
        ex = [(dx[a] - d0[a]) * (sc[a] * N[a]) for a in range(3)]
        ey = [(dy[a] - d0[a]) * (sc[a] * N[a]) for a in range(3)]
        lat_x, lat_y = ex[0] * ex[0] + ex[1] * ex[1], ey[0] * ey[0] + ey[1] * ey[1]
        columns = bool((ey[2] * ey[2]) * lat_x > (ex[2] * ex[2]) * lat_y)
        d1, d8 = (dy, dx) if columns else (dx, dy)        # the rays of lanes 1 and 8 in the tile's final orientation
        for seg in range(nseg):
            zref = _zlin(min(S, (seg + 1) * SEG_LEN) - 1, S)
            s = [sc[a] * f(0.5) * N[a] for a in range(3)]
            a0 = [abs(d0[a] * s[a]) for a in range(3)]
            ex3 = [abs((d1[a] - d0[a]) * s[a] * zref) for a in range(3)]
            ey3 = [abs((d8[a] - d0[a]) * s[a] * zref) for a in range(3)]
            m = 0 if (a0[0] >= a0[1] and a0[0] >= a0[2]) else (1 if a0[1] >= a0[2] else 2)

            def fits(wx, wy):
                e = [f(wx) * ex3[a] + f(wy) * ey3[a] for a in range(3)]
                lat = max([f(0.0)] + [e[a] for a in range(3) if a != m])
                return lat <= f(5.5) and e[m] <= f(4.5)
            split = 0
            if not fits(7, 7):
                hx, hy = fits(3, 7), fits(7, 3)
                sx, sy = ex3[0] + ex3[1] + ex3[2], ey3[0] + ey3[1] + ey3[2]
                split = (1 if sx >= sy else 2) if (hx and hy) else (1 if hx else (2 if hy else 3))
            out[(tile, seg)] = (columns, split)
    return out


def _check_plan(ws, layout, rec, g, o, d, dims, width, height, nimg, S, expect):
    applies, list_off, nb, ntp = layout
    assert applies == 1 and rec is not None
    buf = ws.buf[list_off:list_off + 5 * nb].cpu().numpy()
    order, cost = buf[:4 * nb].view(np.uint32).copy(), buf[4 * nb:].copy()
    x, y = rec[:, 0], rec[:, 1]
    b = order & np.uint32(EMPTY - 1)
    seg, rb = b // ntp, b % ntp
    # the record of list position p belongs to the block the list names there: same segment, same cost, same empty mark
    assert np.array_equal((x >> 24) & 63, seg)
    assert np.array_equal((x >> 18) & 63, cost[b])
    assert np.array_equal(x >> 31, order >> 31) and np.array_equal(x >> 31, (cost[b] == 0).astype(np.uint32))
    # ... and names the rays of that tile slot: ray of pixel (0, 0), columns and rows inside the image (0 / 0: launch padding)
    ntx, per = (width + 7) // 8, (height + 7) // 8
    ntiles = ntx * per * nimg
    real = rb < ntiles
    ty, tx = rb // ntx, rb % ntx
    img, tyi = ty // per, ty % per
    assert np.array_equal((y & 0xffffff)[real], (((img * height + 8 * tyi) * width + 8 * tx))[real].astype(np.uint32))
    assert np.array_equal(((y >> 24) & 15)[real], np.minimum(8, width - 8 * tx)[real].astype(np.uint32))
    assert np.array_equal((y >> 28)[real], np.minimum(8, height - 8 * tyi)[real].astype(np.uint32))
    assert not y[~real].any()
    # first sample of the span inside its segment; forward route -1 .. 2, its reference lane below 64 by construction
    nonempty = cost[b] > 0
    assert (((x >> 13) & 31)[nonempty] + cost[b][nonempty] <= SEG_LEN).all()
    # orientation and split code against the restatement
    want = _restated_decisions(d, dims, [g.norm_scale[a] for a in range(3)], width, height, nimg, S)
    turned, splits = set(), {}
    for p in range(nb):
        key = (int(rb[p]), int(seg[p]))
        if key not in want:
            assert ((x[p] >> 1) & 1) == 0 and ((x[p] >> 2) & 3) == 0, key      # (a tile without the three pixels: rows, whole)
            continue
        got = (bool((x[p] >> 1) & 1), int((x[p] >> 2) & 3))
        assert got == want[key], (key, got, want[key])
        if got[0]:
            turned.add(key[0])
        if got[1]:
            splits.setdefault(got[1], set()).add(key[0])
        # the forward turns the lanes of the same tiles, but only where it gathers from global memory (route -1)
        assert ((x[p] >> 6) & 1) == (1 if (got[0] and ((x[p] >> 4) & 3) == 0) else 0), key
    print("tiles that turn their lanes:", sorted(turned), "| tiles that split, by code:", {k: sorted(v) for k, v in splits.items()})
    tiles_seen = {k[0] for k in want}
    assert {"none": not turned, "all": turned == tiles_seen, "mixed": bool(turned) and turned != tiles_seen}[expect["turn"]]
    split_blocks = sum(1 for v in want.values() if v[1])
    if "split" in expect:
        assert (0 < split_blocks < len(want)) == expect["split"]        # some (tile, segment) split, some run whole
    if expect.get("empty"):
        tile_cost = np.zeros((ntp,), np.int64)
        np.add.at(tile_cost, rb, cost[b].astype(np.int64))
        assert (tile_cost[:ntiles] == 0).any() and (tile_cost[:ntiles] > 0).any()          # empty tiles next to live ones
        assert ((cost[b] == 0) & (tile_cost[rb] > 0)).any()                                # empty segments of live tiles


# every grid x image x sample count x camera of the shapes above; what the restatement must find is stated for the four named
# cases (CASES), for the others only how the camera's tiles lie
GRIDS = {"cube24": (24, 24, 24), "aniso": (20, 24, 28)}
IMAGES = {"48x40": (48, 40), "37x29": (37, 29)}
SAMPLES = (96, 40)
CAMERAS = {name: (CASES[name][3], CASES[name][4]["turn"]) for name in CASES}
NAMED = {(CASES[n][0], CASES[n][1], CASES[n][2], n): CASES[n][4] for n in CASES}
MATRIX = [(gn, im, S, cam) for gn in GRIDS for im in IMAGES for S in SAMPLES for cam in CAMERAS]


def _run_case(dims, size, S, cams, expect, plan_room=True, monkeypatch=None):
    from voxe_hip import ops
    width, height = size
    nimg = len(cams)
    grid = _grid(dims)
    CASES["_"] = (dims, size, S, cams, expect)
    o, d = _rays("_")
    R = o.shape[0]
    cfg = make_render_cfg(S, NEAR, FAR, perturb=True, white_bkgd=True, seed=RNG[0], rng_offset=RNG[1])
    spec, td, tf, to, tdir = gh.spec_of(grid), gh.t(grid.densities), gh.t(grid.features), gh.t(o), gh.t(d)
    r = np.random.default_rng(11)
    gc = r.standard_normal((R, 3)).astype(np.float32)
    gdep = (0.1 * r.standard_normal((R, 1))).astype(np.float32)
    gacc = (0.1 * r.standard_normal((R, 1))).astype(np.float32)
    grads = [gh.t(gc), gh.t(gdep), gh.t(gacc)]
    if not plan_room:      # a caller that sizes its workspace with voxe_workspace_bytes alone: list, no plan, the unplanned kernels
        monkeypatch.setattr(ops, "_render_ws_bytes", lambda L, g, c, n: L.voxe_workspace_bytes(C.byref(g), C.byref(c), n))
    got = {}
    for name, tile_map in (("plan", 4), ("static", 1)):
        params = _params(cfg, width, height if nimg > 1 else 0, tile_map=tile_map)
        layout, g = _offsets(spec, params, td, tf, R)
        assert layout[0] == (1 if name == "plan" else 0)
        ws = ops.Workspace()
        before = _planned_launches()
        outs = _forward(spec, params, td, tf, to, tdir, ws)
        rec = _plan_records(spec, params, td, tf, R, ws, layout[2])
        if name == "plan" and plan_room:
            _check_plan(ws, layout, rec, g, o, d, dims, width, height, nimg, S, expect)
        else:
            assert rec is None          # no room for a plan / the static maps build no list and no plan
        got[name] = [gh.n(v) for v in outs] + list(_backward(spec, params, td, tf, to, tdir, outs, grads, ws))
        after = _planned_launches()
        # the planned kernels ran, forward and backward, exactly where a plan was built -- and nowhere else
        assert (after[0] - before[0], after[1] - before[1]) == ((1, 1) if (name == "plan" and plan_room) else (0, 0)), (name, before, after)
        if name == "plan" and not plan_room:      # ... but the list was built and is the restatement's (tests/test_hip_sched.py)
            order = ws.buf[layout[1]:layout[1] + 4 * layout[2]].cpu().numpy().view(np.uint32)
            assert np.array_equal(np.sort(order & np.uint32(EMPTY - 1)), np.arange(layout[2], dtype=np.uint32))
    for a, b in zip(got["plan"][:4], got["static"][:4]):
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a, b, equal_nan=True)
        assert torch.equal(torch.from_numpy(a).nan_to_num(7.0), torch.from_numpy(b).nan_to_num(7.0))
    err = (rel_l2(got["plan"][4], got["static"][4]), rel_l2(got["plan"][5], got["static"][5]))
    print("plan vs static", err)
    assert err[0] <= ORDER_TOL and err[1] <= ORDER_TOL, err
    ref = vo.render_fwd(grid, cfg, o, d)
    rd, rf = vo.render_bwd(grid, cfg, o, d, gc, d_depth=gdep[:, 0], d_acc=gacc[:, 0])
    for name in ("plan", "static"):
        colour, depth, acc = got[name][0], got[name][1][:, 0], got[name][2][:, 0]
        np.testing.assert_allclose(colour, ref["colour"], rtol=0, atol=FWD_ATOL)
        np.testing.assert_allclose(acc, ref["acc"], rtol=0, atol=FWD_ATOL)
        np.testing.assert_allclose(depth, ref["depth"], rtol=1e-5, atol=FWD_ATOL)
        e = (rel_l2(got[name][4], rd), rel_l2(got[name][5], rf))
        print(name, "vs oracle", e)
        assert e[0] < GRAD_TOL and e[1] < GRAD_TOL, (name, e)


@pytest.mark.parametrize("grid,image,S,camera", MATRIX)
def test_planned_kernels_equal_the_unplanned_ones_and_the_oracle(grid, image, S, camera):
    cams, turn = CAMERAS[camera]
    expect = NAMED.get((GRIDS[grid], IMAGES[image], S, camera), dict(turn=turn))
    _run_case(GRIDS[grid], IMAGES[image], S, cams, expect)


def test_a_workspace_without_room_for_the_plan_runs_the_unplanned_kernels(monkeypatch):
    """the plan is an optional tier of the workspace, behind what voxe_workspace_bytes asks for: a caller that does not add
    voxe_tile_plan_bytes gets the block list and the unplanned kernels -- no planned launch, same forward bits, same gradients"""
    dims, size, S, cams, expect = CASES["two"]
    _run_case(dims, size, S, cams, expect, plan_room=False, monkeypatch=monkeypatch)


def test_a_plan_never_outlives_its_forward():
    """the plan is valid exactly as long as the list and the depth-segment states next to it (tests/test_hip_sched.py, same
    scenario): a forward of rays A with a plan, then a forward of other rays B through the general kernels
    (VoxeDispatch::tile_lean = -1) in the same workspace, then a backward of B whose caller claims the states are its own --
    the library re-marches and rebuilds what that forward builds; the gradient equals the one without list and plan"""
    from voxe_hip import ops
    dims, (width, height), S, _, _ = CASES["oblique"]
    grid = _grid(dims)
    cfg = make_render_cfg(S, NEAR, FAR, perturb=True, white_bkgd=True, seed=RNG[0], rng_offset=RNG[1])
    spec, td, tf = gh.spec_of(grid), gh.t(grid.densities), gh.t(grid.features)
    (oa, da), (ob, db) = _rays("oblique"), _rays("past")
    toa, tda, tob, tdb = gh.t(oa), gh.t(da), gh.t(ob), gh.t(db)
    r = np.random.default_rng(8)
    grads = [gh.t(r.standard_normal((ob.shape[0], 3)).astype(np.float32)), None, None]
    on = _params(cfg, width, 0, tile_map=4)
    got = {}
    for name in ("stale", "off"):
        ws = ops.Workspace()
        if name == "stale":
            _forward(spec, on, td, tf, toa, tda, ws)                                         # rays A: list and plan built
            assert _offsets(spec, on, td, tf, oa.shape[0])[0][0] == 1
            outs = _forward(spec, _params(cfg, width, 0, tile_map=4, tile_lean=-1), td, tf, tob, tdb, ws)   # rays B
            params = on
            # a careless caller's claim: "the workspace holds the forward of exactly this backward"
            g_, c_ = ops._descs(spec, params, td, tf, RNG[0], RNG[1], False)
            ws.remember_states(ops._state_key(ops._pack_key(spec, td, tf), params, tob, tdb, None, RNG, ops._route(g_, c_, ob.shape[0])), tob, tdb, None)
        else:
            params = _params(cfg, width, 0, tile_map=1)
            outs = _forward(spec, params, td, tf, tob, tdb, ws)
        if name == "stale":
            nb = _offsets(spec, on, td, tf, ob.shape[0])[0][2]
            plan_a = _plan_records(spec, on, td, tf, ob.shape[0], ws, nb)       # still the plan of rays A: forward B built none
        got[name] = _backward(spec, params, td, tf, tob, tdb, outs, grads, ws)
        assert np.isfinite(got[name][0]).all() and np.isfinite(got[name][1]).all()
        if name == "stale":
            plan_after = _plan_records(spec, on, td, tf, ob.shape[0], ws, nb)   # what the backward's re-march left, and read
    err = (rel_l2(got["stale"][0], got["off"][0]), rel_l2(got["stale"][1], got["off"][1]))
    assert err[0] <= ORDER_TOL and err[1] <= ORDER_TOL, err
    # the plan in the workspace IS that of rays B now: equal to the one a fresh forward of B writes, and not the one of rays A
    fresh = ops.Workspace()
    _forward(spec, on, td, tf, tob, tdb, fresh)
    plan_b = _plan_records(spec, on, td, tf, ob.shape[0], fresh, nb)
    assert plan_a is not None and plan_b is not None and not np.array_equal(plan_a, plan_b)
    assert np.array_equal(plan_after, plan_b)
