"""The specialised planned tile kernels: launches with the headline's launch-uniform configuration -- softplus
post-activation, white background, both gradients wanted, term_eps = 0 -- run render_*_tile4*_plan_sw_kernel, whose sample
loops have those switches resolved at compile time and whose flush addresses the gradient as (base + 32-bit offset) with the
layer origins out of the per-layer table; every other configuration runs the planned kernels that read the switches.

Every case, at the shapes of tests/test_hip_tile_plan.py (a partial last depth segment, partial tiles on both image edges,
VoxeDispatch tile_map = 4, tile_qsplit = 1, tile_kl = 8: a list and a plan are built):
  * the forward equals the ray-ordered forward (fwd_window = -1, tile_lean = -1) bit for bit;
  * the gradients are within 1e-4 rel-L2 of the CPU oracle and within 2e-6 of the general tile kernel (tile_lean = -1): the
    bounds of tests/test_hip_sched.py;
  * the planned kernels ran (launch counts of the library).
Cases: the specialised configuration over grids x images x sample counts x cameras (the "axis" camera looks down z: its
layers go out in z-neighbour pairs; the "oblique" one marches x and y); each single deviation from it through the generic
planned kernels (ReLU, black background, densities frozen, features frozen, term_eps = 1e-3 against the truncated oracle as
in tests/test_hip_term_eps.py); an off-axis z-dominant camera; tiles that split, so that several passes of a block re-build
the table.  (The launcher's 32-bit guard needs a gradient buffer above 4 GiB and is not exercised here.)"""
import functools

import numpy as np
import pytest
import torch

import term_eps_cases as tc
from helpers import rel_l2
from synth import FAR, NEAR, RADIUS, focal_for
from test_hip_tile_plan import (AABB, GRIDS, IMAGES, RNG, _forward, _params, _planned_launches,
                                _restated_decisions)
from voxe_hip import abi
from voxe_hip.desc import make_render_cfg, norm_constants

from oracle import voxe_oracle as vo

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import gpu_helpers as gh
    from thre3d_atom.utils.imaging_utils import pose_spherical

GRAD_TOL = 1e-4      # vs the oracle
ORDER_TOL = 2e-6     # vs the general tile kernel: two summation orders of the same float atomics (tests/test_hip_sched.py)
DELTA = 1e-3         # rays whose cut depends on the last 1e-3 of the threshold carry no upstream gradient (tests/term_eps_cases.py)
CAMERAS = {"axis": (0.0, 0.0, 0.0), "oblique": (40.0, 63.0, 20.0), "zdom": (15.0, 12.0, 0.0)}
# what a case changes of the specialised configuration
DEVIATIONS = {
    "headline": {},
    "relu": dict(post_act="relu"),
    "black": dict(white=False),
    "densities_frozen": dict(want_d=False),
    "features_frozen": dict(want_f=False),
    "term_eps": dict(term_eps=1e-3),
}


def _rays(camera, size):
    yaw, pitch, roll = CAMERAS[camera]
    w, h = size
    pose = pose_spherical(yaw, pitch, RADIUS)
    cr, sr = np.cos(np.radians(roll)), np.sin(np.radians(roll))
    rot = pose.rotation.numpy() @ np.array([[cr, -sr, 0.0], [sr, cr, 0.0], [0.0, 0.0, 1.0]], dtype=np.float32)
    o, d = vo.cast_rays(h, w, focal_for(48), rot, pose.translation.numpy())
    return np.ascontiguousarray(o, dtype=np.float32), np.ascontiguousarray(d, dtype=np.float32)


def _grid(dims, post_act):
    g = torch.Generator().manual_seed(3)
    dens = torch.empty((*dims, 1)).uniform_(-1.0, 1.0, generator=g)
    feat = torch.empty((*dims, 3)).uniform_(-1.0, 1.0, generator=g)
    return vo.Grid(dens.numpy(), feat.numpy(), AABB, 100.0 / 3.0, abi.ACT_IDENTITY, abi.ACT_RELU if post_act == "relu" else abi.ACT_SOFTPLUS)


@functools.lru_cache(maxsize=None)
def _reference(grid_name, image, S, camera, deviation):
    """the case's inputs, the oracle's gradients and what the ray-ordered forward + general tile backward give: computed once"""
    dev = dict(post_act="softplus", white=True, want_d=True, want_f=True, term_eps=0.0)
    dev.update(DEVIATIONS[deviation])
    dims, size = GRIDS[grid_name], IMAGES[image]
    grid = _grid(dims, dev["post_act"])
    o, d = _rays(camera, size)
    R = o.shape[0]
    cfg = make_render_cfg(S, NEAR, FAR, perturb=True, white_bkgd=dev["white"], seed=RNG[0], rng_offset=RNG[1], term_eps=dev["term_eps"])
    r = np.random.default_rng(11)
    gc = r.standard_normal((R, 3)).astype(np.float32)
    gdep = (0.1 * r.standard_normal((R, 1))).astype(np.float32)
    gacc = (0.1 * r.standard_normal((R, 1))).astype(np.float32)
    cut = None
    if dev["term_eps"] > 0.0:
        T = tc.transmittance(vo.sample_probe(grid, cfg, o, d, None), d)
        cut = tc.cut_of(T, dev["term_eps"])
        amb = tc.cut_of(T, dev["term_eps"] * (1 + DELTA)) != tc.cut_of(T, dev["term_eps"] * (1 - DELTA))
        for upstream in (gc, gdep, gacc):
            upstream[amb] = 0.0
        assert 0 < (cut < S).sum() and (cut[~amb] < S).any(), "the truncation must cut some rays"
    rd, rf = vo.render_bwd(grid, cfg, o, d, gc, d_depth=gdep[:, 0], d_acc=gacc[:, 0], want_densities=dev["want_d"],
                           want_features=dev["want_f"], cut=cut)
    ref = dict(dev=dev, dims=dims, size=size, grid=grid, cfg=cfg, o=o, d=d, gc=gc, gdep=gdep, gacc=gacc, oracle=(rd, rf))
    ref["general"] = _run(ref, tile_map=1, tile_lean=-1, fwd_window=-1)
    return ref


def _run(ref, **disp):
    """forward + backward through the library -> ([colour, depth, acc, disparity], (d_densities, d_features)); a frozen tensor: None"""
    from voxe_hip import ops
    grid, dev = ref["grid"], ref["dev"]
    spec, td, tf, to, tdir = gh.spec_of(grid), gh.t(grid.densities), gh.t(grid.features), gh.t(ref["o"]), gh.t(ref["d"])
    params = _params(ref["cfg"], ref["size"][0], 0, **disp)
    params.term_eps = float(dev["term_eps"])
    grads = [gh.t(ref["gc"]), gh.t(ref["gdep"]), gh.t(ref["gacc"])]
    ws = ops.Workspace()
    outs = _forward(spec, params, td, tf, to, tdir, ws)
    d_d = torch.zeros_like(td) if dev["want_d"] else None
    d_f = torch.zeros_like(tf) if dev["want_f"] else None
    ops.render_bwd_into(spec, params, td, tf, to, tdir, None, outs[0], outs[1], outs[2], grads[0], grads[1], grads[2], d_d, d_f, ws, RNG)
    torch.cuda.synchronize()
    return [gh.n(v) for v in outs], (None if d_d is None else gh.n(d_d), None if d_f is None else gh.n(d_f))


def _check(grid_name, image, S, camera, deviation="headline"):
    ref = _reference(grid_name, image, S, camera, deviation)
    before = _planned_launches()
    outs, grads = _run(ref, tile_map=4)
    after = _planned_launches()
    assert (after[0] - before[0], after[1] - before[1]) == (1, 1), "the planned route did not run"
    for a, b in zip(outs[:3], ref["general"][0][:3]):      # colour, depth, acc: every bit of the ray-ordered forward
        assert np.array_equal(a, b, equal_nan=True)
    assert np.array_equal(np.isnan(outs[3]), np.isnan(ref["general"][0][3]))
    for name, got, general, oracle in zip(("densities", "features"), grads, ref["general"][1], ref["oracle"]):
        if got is None:
            assert general is None
            continue
        assert np.isfinite(got).all() and np.abs(oracle).max() > 0.0
        e_or, e_gen = rel_l2(got, oracle), rel_l2(got, general)
        print(f"{grid_name} {image} S {S} {camera} {deviation} {name}: vs oracle {e_or:.3e}  vs general tile kernel {e_gen:.3e}")
        assert e_or < GRAD_TOL, (name, e_or)
        assert e_gen <= ORDER_TOL, (name, e_gen)
    return ref


@pytest.mark.parametrize("camera", ["axis", "oblique"])
@pytest.mark.parametrize("S", [96, 40])
@pytest.mark.parametrize("image", list(IMAGES))
@pytest.mark.parametrize("grid", list(GRIDS))
def test_specialised_kernels_equal_the_ray_ordered_forward_the_general_kernel_and_the_oracle(grid, image, S, camera):
    _check(grid, image, S, camera)


@pytest.mark.parametrize("shape", [("cube24", "48x40", 96, "axis"), ("aniso", "37x29", 40, "oblique")])
@pytest.mark.parametrize("deviation", [k for k in DEVIATIONS if k != "headline"])
def test_each_single_deviation_runs_the_generic_planned_kernels_with_the_same_agreement(deviation, shape):
    _check(*shape, deviation)


@pytest.mark.parametrize("grid,image,S", [("cube24", "48x40", 96), ("aniso", "37x29", 40)])
def test_a_z_dominant_view_flushes_its_layer_pairs_with_the_tabulated_offsets(grid, image, S):
    """every ray of this camera advances fastest along z (and none along an axis): the tiles march z, consecutive layers are
    z-neighbours and go out as pairs under one base with both layers' table offsets in the lane offsets"""
    ref = _check(grid, image, S, "zdom")
    step = np.abs(ref["d"] * (np.asarray(GRIDS[grid], np.float32) / 3.0)[None, :])      # voxels per unit depth (AABB side 3)
    assert (step.argmax(1) == 2).all() and (step.min(1) > 0.05 * step.max(1)).mean() > 0.5


def test_tiles_that_split_rebuild_the_table_in_every_pass():
    """the "axis" camera at 48x40, S = 96: whole tiles in the front segments, quadrants in the last one (restatement of the split
    decision, tests/test_hip_tile_plan.py) -- a block of four passes builds the table four times"""
    dims, size, S = GRIDS["cube24"], IMAGES["48x40"], 96
    ref = _check("cube24", "48x40", S, "axis")
    scale = norm_constants(AABB)[0]
    want = _restated_decisions(ref["d"], dims, scale, size[0], size[1], 1, S)
    splits = {v[1] for v in want.values()}
    assert 0 in splits and 3 in splits, splits
