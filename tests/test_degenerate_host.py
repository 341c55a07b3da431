"""The degenerate-geometry case table (tests/degenerate_cases.py) on the oracle alone: every case still is what its name says --
the counts of samples exactly on voxel planes and on AABB faces, the exact zero direction components, the bit-equal ties between
march axes, and for the launches that miss the grid a background-coloured render with exact-zero gradients.  CPU only; the GPU
comparison of the same table is tests/test_hip_degenerate_rays.py."""
import numpy as np
import pytest

import degenerate_cases as dc

from oracle import voxe_oracle as vo


def test_the_lattice_grid_is_exact_in_float32():
    from voxe_hip.desc import norm_constants

    scale, bias = norm_constants(dc.LATTICE_AABB)
    assert [float(s) for s in scale] == [0.5, 1.0, 0.25] and [float(b) for b in bias] == [0.0, 0.0, 0.0]
    for n, (lo, hi) in zip(dc.LATTICE_DIMS, dc.LATTICE_AABB):
        assert (hi - lo) / n == 0.25
    g = dc.lattice_grid()
    assert g.density_scale == 2.0 and dc.lattice_grid(relu=True).density_scale == 100.0 / 3.0
    assert dc.generic_grid().densities.shape[:3] == (16, 12, 20)


@pytest.mark.parametrize("name", dc.NAMES)
def test_case_preconditions_hold_on_the_oracle(name):
    c = dc.case(name)
    grid, kw, H, W, focal, rot, eye, S, near, far = c
    o, d = dc.rays(c)
    assert o.shape == (c.views * H * W, 3) and c.cfg().num_samples == S
    facts = dc.check_preconditions(c, o, d)
    out = vo.render_fwd(grid, c.cfg(), o, d, dc.jitter_of(c))
    R = o.shape[0]
    rng = np.random.default_rng(1)
    gc = rng.standard_normal((R, 3)).astype(np.float32)
    gdep, gacc = rng.standard_normal(R).astype(np.float32), rng.standard_normal(R).astype(np.float32)
    gd, gf = vo.render_bwd(grid, c.cfg(), o, d, gc, d_depth=gdep, d_acc=gacc, jitter=dc.jitter_of(c))
    if c.need.get("miss"):
        assert np.array_equal(out["acc"], np.zeros(R, np.float32)) and np.isnan(out["disparity"]).all()
        assert np.array_equal(out["colour"], np.full((R, 3), float(bool(kw.get("white_bkgd"))), np.float32))
        assert np.array_equal(gd, np.zeros_like(gd)) and np.array_equal(gf, np.zeros_like(gf))
    else:
        assert facts["inside"] > 0 and float(out["acc"].max()) > 0.4 and np.abs(gd).max() > 0 and np.abs(gf).max() > 0


def test_axis_views_sample_the_entry_and_the_exit_face_exactly():
    """sample 0 of the central ray lies on the entry face, the last sample on the exit face, every second sample on a voxel plane"""
    for name in ("axis+x", "axis-x", "axis+y", "axis-y", "axis+z", "axis-z"):
        c = dc.case(name)
        o, d = dc.rays(c)
        mid = (c.H // 2) * c.W + c.W // 2
        z = vo.sample_probe(c.grid, c.cfg(), o, d)["z"][mid]
        p = o[mid] + d[mid] * z[:, None]
        a = dc._AXES[name[5]]
        lo, hi = dc.LATTICE_AABB[a]
        assert {float(p[0, a]), float(p[-1, a])} == {lo, hi}
        u = dc.index_coords(c.grid, p.astype(np.float32))[:, a]
        assert np.array_equal(u[1::2], np.floor(u[1::2])) and np.array_equal(u[0::2] - np.floor(u[0::2]), np.full(len(u[0::2]), 0.5, np.float32))
