"""The oracle's backward with a per-ray cut (vo.render_bwd(..., cut=...), oracle/voxe_cpu.c) and the case table of the gradient
truncation (tests/term_eps_cases.py) on the oracle alone.  CPU only; the GPU comparison of the same table is
tests/test_hip_term_eps.py."""
import numpy as np
import pytest

import term_eps_cases as tc

from oracle import voxe_oracle as vo


def _small(name="sp_s64_e0.1", rays=slice(600, 1000), deg=0):
    """a few hundred rays of one case with upstream gradients on colour, depth and acc and a caller's jitter tensor (a launch can
    then be split without moving a ray to another place of the in-kernel jitter stream)"""
    c = tc.case(name)
    grid = tc.grid_of(c.field, c.attn, deg)
    o, d = tc.rays(c)
    o, d = np.ascontiguousarray(o[rays]), np.ascontiguousarray(d[rays])
    rng = np.random.default_rng(12)
    R = o.shape[0]
    jit = rng.uniform(0, 1, (R, c.S)).astype(np.float32)
    gc = rng.standard_normal((R, grid.cout)).astype(np.float32)
    gdep, gacc = rng.standard_normal(R).astype(np.float32), rng.standard_normal(R).astype(np.float32)
    return c, grid, c.cfg(deg), o, d, jit, gc, gdep, gacc


def test_a_cut_behind_the_last_sample_is_the_plain_backward_bit_for_bit():
    for name, deg in (("sp_s64_e0.1", 0), ("relu_s97_clip_e0.5", 2), ("attn_relu_s64_e0.1", 0)):
        c, grid, cfg, o, d, jit, gc, gdep, gacc = _small(name, deg=deg)
        plain = vo.render_bwd(grid, cfg, o, d, gc, d_depth=gdep, d_acc=gacc, jitter=jit)
        full = vo.render_bwd(grid, cfg, o, d, gc, d_depth=gdep, d_acc=gacc, jitter=jit, cut=np.full(o.shape[0], c.S, np.int32))
        assert np.abs(plain[0]).max() > 0 and np.abs(plain[1]).max() > 0
        assert np.array_equal(plain[0], full[0]) and np.array_equal(plain[1], full[1])
        # the oracle does not read cfg.term_eps: the caller owns the threshold decision
        eps = vo.render_bwd(grid, c.cfg(deg, term_eps=0.5), o, d, gc, d_depth=gdep, d_acc=gacc, jitter=jit)
        assert np.array_equal(plain[0], eps[0]) and np.array_equal(plain[1], eps[1])


def test_a_cut_at_sample_zero_leaves_exact_zeros():
    c, grid, cfg, o, d, jit, gc, gdep, gacc = _small()
    gd, gf = vo.render_bwd(grid, cfg, o, d, gc, d_depth=gdep, d_acc=gacc, jitter=jit, cut=np.zeros(o.shape[0], np.int32))
    assert not gd.any() and not gf.any()
    gd, _ = vo.render_bwd(grid, cfg, o, d, gc, jitter=jit, cut=np.zeros(o.shape[0], np.int32), want_features=False)
    assert _ is None and not gd.any()


@pytest.mark.parametrize("name", ["sp_s64_e0.1", "relu_s97_clip_e0.5"])
def test_moving_one_ray_s_cut_by_one_touches_the_corners_of_that_sample_only(name):
    """G(cut = K) - G(cut = K - 1) of a single ray is the deposit of sample K - 1: non-zero on the (up to 8, in-bounds) corners of
    its cell only, and exactly zero when that sample is outside the grid -- an off-by-one in the oracle's own cut would move the
    support to the neighbouring sample's cell"""
    c, grid, cfg, o, d, jit, gc, gdep, gacc = _small(name, rays=slice(815, 825))
    dims = np.array(grid.densities.shape[:3])
    probe = vo.sample_probe(grid, cfg, o, d, jit)
    T = tc.transmittance(probe, d)
    seen_inside = seen_outside = 0
    for r in range(o.shape[0]):
        one = slice(r, r + 1)
        args = (grid, cfg, o[one], d[one], gc[one])
        kw = dict(d_depth=gdep[one], d_acc=gacc[one], jitter=jit[one])
        prev = vo.render_bwd(*args, cut=np.array([0], np.int32), **kw)
        for K in range(1, c.S + 1):
            cur = vo.render_bwd(*args, cut=np.array([K], np.int32), **kw)
            k = K - 1
            support = np.zeros(grid.densities.shape[:3], bool)
            if probe["inside"][r, k]:
                for corner in range(8):
                    i = probe["idx"][r, k] + np.array([corner & 1, (corner >> 1) & 1, corner >> 2])
                    if np.all(i >= 0) and np.all(i < dims):
                        support[tuple(i)] = True
            for a, b in zip(cur, prev):
                moved = (a != b).any(-1)
                assert not (moved & ~support).any(), (r, K)
            if k < c.S - 1 and T[r, k] - T[r, k + 1] > 1e-3:      # a sample with weight: it deposits into both tensors
                assert probe["inside"][r, k]
                assert (cur[0] != prev[0]).any() and (cur[1] != prev[1]).any(), (r, K)
                seen_inside += 1
            seen_outside += int(not probe["inside"][r, k])
            prev = cur
    # (a clipped march has every sample between the faces its ray crosses)
    assert seen_inside >= 20 and (c.clip or seen_outside >= 20), (seen_inside, seen_outside)


def test_two_launches_sum_to_one():
    c, grid, cfg, o, d, jit, gc, gdep, gacc = _small("relu_s64_e0.5", rays=slice(400, 1200))
    R = o.shape[0]
    cut = tc.cut_of(tc.transmittance(vo.sample_probe(grid, cfg, o, d, jit), d), c.eps)
    assert 0.25 < (cut < c.S).mean() < 0.98
    whole = vo.render_bwd(grid, cfg, o, d, gc, d_depth=gdep, d_acc=gacc, jitter=jit, cut=cut)
    parts = [vo.render_bwd(grid, cfg, o[s], d[s], gc[s], d_depth=gdep[s], d_acc=gacc[s], jitter=jit[s], cut=cut[s])
             for s in (slice(0, 333), slice(333, R))]
    plain = vo.render_bwd(grid, cfg, o, d, gc, d_depth=gdep, d_acc=gacc, jitter=jit)
    for w, a, b, p in zip(whole, parts[0], parts[1], plain):
        # (each launch rounds its float64 sums to float32 once)
        np.testing.assert_allclose(a.astype(np.float64) + b.astype(np.float64), w, rtol=3e-7, atol=3e-7 * float(np.abs(w).max()))
        assert np.linalg.norm(w - p) > 1e-2 * np.linalg.norm(p)         # the cuts really change this gradient


def test_the_cut_is_where_the_forward_s_transmittance_crosses_the_threshold():
    """T of the table (float64, from the probe) against the forward: 1 - acc = T behind the last sample; and the cut's definition"""
    c, grid, cfg, o, d, jit, *_ = _small()
    probe = vo.sample_probe(grid, cfg, o, d, jit)
    T = tc.transmittance(probe, d)
    acc = vo.render_fwd(grid, cfg, o, d, jit)["acc"]
    last_inside = probe["inside"][:, -1]
    np.testing.assert_allclose((1.0 - acc)[~last_inside], T[~last_inside, -1], rtol=0, atol=2e-6)
    assert np.all(T[:, 0] == 1.0) and np.all(np.diff(T, axis=1) <= 0)
    cut = tc.cut_of(T, 0.1)
    for r in range(T.shape[0]):
        assert np.all(T[r, :cut[r]] >= 0.1) and (cut[r] == c.S or T[r, cut[r]] < 0.1)


@pytest.mark.parametrize("order", ["image", "permuted"])
@pytest.mark.parametrize("name", tc.NAMES)
def test_case_conditions_hold_on_the_oracle(name, order):
    ref = tc.reference(name, order)
    print(tc.describe(ref))
    tc.check_conditions(ref)
    c = ref["case"]
    assert ref["o"].shape == (c.R, 3) and ref["cfg"].num_samples == c.S and ref["cfg"].term_eps == 0.0
    assert (ref["jit"] is not None) == (c.jitter_seed >= 0)
    for g in (ref["gc"], ref["gdep"], ref["gacc"]):          # ambiguous rays carry no upstream gradient, the others do
        assert not g[ref["amb"]].any() and g[~ref["amb"]].any()


@pytest.mark.parametrize("deg", [1, 2, 3])
@pytest.mark.parametrize("name", tc.SH_CASES)
def test_view_dependent_case_conditions_hold_on_the_oracle(name, deg):
    for order in ("image", "permuted"):
        ref = tc.reference(name, order, deg)
        print(tc.describe(ref))
        tc.check_conditions(ref)
        assert ref["grid"].features.shape[-1] == 3 * (deg + 1) ** 2 and ref["gdep"] is None
        assert np.array_equal(ref["grid"].densities, tc.grid_of(ref["case"].field).densities)      # a second feature tensor on the same grid


def test_the_table_covers_what_it_promises():
    cs = [tc.case(n) for n in tc.NAMES]
    assert {c.eps for c in cs} == {0.1, 0.5, 1e-3} and {c.S for c in cs} == {33, 64, 97}
    assert any(c.clip for c in cs) and any(not c.clip for c in cs) and any(c.attn for c in cs) and any(c.views > 1 for c in cs)
    assert {c.seg_len for c in cs} == {16, 32} and {c.field for c in cs} == {"sp", "relu"}
    for names in (tc.ROUTE_CASES, tc.SH_CASES):
        assert sum(tc.case(n).realistic for n in names) == 1 and {tc.case(n).eps for n in names} == {0.1, 0.5, 1e-3}
    two = tc.reference("two_views_s64_e0.5")
    R1 = two["case"].hw ** 2
    a, b = two["cut"][:R1], two["cut"][R1:]
    hist = lambda x: np.bincount(x, minlength=65) / x.size       # noqa: E731
    assert 0.5 * np.abs(hist(a) - hist(b)).sum() > 0.1            # the two cameras' cut distributions differ (total variation)
