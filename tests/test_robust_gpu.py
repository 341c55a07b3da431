"""GPU checks of the robust photometric loss on pixel patches (voxe_robust_fwd_bwd, ops.robust_loss / robust_mask, the trainer's
robust_loss option) against the numpy restatement tests/robust_ref.py.

Bounds.  mask_out, tau_out, stats and d_x are compared bit for bit: the header states every operation behind them.  loss_out and
mse_out are double sums of terms that are exact in double (|d| and d * d of float32 d), in a fixed order, times 1 / (C M) (the
reciprocal and the product: 2 roundings), then rounded to float once.  Any order of n = C M non-negative terms is within
(n - 1) 2^-53 of the exact sum, relatively, and so is the restatement's; the float rounding adds 2^-24.  The bound used is
ref * (2^-24 + (n + 8) 2^-53): nothing is tuned.

No test compares a training run with the option against one without it.  On the synthetic capture that was tried for it (the
schedule and sphere model of test_exposure_gpu's trainer test, 2 x 150 iterations of 4 096 rays; 12 views, 4 of them with an
opaque 12 x 12 square of a saturated colour; 4 clean views held out) the ordering of the held-out figures did not hold on an
MI355X: cc_psnr 18.45 dB without / 18.01 dB with robust_loss (cc_ssim 0.596 / 0.527, raw psnr 7.97 / 7.87 dB), the unmasked
training PSNR of the last batch 21.96 / 25.34 dB, final inlier fractions 0.500 / 0.535 / 0.568.  The scene was not tuned until
it did; DESIGN.md 4.22 records the figures."""
import numpy as np
import pytest
import torch

import robust_ref as RR
from voxe_hip import abi, ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _t(a):
    return None if a is None else torch.as_tensor(a).to(DEV)


def _call(x, y, rank=0, smooth_min=5, patch_min=1, kind="l1", mask_in=None, grad_scale=1.0):
    """every output as numpy: loss, mse, tau (float32 scalars as numpy), mask, stats, d_x"""
    xt, yt = _t(x), _t(y)
    d_x = torch.full_like(xt, float("nan"))
    loss, mse, tau, mask, stats = ops.robust_fwd_bwd(xt, yt, rank, smooth_min, patch_min, kind, _t(mask_in), grad_scale=grad_scale,
                                                     d_x=d_x)
    return {"loss": loss.cpu().numpy(), "mse": mse.cpu().numpy(), "tau": tau.cpu().numpy(), "mask": mask.cpu().numpy(),
            "stats": tuple(int(v) for v in stats.cpu()), "d_x": d_x.cpu().numpy()}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _scalar_ratio(got, ref, n):
    """|got - ref| / bound for a double sum of n terms rounded to float once (module docstring)"""
    bound = abs(ref) * (2.0 ** -24 + (n + 8) * 2.0 ** -53)
    err = abs(float(got) - ref)
    return 0.0 if err == 0.0 else (err / bound if bound > 0 else float("inf"))


def _same_as_reference(tag, got, ref, n, scalars=True):
    """mask, tau, stats and d_x bit for bit; loss and mse inside the bound; returns the worst ratio to the bound"""
    assert set(np.unique(got["mask"])) <= {0, 1}, tag
    assert np.array_equal(got["mask"], ref["mask"]), (tag, int((got["mask"] != ref["mask"]).sum()))
    assert _bits(got["tau"]) == _bits(ref["tau"]), (tag, got["tau"], ref["tau"])
    assert got["stats"] == ref["stats"], (tag, got["stats"], ref["stats"])
    assert np.array_equal(_bits(got["d_x"]), _bits(ref["d_x"])), (tag, int((_bits(got["d_x"]) != _bits(ref["d_x"])).sum()))
    if not scalars:
        return 0.0
    ratios = (_scalar_ratio(got["loss"], ref["loss"], n), _scalar_ratio(got["mse"], ref["mse"], n))
    assert max(ratios) <= 1.0, (tag, ratios, got["loss"], ref["loss"], got["mse"], ref["mse"])
    return max(ratios)


def _check(tag, x, y, rank, smooth_min=5, patch_min=1, kinds=RR.KINDS, grad_scale=0.7, scalars=True):
    worst = 0.0
    for kind in kinds:
        ref = RR.fwd_bwd(x, y, rank, smooth_min, patch_min, kind, grad_scale=grad_scale)
        got = _call(x, y, rank, smooth_min, patch_min, kind, grad_scale=grad_scale)
        worst = max(worst, _same_as_reference(f"{tag} {kind}", got, ref, x.size, scalars))
    return worst


# ---- 1: every shape against the restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,P,C", RR.SHAPES + (RR.MANY_PATCHES,))
def test_outputs_agree_with_the_restatement(N, P, C):
    x, y = RR.inputs(N, P, C)
    M = N * P * P
    worst = 0.0
    for q, smooth_min, f in ((0.5, 5, 0.6), (0.8, 4, 0.9), (0.3, 6, None)):
        rank, patch_min = RR.rank_of_quantile(q, M), RR.patch_min_of_fraction(f, P)
        worst = max(worst, _check(f"{(N, P, C)} q {q}", x, y, rank, smooth_min, patch_min))
    # (the inputs make every rule fire at the trainer's size: raw inliers, forgiven pixels and the patch rule all differ)
    if (N, P, C) == (128, 16, 3):
        s = RR.fwd_bwd(x, y, RR.rank_of_quantile(0.5, M), 5, RR.patch_min_of_fraction(0.6, P))["stats"]
        assert s[0] < s[1] < s[2] < M, s
    print(f"{(N, P, C)}: worst error / bound of loss and mse {worst:.3f}")


# ---- 2: inputs that aim at the select --------------------------------------------------------------------------------------------
def _from_residual_roots(values, N, P):
    """x [N,P,P,1], y = 0: e = x * x"""
    x = np.asarray(values, np.float32).reshape(N, P, P, 1)
    return x, np.zeros_like(x)


def test_select_when_all_residuals_share_their_top_22_bits():
    # x = 1 + k 2^-23, k < 256: x * x rounds to 1 + k 2^-22, inside [1, 1 + 2^-14], all with the same top 22 bits
    N, P = 9, 16
    rng = np.random.default_rng(0)
    k = rng.integers(0, 256, N * P * P)
    x, y = _from_residual_roots(1.0 + k * 2.0 ** -23, N, P)
    e = RR.residuals(x, y)
    assert e.min() >= 1.0 and e.max() <= 1.0 + 2.0 ** -14 and len(np.unique(_bits(e) >> 10)) == 1 and len(np.unique(e)) > 200
    for rank in (0, 1, 1151, 1152, N * P * P - 2, N * P * P - 1):
        _check(f"top bits shared, rank {rank}", x, y, rank, 5, RR.patch_min_of_fraction(0.6, P))


def test_select_with_long_runs_of_equal_values_across_the_rank():
    N, P = 6, 16
    M = N * P * P
    rng = np.random.default_rng(1)
    values = np.repeat(np.array([0.125, 0.25, 0.5], np.float32), M // 3)
    rng.shuffle(values)
    x, y = _from_residual_roots(values, N, P)
    # ranks at both ends of the middle run, inside it, and one to each side of it
    for rank in (M // 3 - 1, M // 3, M // 2, 2 * M // 3 - 1, 2 * M // 3):
        got = _call(x, y, rank, 5, RR.patch_min_of_fraction(0.6, P))
        want = 0.125 ** 2 if rank < M // 3 else (0.25 ** 2 if rank < 2 * M // 3 else 0.5 ** 2)
        assert float(got["tau"]) == want and got["stats"][0] == (M // 3 if rank < M // 3 else 2 * M // 3 if rank < 2 * M // 3 else M)
        _check(f"runs, rank {rank}", x, y, rank, 5, RR.patch_min_of_fraction(0.6, P))


@pytest.mark.parametrize("kind", RR.KINDS)
def test_identical_images_have_threshold_zero_and_no_gradient(kind):
    x, _ = RR.inputs(3, 16, 3)
    M = 3 * 16 * 16
    for rank in (0, M // 2, M - 1):
        got = _call(x, x.copy(), rank, 5, 200, kind)
        assert float(got["tau"]) == 0.0 and got["stats"] == (M, M, M) and got["mask"].all()
        assert float(got["loss"]) == 0.0 and float(got["mse"]) == 0.0 and not got["d_x"].any()
        _same_as_reference("x == y", got, RR.fwd_bwd(x, x.copy(), rank, 5, 200, kind), x.size)


def test_rank_zero_and_rank_last():
    for N, P, C in ((1, 4, 1), (5, 6, 3)):
        x, y = RR.inputs(N, P, C)
        e = RR.residuals(x, y)
        for rank, want in ((0, e.min()), (N * P * P - 1, e.max())):
            got = _call(x, y, rank, 9, P * P + 1)
            assert _bits(got["tau"]) == _bits(want)
            _check(f"{(N, P, C)} rank {rank}", x, y, rank, 9, P * P + 1)


def test_infinite_residuals_sit_above_the_rank():
    N, P, C = 3, 16, 3
    x, y = RR.inputs(N, P, C)
    x[1, 2:9, 3:11, 0] = 1e30          # d is finite, e = d * d overflows to +inf
    e = RR.residuals(x, y)
    assert np.isinf(e).sum() == 56 and np.isfinite(x).all()
    rank = RR.rank_of_quantile(0.5, N * P * P)
    got = _call(x, y, rank, 5, P * P + 1)
    assert np.isfinite(got["tau"]) and not got["mask"][1, 3:8, 4:10].any()      # (the pixels with no finite neighbour)
    # (mse overflows a float: the scalars are not compared here)
    _check("inf", x, y, rank, 5, RR.patch_min_of_fraction(0.6, P), scalars=False)
    # ... and at the last rank tau is +inf and everything is an inlier
    got = _call(x, y, N * P * P - 1, 5, 1)
    assert np.isposinf(got["tau"]) and got["mask"].all()


# ---- 3: inputs that aim at the neighbourhoods (C = 1, y = 0, two residual levels) -------------------------------------------------
IN, OUT = 0.25, 0.75


def _from_inliers(a):
    """x, y, rank such that the raw inlier mask is exactly `a` [N,P,P] of 0 / 1 (at least one inlier)"""
    a = np.asarray(a)
    x, y = _from_residual_roots(np.where(a != 0, IN, OUT), a.shape[0], a.shape[1])
    return x, y, int(a.sum()) - 1


def _mask(a, smooth_min, patch_min):
    x, y, rank = _from_inliers(a)
    got = _call(x, y, rank, smooth_min, patch_min)
    ref = RR.fwd_bwd(x, y, rank, smooth_min, patch_min)
    assert np.array_equal(ref["mask"] | np.asarray(a, np.uint8), ref["mask"])      # (the restatement's a is the `a` asked for)
    _same_as_reference("neighbourhood", got, ref, x.size)
    return got


def test_checkerboard_of_inliers():
    P = 8
    board = (np.add.outer(np.arange(P), np.arange(P)) % 2 == 0).astype(np.uint8)[None]
    # an interior outlier of a checkerboard has 4 inlier neighbours, an interior inlier 5 (itself and 4 diagonals)
    assert _mask(board, 5, P * P + 1)["stats"] == (32, 32, 32)
    got = _mask(board, 4, P * P + 1)
    assert got["stats"][0] == 32 and got["mask"][0, 1:-1, 1:-1].all() and not got["mask"][0, 0, 1] and not got["mask"][0, 7, 0]
    # with the patch rule met by the 32 inliers alone the inner half fills in
    got = _mask(board, 5, 32)
    assert got["mask"][0, 2:6, 2:6].all() and got["stats"] == (32, 32, 32 + 8)
    assert _mask(board, 5, 33)["stats"] == (32, 32, 32)


def test_no_count_leaks_from_a_patch_into_the_next_one_in_memory():
    P = 4
    a = np.zeros((4, P, P), np.uint8)
    a[0] = 1
    a[2] = 1
    a[3, 0, 0] = 1     # (the patch behind an all-outlier patch: its first pixel is next in memory to patch 2's last)
    got = _mask(a, 1, P * P + 1)
    # smooth_min 1: any inlier in reach forgives.  Patch 1 has none inside: all of it stays out, whatever its neighbours hold
    assert got["mask"][0].all() and not got["mask"][1].any() and got["mask"][2].all()
    assert got["mask"][3].sum() == 4 and got["mask"][3, :2, :2].all()
    for smooth_min in (2, 4, 9):
        assert not _mask(a, smooth_min, P * P + 1)["mask"][1].any()


@pytest.mark.parametrize("where,inliers_around", [((0, 0), 3), ((0, 3), 5), ((7, 7), 3), ((5, 0), 5), ((3, 4), 8)])
def test_a_single_outlier_at_a_corner_on_an_edge_and_inside(where, inliers_around):
    P = 8
    a = np.ones((2, P, P), np.uint8)
    a[1][where] = 0
    for smooth_min in (4, 5, 6):
        got = _mask(a, smooth_min, P * P + 1)
        forgiven = inliers_around >= smooth_min
        assert bool(got["mask"][1][where]) == forgiven and got["stats"] == (2 * P * P - 1,) + (2 * P * P - 1 + forgiven,) * 2


def test_patch_rule_exactly_met_and_missed_by_one():
    P = 16
    a = np.zeros((3, P, P), np.uint8)
    a[0, :, :9] = 1       # 144 inliers in columns 0..8; column 9 is forgiven by smooth_min 2: c counts 160
    a[1, :, :8] = 1       # c counts 144
    a[2] = 1
    x, y, rank = _from_inliers(a)
    c = RR.mask_from_inliers(a, 2, P * P + 1)[0].reshape(3, -1).sum(1)
    assert c.tolist() == [160, 144, 256]
    inner = RR.inner(P)
    assert inner.sum() == 64 and inner[4:12, 4:12].all()
    for patch_min, filled in ((160, (True, False)), (161, (False, False)), (144, (True, True)), (145, (True, False)),
                              (P * P + 1, (False, False))):
        got = _mask(a, 2, patch_min)["mask"]
        for n in (0, 1):
            assert bool(got[n, 4:12, 4:12].all()) == filled[n], (patch_min, n)
            assert np.array_equal(got[n][~inner], RR.mask_from_inliers(a, 2, P * P + 1)[0][n][~inner].astype(np.uint8))
    # off: not even a patch of all inliers counts as P^2 + 1
    assert _mask(a, 2, P * P + 1)["stats"] == (144 + 128 + 256, 160 + 144 + 256, 160 + 144 + 256)


# ---- 4: invariance and repeatability ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", RR.KINDS)
def test_same_bytes_from_call_to_call_and_under_a_permutation_of_the_patches(kind):
    N, P, C = 128, 16, 3
    x, y = RR.inputs(N, P, C)
    rank, patch_min = RR.rank_of_quantile(0.5, N * P * P), RR.patch_min_of_fraction(0.6, P)
    a, b = _call(x, y, rank, 5, patch_min, kind), _call(x, y, rank, 5, patch_min, kind)
    for key in a:
        assert np.array_equal(np.atleast_1d(a[key]).view(np.uint8), np.atleast_1d(b[key]).view(np.uint8)), key
    perm = np.random.default_rng(2).permutation(N)
    c = _call(x[perm], y[perm], rank, 5, patch_min, kind)
    assert _bits(c["tau"]) == _bits(a["tau"]) and c["stats"] == a["stats"]
    assert np.array_equal(c["mask"], a["mask"][perm]) and np.array_equal(_bits(c["d_x"]), _bits(a["d_x"][perm]))


# ---- 5: mask_in --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,P,C", [(3, 16, 3), (1, 64, 4), (5, 6, 1)])
def test_mask_in_replaces_the_selection(N, P, C):
    x, y = RR.inputs(N, P, C)
    rng = np.random.default_rng(3)
    mask = rng.choice(np.array([0, 0, 1, 2, 255], np.uint8), (N, P, P))
    for kind in RR.KINDS:
        # (rank, smooth_min and patch_min are ignored: out-of-range values pass)
        got = _call(x, y, -5, 0, 0, kind, mask_in=mask, grad_scale=0.7)
        ref = RR.fwd_bwd(x, y, kind=kind, mask_in=mask, grad_scale=0.7)
        assert float(got["tau"]) == 0.0 and got["stats"] == (0, 0, 0)
        _same_as_reference(f"mask_in {kind}", got, ref, x.size)


def test_mask_out_may_be_mask_in():
    from voxe_hip.runtime import lib, stream_ptr

    N, P, C = 5, 6, 3
    x, y = RR.inputs(N, P, C)
    mask = np.random.default_rng(4).choice(np.array([0, 1, 7, 255], np.uint8), (N, P, P))
    xt, yt, mt = _t(x), _t(y), _t(mask)
    loss = torch.empty((), device=DEV)
    d_x = torch.empty_like(xt)
    L = lib()
    sc = torch.empty(L.voxe_robust_scratch_bytes(N, P, C), dtype=torch.uint8, device=DEV)
    status = L.voxe_robust_fwd_bwd(xt.data_ptr(), yt.data_ptr(), N, P, C, abi.DREG_L1, 0, 5, 1, mt.data_ptr(), 1.0, loss.data_ptr(),
                                   None, None, mt.data_ptr(), None, d_x.data_ptr(), sc.data_ptr(), sc.numel(), stream_ptr(DEV))
    torch.cuda.synchronize()
    assert status == abi.OK
    ref = RR.fwd_bwd(x, y, mask_in=mask)
    assert np.array_equal(mt.cpu().numpy(), (mask != 0).astype(np.uint8))
    assert np.array_equal(_bits(d_x.cpu().numpy()), _bits(ref["d_x"])) and _scalar_ratio(loss.cpu().numpy(), ref["loss"], x.size) <= 1.0


# ---- 6: the buffer contract ----------------------------------------------------------------------------------------------------------
CONTRACT = (3, 16, 3)
OUTPUTS = ("loss", "mse", "tau", "mask", "stats", "d_x")


def _contract_buffers(k, x, y, mask_in=None):
    from voxe_hip.runtime import lib

    N, P, C = x.shape[0], x.shape[1], x.shape[3]
    M = N * P * P
    bufs = {"x": k.inp("x", x), "y": k.inp("y", y)}
    if mask_in is not None:
        bufs["mask_in"] = k.inp("mask_in", mask_in)
    bufs.update(loss=k.out("loss", 1), mse=k.out("mse", 1), tau=k.out("tau", 1), mask=k.out("mask", M, torch.uint8),
                stats=k.out("stats", 3, torch.int64), d_x=k.out("d_x", M * C))
    bufs["scratch"] = k.scratch("scratch", lib().voxe_robust_scratch_bytes(N, P, C))
    return bufs


def _contract_call(k, bufs, shape, kind, rank, which, nbytes=None, expect=abi.OK):
    from contract import P as ptr_of
    from voxe_hip.runtime import lib, stream_ptr

    N, P, C = shape
    o = [bufs[name].ptr if name in which else None for name in OUTPUTS]
    return k.call(lib().voxe_robust_fwd_bwd, bufs["x"].ptr, bufs["y"].ptr, N, P, C, kind, rank, 5, RR.patch_min_of_fraction(0.6, P),
                  ptr_of(bufs.get("mask_in")), 0.7, *o, bufs["scratch"].ptr, bufs["scratch"].nbytes if nbytes is None else nbytes,
                  stream_ptr(DEV), expect=expect)


@pytest.mark.parametrize("with_mask_in", (False, True))
@pytest.mark.parametrize("kind", (abi.DREG_L1, abi.DREG_L2))
def test_buffer_contract_of_every_output_combination(kind, with_mask_in):
    """every subset of the six outputs, each single one included, under both fills: bands clean, inputs unchanged, an output
    that is not asked for keeps every byte of the fill, one that is holds the bytes of the call with all six"""
    from contract import K

    N, P, C = CONTRACT
    x, y = RR.inputs(N, P, C)
    mask_in = np.random.default_rng(5).choice(np.array([0, 1, 9], np.uint8), (N, P, P)) if with_mask_in else None
    rank = RR.rank_of_quantile(0.5, N * P * P)
    full = {}
    for pattern in (0xFF, 0x00):
        k = K(pattern, capacity=8 << 20)
        bufs = _contract_buffers(k, x, y, mask_in)
        k.begin()
        _contract_call(k, bufs, CONTRACT, kind, rank, OUTPUTS)
        for name in OUTPUTS:
            k.written(bufs[name])
            got = bufs[name].cpu().view(torch.uint8)
            assert torch.equal(full.setdefault(name, got), got), f"{name} depends on what the buffers held before the call"
        for subset in range(1, 2 ** len(OUTPUTS) - 1):
            which = [name for i, name in enumerate(OUTPUTS) if subset >> i & 1]
            k.refill(*(bufs[name] for name in OUTPUTS), bufs["scratch"])
            _contract_call(k, bufs, CONTRACT, kind, rank, which)
            for name in OUTPUTS:
                if name in which:
                    assert torch.equal(bufs[name].cpu().view(torch.uint8), full[name]), (which, name)
                else:
                    assert k.a.poisoned(name) == bufs[name].nbytes, (which, name)
    kind_name = "l1" if kind == abi.DREG_L1 else "l2"
    ref = RR.fwd_bwd(x, y, rank, 5, RR.patch_min_of_fraction(0.6, P), kind_name, mask_in=mask_in, grad_scale=0.7)
    assert np.array_equal(full["mask"].numpy().reshape(N, P, P), ref["mask"])
    assert np.array_equal(full["d_x"].numpy().view(np.uint32).reshape(x.shape), _bits(ref["d_x"]))


def test_buffer_contract_short_scratch_and_no_outputs():
    from contract import K, Stop

    N, P, C = CONTRACT
    x, y = RR.inputs(N, P, C)
    # one byte short: refused, and the whole arena -- outputs, scratch, bands -- as it was
    k = K(0xFF, short="scratch", capacity=8 << 20)
    bufs = _contract_buffers(k, x, y)
    k.begin()
    with pytest.raises(Stop):
        _contract_call(k, bufs, CONTRACT, abi.DREG_L1, 7, OUTPUTS, nbytes=k.size(bufs["scratch"], "scratch"))
    # no output: VOXE_OK and nothing is launched (the scratch keeps its fill)
    k = K(0xFF, capacity=8 << 20)
    bufs = _contract_buffers(k, x, y)
    k.begin()
    _contract_call(k, bufs, CONTRACT, abi.DREG_L1, 7, ())
    assert all(k.a.poisoned(name) == bufs[name].nbytes for name in OUTPUTS + ("scratch",))


def test_one_nan_pixel_neither_hangs_nor_leaves_the_buffers():
    """the call returns, the mask bytes are 0 or 1, the guard bands are intact and the inputs unchanged; nothing else is asserted"""
    from contract import K

    for shape in ((3, 16, 3), (1, 4, 1)):
        N, P, C = shape
        x, y = RR.inputs(N, P, C)
        x[0, 1, 2, 0] = np.nan
        for rank in (0, N * P * P // 2, N * P * P - 1):
            k = K(0xFF, capacity=8 << 20)
            bufs = _contract_buffers(k, x, y)
            k.begin()
            _contract_call(k, bufs, shape, abi.DREG_L1, rank, OUTPUTS)
            assert int(bufs["mask"].t.max()) <= 1


# ---- 7: autograd ---------------------------------------------------------------------------------------------------------------------
def _stable_inputs(N, P, C, q):
    """inputs whose mask does not depend on the precision: no residual within 1e-3 (relative) of tau, no d_c == 0"""
    M = N * P * P
    for seed in range(20):
        x, y = RR.inputs(N, P, C, seed=seed)
        e = RR.residuals(x, y).astype(np.float64).reshape(-1)
        tau = np.partition(e, RR.rank_of_quantile(q, M))[RR.rank_of_quantile(q, M)]
        near = np.abs(e - tau) <= 1e-3 * tau
        if near.sum() == 1 and (x != y).all():          # (tau itself)
            return x, y
    raise AssertionError("no seed gave stable inputs")


@pytest.mark.parametrize("kind", RR.KINDS)
def test_autograd_op_equals_the_direct_call_and_the_float64_gradient(kind):
    N, P, C = 3, 16, 3
    M = N * P * P
    x, y = _stable_inputs(N, P, C, 0.5)
    rank, patch_min = RR.rank_of_quantile(0.5, M), RR.patch_min_of_fraction(0.6, P)
    direct = _call(x, y, rank, 5, patch_min, kind)
    xt = _t(x).requires_grad_(True)
    loss, mse, mask, info = ops.robust_loss(xt, _t(y), kind=kind)
    assert (info["rank"], info["smooth_min"], info["patch_min"]) == (rank, 5, patch_min)
    assert loss.requires_grad and not mse.requires_grad and mask.dtype == torch.uint8 and not mask.requires_grad
    (3.0 * loss).backward()
    assert np.array_equal(_bits(xt.grad.cpu().numpy()), _bits(3.0 * torch.from_numpy(direct["d_x"])))
    assert _bits(loss.detach().cpu().numpy()) == _bits(direct["loss"]) and _bits(mse.cpu().numpy()) == _bits(direct["mse"])
    assert np.array_equal(mask.cpu().numpy(), direct["mask"]) and tuple(int(v) for v in info["stats"].cpu()) == direct["stats"]
    assert _bits(info["tau"].cpu().numpy()) == _bits(direct["tau"])
    # the float64 restatement: residuals, threshold and mask in double give the same mask, and the analytic gradient of the
    # masked mean is w sign(d) / CM or 2 w d / CM.  The kernel rounds g = 1 / CM to float and forms one product, autograd
    # multiplies by the upstream 3: three roundings of 2^-24 each, and one more for their second-order terms
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    d = x64 - y64
    e = (d * d).sum(-1)
    a = (e <= np.partition(e.reshape(-1), rank)[rank]).astype(np.int64)
    w = RR.mask_from_inliers(a, 5, patch_min)[1]
    assert np.array_equal(w.astype(np.uint8), direct["mask"])
    grad = 3.0 * w[..., None] * (np.sign(d) if kind == "l1" else 2.0 * d) / (C * M)
    err = np.abs(xt.grad.cpu().numpy().astype(np.float64) - grad)
    assert (err <= 4 * 2.0 ** -24 * np.abs(grad)).all(), float((err / np.maximum(np.abs(grad), 1e-300)).max())
    # the mask alone, and the mask handed to a second call (the trainer's diffuse term)
    only, info2 = ops.robust_mask(_t(x), _t(y))
    assert torch.equal(only, mask) and torch.equal(info2["stats"], info["stats"]) and torch.equal(info2["tau"], info["tau"])
    again = ops.robust_loss(_t(x), _t(y), kind=kind, mask=mask)
    assert _bits(again[0].cpu().numpy()) == _bits(direct["loss"]) and torch.equal(again[2], mask)
    assert not again[3]["stats"].any() and float(again[3]["tau"]) == 0.0


# ---- 8: the trainer ----------------------------------------------------------------------------------------------------------------
def _sphere_views(count):
    from test_trainers_gpu import _sphere_model
    from thre3d_atom.utils.imaging_utils import CameraIntrinsics, pose_spherical

    torch.manual_seed(1)
    truth = _sphere_model(side=24, samples=96)
    intr = CameraIntrinsics(48, 48, 0.5 * 48 / np.tan(0.5 * 0.6911112))
    poses, images = [], []
    for i in range(count):
        pose = pose_spherical(360.0 * i / count, 20.0 + 50.0 * ((i * 0.618) % 1.0), 4.0311)
        poses.append(torch.cat([pose.rotation, pose.translation], dim=1))
        images.append(truth.render(pose, intr, perturb_sampled_points=False).colour.permute(2, 0, 1).cpu())
    return torch.stack(images), torch.stack(poses), intr


def _fresh_model(bounds, render_samples=None):
    from thre3d_atom.modules.volumetric_model import VolumetricModel
    from thre3d_atom.thre3d_reprs.renderers import SHVoxGridRenderConfig, render_sh_voxel_grid
    from thre3d_atom.thre3d_reprs.voxels import VoxelGrid, VoxelSize

    g = torch.Generator().manual_seed(3)
    vg = VoxelGrid(torch.empty(24, 24, 24, 1).uniform_(-1, 1, generator=g), torch.empty(24, 24, 24, 3).uniform_(-1, 1, generator=g),
                   VoxelSize(0.125, 0.125, 0.125), density_preactivation=torch.nn.Identity(),
                   density_postactivation=torch.nn.Softplus(), expected_density_scale=100.0 / 3.0, tunable=True)
    config = SHVoxGridRenderConfig(96, bounds, white_bkgd=True, **({} if render_samples is None else
                                                                   {"render_num_samples_per_ray": render_samples}))
    return VolumetricModel(vg, render_sh_voxel_grid, config, device=DEV)


def test_trainer_hands_the_specular_mask_to_the_diffuse_term_and_to_the_exposure_loss(tmp_path):
    from thre3d_atom.data.datasets import InMemoryPosedImages
    from thre3d_atom.modules.trainers import train_sh_vox_grid_vol_mod_with_posed_images
    from thre3d_atom.utils.imaging_utils import CameraBounds

    images, poses, intr = _sphere_views(4)
    bounds = CameraBounds(1.8, 6.6)
    data = InMemoryPosedImages(images, poses, intr, bounds)
    seen, weights = [], []
    real_loss, real_exposure = ops.robust_loss, ops.exposure_loss

    def spy(x, y, **kw):
        out = real_loss(x, y, **kw)
        seen.append((kw.get("mask"), out[2], x.requires_grad, tuple(x.shape)))
        return out

    def spy_exposure(colour, target, image_ids, delta, **kw):
        weights.append(kw.get("ray_weight"))
        return real_exposure(colour, target, image_ids, delta, **kw)

    def train(**kw):
        train_sh_vox_grid_vol_mod_with_posed_images(_fresh_model(bounds), data, tmp_path, random_initializer=lambda t: t,
                                                    ray_batch_size=4096, num_stages=1, num_iterations_per_stage=3,
                                                    fast_debug_mode=True, robust_loss=True, **kw)

    ops.robust_loss, ops.exposure_loss = spy, spy_exposure
    try:
        train()
        assert len(seen) == 6 and not weights
        for (mask_in, mask_out, grad, shape), (mask_in2, mask_out2, grad2, _) in zip(seen[0::2], seen[1::2]):
            assert mask_in is None and mask_in2 is mask_out and torch.equal(mask_out2, mask_out) and grad and grad2
            assert shape == (16, 16, 16, 3) and mask_out.dtype == torch.uint8 and int(mask_out.max()) == 1
        # under exposure compensation the mask goes to the existing exposure loss as per-ray weights, for both terms
        del seen[:]
        train(exposure_learning_rate=1e-2)
        assert not seen and len(weights) == 6
        for spec, diff in zip(weights[0::2], weights[1::2]):
            assert spec is diff and spec.shape == (4096,) and spec.dtype == torch.float32
            assert set(spec.unique().tolist()) <= {0.0, 1.0} and 0.5 <= float(spec.mean()) <= 1.0
    finally:
        ops.robust_loss, ops.exposure_loss = real_loss, real_exposure
