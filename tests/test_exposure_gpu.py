"""GPU checks of the per-image exposure compensation (voxe_exposure_fwd_bwd / _apply_bwd / _fit_sums, ops.exposure_loss,
ops.fit_affine_colour, thre3d_reprs.exposure, the trainer's exposure_learning_rate and the tester's colour-corrected metrics)
against the float64 restatement tests/exposure_ref.py.  The inputs are exposure_ref.inputs(); tests/test_exposure_host.py
checks on the host that they keep the L1 residuals away from 0.

Bounds.  Every comparison is |error| <= k * 2^-24 * sum|terms| with the restatement's own sum of |terms| (residuals expanded, see
exposure_ref) and k = the float32 roundings a term passes through in voxe_exposure.hip as written, plus 2; the K_* tables below
count them.  d_delta adds the fixed point's own resolution, 2^-33 per product before the scale applies.  Nothing is tuned."""
import logging
import re

import numpy as np
import pytest
import torch

import exposure_ref as ER
from voxe_hip import abi, ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U24 = 2.0 ** -24

# float32 roundings per term, in the order the kernel performs them, + 2
#   corrected : a_cc = 1 + dA_cc (1), c' = fma(a2, x2, fma(a1, x1, fma(a0, x0, b))) (3)
K_CORRECTED = 4 + 2
#   d_x  L2   : c' (4), e = c' - y (1), g = (2 w) e (1; 2 w is exact), the a_cj of the outer factor (1),
#               a0 g0, fma, fma (3), gs = (float)(grad_scale / 3R) (1), gs * (...) (1)
#        L1   : g = w sign(e) is exact; a_cj (1), the chain (3), gs (1), gs * (1)
K_DX = {"l2": 12 + 2, "l1": 6 + 2}
#   d_delta L2: c' (4), e (1), g (1), t = g x_j (1), then integers; (float)(acc 2^-32 gs) with gs in double (1)
#        L1   : t = g x_j (1), the final conversion (1)
#   plus per product the fixed point's 2^-33, times |gs|, times the rays of the image
K_DDELTA = {"l2": 8 + 2, "l1": 2 + 2}
#   loss L2, mse: each factor e of e * e carries c' (4) + e (1); the product and every sum are double; (float) at the end (1)
#   loss L1     : |e| (5), w |e| and the sums in double, (float) (1)
K_LOSS = {"l2": 11 + 2, "l1": 6 + 2}
K_MSE = 11 + 2
#   apply_bwd d_x : a_cj (1), the chain (3);  d_delta: t = (g unit) x_j (1; unit is a power of two), the final conversion (1)
K_BWD_DX, K_BWD_DDELTA = 4 + 2, 2 + 2


def _t(a, dtype=None):
    return None if a is None else torch.as_tensor(a, dtype=dtype).to(DEV)


def _call(x, y, ids, delta, kind, w=None, grad_scale=1.0, d_delta=None, accumulate=False):
    """(loss, mse, corrected, d_x, d_delta) as numpy"""
    xt, yt, it, dt, wt = _t(x), _t(y), _t(ids), _t(delta), _t(w)
    d_x = torch.full_like(xt, float("nan"))
    dd = torch.full_like(dt, float("nan")) if d_delta is None else d_delta
    loss, mse, corrected = ops.exposure_fwd_bwd(xt, yt, it, dt, kind, wt, grad_scale=grad_scale, want_mse=True, want_corrected=True,
                                                d_colour=d_x, d_delta=dd, accumulate=accumulate)
    return float(loss), float(mse), corrected.cpu().numpy(), d_x.cpu().numpy(), dd.cpu().numpy()


def _within(name, got, ref_abs, k, extra=0.0, where=None):
    """|got - ref| <= k 2^-24 sum|terms| + extra wherever `where`; prints the worst ratio error / bound"""
    ref, mag = ref_abs
    err = np.abs(np.asarray(got, np.float64) - ref)
    bound = k * U24 * mag + extra
    ok = np.ones(err.shape, bool) if where is None else where
    ratio = float(np.max(np.where(ok & (bound > 0), err / np.where(bound > 0, bound, 1.0), 0.0), initial=0.0))
    assert bool(np.all(np.where(ok, err <= bound, True))), (name, ratio, float(err.max()))
    return ratio


# ---- 1: forward and backward against the restatement ---------------------------------------------------------------------
@pytest.mark.parametrize("R,N", ER.cases())
def test_forward_and_backward_agree_with_the_restatement(R, N):
    worst = {}
    for kind, weighted, pattern in ER.variants():
        x, y, ids, delta, w = ER.inputs(R, N, pattern, weighted)
        ref = ER.fwd_bwd(x, y, ids, delta, kind, w, grad_scale=0.7)
        loss, mse, corrected, d_x, d_delta = _call(x, y, ids, delta, kind, w, grad_scale=0.7)
        tag = f"{kind}{'_w' if weighted else ''}_{pattern}"
        # L1: what a residual too close to 0 for a float32 sign enters is left out, and that is at most 0.1 % of the residuals
        flip = ref["flip"]
        keep_x = np.repeat(~flip.any(axis=1)[:, None], 3, axis=1)
        keep_d = ~ER.delta_rows_with_flips(ids, N, flip)
        assert (~keep_x).mean() <= ER.FLIP_CAP and (~keep_d).mean() <= ER.FLIP_CAP, (tag, int(flip.sum()))
        fixed = abs(ref["gs"]) * ref["count"][:, None] * 2.0 ** -33
        r = {"corrected": _within(tag, corrected, ref["corrected"], K_CORRECTED),
             "loss": _within(tag, loss, ref["loss"], K_LOSS[kind]),
             "mse": _within(tag, mse, ref["mse"], K_MSE),
             "d_x": _within(tag, d_x, ref["d_x"], K_DX[kind], where=keep_x),
             "d_delta": _within(tag, d_delta, ref["d_delta"], K_DDELTA[kind], extra=fixed, where=keep_d)}
        for key, v in r.items():
            worst[key] = max(worst.get(key, 0.0), v)
        # rows of images that no ray names: exact zeros, sign included
        unused = d_delta[~ref["used"]]
        assert not unused.any() and not np.signbit(unused).any(), tag
        assert np.isfinite(d_x).all() and np.isfinite(d_delta).all(), tag
    print(f"R {R} N {N}: worst error / bound " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))


def test_ids_out_of_range_are_clamped():
    x, y, ids, delta, w = ER.inputs(257, 3, "shuffle", True)
    wild = ids.copy()
    wild[::5] = np.array([-7, 3, 1 << 30, -(1 << 31)], np.int64).astype(np.int32)[np.arange(len(wild[::5])) % 4]
    a = _call(x, y, wild, delta, "l2", w)
    b = _call(x, y, np.clip(wild, 0, 2), delta, "l2", w)
    assert a[0] == b[0] and a[1] == b[1] and all(np.array_equal(p, q) for p, q in zip(a[2:], b[2:]))


# ---- 2: reproducibility ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ER.KINDS)
def test_same_bits_from_call_to_call_and_under_a_permutation_of_the_rays(kind):
    R, N = 4099, 70
    x, y, ids, delta, w = ER.inputs(R, N, "shuffle", True)
    a, b = _call(x, y, ids, delta, kind, w), _call(x, y, ids, delta, kind, w)
    assert a[0] == b[0] and a[1] == b[1] and all(np.array_equal(p, q) for p, q in zip(a[2:], b[2:]))
    # fixed point: any order of the rays gives the bits of d_delta (sorted runs and a second shuffle)
    for perm in (np.argsort(ids, kind="stable"), np.random.default_rng(1).permutation(R)):
        c = _call(x[perm], y[perm], ids[perm], delta, kind, w[perm])
        assert np.array_equal(c[4].view(np.int32), a[4].view(np.int32))
        assert np.array_equal(c[3], a[3][perm]) and np.array_equal(c[2], a[2][perm])
        ref = ER.fwd_bwd(x, y, ids, delta, kind, w)
        _within("loss permuted", c[0], ref["loss"], K_LOSS[kind])


# ---- 3: accumulate, grad_scale, R == 0 ---------------------------------------------------------------------------------------
def test_accumulate_grad_scale_and_no_rays():
    R, N = 257, 70
    x, y, ids, delta, w = ER.inputs(R, N, "unused", True)
    ref = ER.fwd_bwd(x, y, ids, delta, "l1", w)
    fresh = _call(x, y, ids, delta, "l1", w)
    # accumulate adds to what is there and leaves the rows of unused images alone, bit for bit (-0.0 stays -0.0)
    before = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, (N, 12)).astype(np.float32))
    before[~torch.from_numpy(ref["used"])] = -0.0
    before[1] = 0.25                                       # (image 1 is unused too: 7 does not divide it)
    assert not ref["used"][1]
    buf = before.clone().to(DEV)
    got = _call(x, y, ids, delta, "l1", w, d_delta=buf, accumulate=True)[4]
    want = (before + torch.from_numpy(fresh[4])).numpy()
    assert np.array_equal(got[ref["used"]], want[ref["used"]])
    assert np.array_equal(got[~ref["used"]].view(np.int32), before.numpy()[~ref["used"]].view(np.int32))
    # grad_scale scales both gradients and neither scalar: a power of two exactly
    half = _call(x, y, ids, delta, "l1", w, grad_scale=0.5)
    assert half[0] == fresh[0] and half[1] == fresh[1] and np.array_equal(half[2], fresh[2])
    assert np.array_equal(half[3], 0.5 * fresh[3]) and np.array_equal(half[4], 0.5 * fresh[4])
    zero = _call(x, y, ids, delta, "l2", w, grad_scale=0.0)
    assert not zero[3].any() and not zero[4].any()
    # R == 0: the outputs that exist are zeroed, d_delta only when it does not accumulate
    e3 = np.zeros((0, 3), np.float32)
    empty = _call(e3, e3, np.zeros(0, np.int32), delta, "l1")
    assert empty[0] == 0.0 and empty[1] == 0.0 and empty[2].shape == (0, 3) and not empty[4].any() and np.isfinite(empty[4]).all()
    buf = before.clone().to(DEV)
    kept = _call(e3, e3, np.zeros(0, np.int32), delta, "l1", d_delta=buf, accumulate=True)[4]
    assert np.array_equal(kept.view(np.int32), before.numpy().view(np.int32))


# ---- 4: the chain rule of the corrected colours alone ------------------------------------------------------------------------
@pytest.mark.parametrize("R,N,pattern", [(1, 1, "one"), (65, 3, "runs64"), (4099, 70, "shuffle"), (4099, 70, "unused")])
def test_apply_and_its_backward_agree_with_the_restatement(R, N, pattern):
    x, y, ids, delta, _ = ER.inputs(R, N, pattern, False)
    g = ((y - 0.5) / R).astype(np.float32)                 # an upstream gradient of a mean over the batch
    ref = ER.apply_bwd(x, ids, delta, g)
    xt, dt = _t(x).requires_grad_(True), _t(delta).requires_grad_(True)
    corrected = ops.exposure_apply(xt, _t(ids), dt)
    _within("apply", corrected.detach().cpu().numpy(), ER.fwd_bwd(x, y, ids, delta, "l2")["corrected"], K_CORRECTED)
    corrected.backward(_t(g))
    unit = 2.0 ** np.ceil(np.log2(R))
    a = _within("apply d_x", xt.grad.cpu().numpy(), ref["d_x"], K_BWD_DX)
    b = _within("apply d_delta", dt.grad.cpu().numpy(), ref["d_delta"], K_BWD_DDELTA, extra=ref["count"][:, None] * 2.0 ** -33 / unit)
    print(f"apply_bwd R {R} N {N} {pattern}: worst error / bound d_x {a:.2f} d_delta {b:.2f}")
    assert not dt.grad.cpu().numpy()[ref["count"] == 0].any()
    again = torch.empty_like(dt)
    ops.exposure_apply_bwd(_t(x), _t(ids), _t(delta), _t(g), d_delta=again)
    assert torch.equal(again, dt.grad)


# ---- 5: fit sums and the fitted affine -----------------------------------------------------------------------------------------
def _fit_inputs(N, P, seed=0):
    rng = np.random.default_rng([N, P, seed])
    x = rng.uniform(0, 1, (N, P, 3)).astype(np.float32)
    A = np.eye(3) + rng.uniform(-0.3, 0.3, (N, 3, 3))
    b = rng.uniform(-0.05, 0.05, (N, 3))
    y = (np.einsum("ncj,npj->npc", A, x.astype(np.float64)) + b[:, None, :]).astype(np.float32)
    return x, y


@pytest.mark.parametrize("N", (1, 3))
@pytest.mark.parametrize("P", (1, 5, 64, 65, 1499, 2048, 2049, 5000))   # (2049: the first size with two blocks per image)
def test_fit_sums_agree_with_float64(N, P):
    x, y = _fit_inputs(N, P)
    ref, mag = ER.fit_sums(x, y)
    got = ops.exposure_fit_sums(_t(x), _t(y))
    assert got.dtype == torch.float64 and got.shape == (N, 25)
    err = np.abs(got.cpu().numpy() - ref)
    # products of two float32 are exact in double; a sum of P terms in any order errs by at most (P - 1) 2^-53 sum|terms|
    bound = P * 2.0 ** -53 * mag
    print(f"fit sums N {N} P {P}: worst error / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    assert torch.equal(got, ops.exposure_fit_sums(_t(x), _t(y)))          # the same bits from call to call


@pytest.mark.parametrize("P", (64, 1499, 5000))
def test_fitted_affine_equals_least_squares(P):
    N = 3
    x, y = _fit_inputs(N, P, seed=1)
    A, b = ops.fit_affine_colour(_t(x), _t(y))
    assert A.shape == (N, 3, 3) and b.shape == (N, 3) and A.dtype == torch.float64
    G, _ = ER.gram(ER.fit_sums(x, y)[0])
    for n in range(N):
        cond = np.linalg.cond(G[n])
        assert cond <= 1e4, cond
        U = np.concatenate([x[n].astype(np.float64), np.ones((P, 1))], axis=1)
        theta = np.linalg.lstsq(U, y[n].astype(np.float64), rcond=None)[0]         # [4,3]
        err = max(np.abs(A[n].cpu().numpy() - theta[:3].T).max(), np.abs(b[n].cpu().numpy() - theta[3]).max())
        tol = P * 2.0 ** -53 * cond
        print(f"fit P {P} image {n}: cond(G) {cond:.1f}, max |fit - lstsq| {err:.2e} (tolerance {tol:.2e})")
        assert err <= tol


def test_fit_of_degenerate_images_is_finite():
    one = np.random.default_rng(0).uniform(0, 1, (2, 1, 3)).astype(np.float32)
    A, b = ops.fit_affine_colour(_t(one), _t(one[::-1].copy()))
    assert bool(torch.isfinite(A).all()) and bool(torch.isfinite(b).all())
    flat_x, flat_y = np.full((1, 300, 3), 0.5, np.float32), np.full((1, 300, 3), 0.25, np.float32)
    A, b = ops.fit_affine_colour(_t(flat_x), _t(flat_y))
    assert bool(torch.isfinite(A).all()) and bool(torch.isfinite(b).all())
    assert np.allclose((A[0].cpu().numpy() @ np.full(3, 0.5) + b[0].cpu().numpy()), 0.25, atol=1e-8)


# ---- 6: autograd ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ER.KINDS)
def test_autograd_op_equals_the_direct_call(kind):
    x, y, ids, delta, w = ER.inputs(4099, 3, "shuffle", True)
    loss0, mse0, corrected0, d_x0, d_delta0 = _call(x, y, ids, delta, kind, w)
    xt, dt = _t(x).requires_grad_(True), _t(delta).requires_grad_(True)
    loss, mse, corrected = ops.exposure_loss(xt, _t(y), _t(ids), dt, kind=kind, ray_weight=_t(w), return_corrected=True)
    assert loss.dim() == 0 and float(loss.detach()) == loss0 and float(mse) == mse0 and np.array_equal(corrected.cpu().numpy(), corrected0)
    assert not mse.requires_grad and not corrected.requires_grad
    (2.5 * loss).backward()
    assert torch.equal(xt.grad, _t(d_x0) * 2.5) and torch.equal(dt.grad, _t(d_delta0) * 2.5)
    # only the inputs that require a gradient get one; int64 ids are taken
    dt2 = _t(delta).requires_grad_(True)
    out = ops.exposure_loss(_t(x), _t(y), _t(ids.astype(np.int64)), dt2, kind=kind, ray_weight=_t(w))
    assert len(out) == 2 and float(out[0].detach()) == loss0
    out[0].backward()
    assert torch.equal(dt2.grad, _t(d_delta0))
    from thre3d_atom.thre3d_reprs.exposure import PerImageExposure

    module = PerImageExposure(3).to(DEV)
    with torch.no_grad():
        module.delta.copy_(_t(delta))
    got = module(_t(x), _t(y), _t(ids), kind=kind, ray_weight=_t(w))
    assert float(got[0].detach()) == loss0 and float(got[1]) == mse0
    assert np.array_equal(module.corrected(_t(x), _t(ids)).cpu().numpy(), corrected0)


# ---- 7: the buffer contract (tests/contract.py, tests/arena.py) -------------------------------------------------------------
CONTRACT_R, CONTRACT_N = 1499, 7


def _contract_inputs():
    x, y, ids, delta, w = ER.inputs(CONTRACT_R, CONTRACT_N, "shuffle", True)
    ids = ids.copy()
    ids[::97] = CONTRACT_N + 5          # out of range on purpose: clamped, and nothing lands outside d_delta
    ids[50::97] = -2
    return x, y, ids, delta, w


def exposure_case(k, kind):
    from contract import P
    from voxe_hip.runtime import lib, stream_ptr

    L, st = lib(), stream_ptr(DEV)
    x, y, ids, delta, w = _contract_inputs()
    R, N = CONTRACT_R, CONTRACT_N
    bx, by, bi, bd, bw = k.inp("x", x), k.inp("y", y), k.inp("image_id", ids), k.inp("delta", delta), k.inp("ray_weight", w)
    loss, mse = k.out("loss", 1), k.out("mse", 1)
    corrected, d_x, d_delta = k.out("corrected", 3 * R), k.out("d_x", 3 * R), k.out("d_delta", 12 * N)
    scr = k.scratch("scratch", L.voxe_exposure_scratch_bytes(R, N))
    k.begin()
    k.call(L.voxe_exposure_fwd_bwd, bx.ptr, by.ptr, bi.ptr, R, bd.ptr, N, kind, bw.ptr, 0.7, loss.ptr, mse.ptr, corrected.ptr,
           d_x.ptr, d_delta.ptr, 0, scr.ptr, k.size(scr, "scratch"), st)
    for buf in (loss, mse, corrected, d_x, d_delta):
        k.bits(buf)
    ref = ER.fwd_bwd(x, y, ids, delta, "l1" if kind == abi.DREG_L1 else "l2", w, grad_scale=0.7)
    _within("contract corrected", corrected.cpu().numpy().reshape(R, 3), ref["corrected"], K_CORRECTED)


def exposure_bwd_case(k):
    from voxe_hip.runtime import lib, stream_ptr

    L, st = lib(), stream_ptr(DEV)
    x, y, ids, delta, _ = _contract_inputs()
    R, N = CONTRACT_R, CONTRACT_N
    bx, bi, bd = k.inp("x", x), k.inp("image_id", ids), k.inp("delta", delta)
    bg = k.inp("d_corrected", ((y - 0.5) / R).astype(np.float32))
    d_x, d_delta = k.out("d_x", 3 * R), k.out("d_delta", 12 * N)
    scr = k.scratch("scratch", L.voxe_exposure_scratch_bytes(R, N))
    k.begin()
    k.call(L.voxe_exposure_apply_bwd, bx.ptr, bi.ptr, R, bd.ptr, N, bg.ptr, d_x.ptr, d_delta.ptr, 0, scr.ptr,
           k.size(scr, "scratch"), st)
    k.bits(d_x)
    k.bits(d_delta)


def exposure_empty_case(k):
    """R == 0 with the per-ray outputs only: VOXE_OK and nothing is touched (loss_out, mse_out and a d_delta that does not
    accumulate are zeroed by the header: not this case)"""
    from voxe_hip.runtime import lib, stream_ptr

    L, st = lib(), stream_ptr(DEV)
    x, y, ids, delta, w = _contract_inputs()
    bx, by, bi, bd, bw = k.inp("x", x), k.inp("y", y), k.inp("image_id", ids), k.inp("delta", delta), k.inp("ray_weight", w)
    corrected, d_x, d_delta = k.out("corrected", 3 * CONTRACT_R), k.out("d_x", 3 * CONTRACT_R), k.out("d_delta", 12 * CONTRACT_N)
    scr = k.scratch("scratch", L.voxe_exposure_scratch_bytes(CONTRACT_R, CONTRACT_N))
    k.begin()
    k.call(L.voxe_exposure_fwd_bwd, bx.ptr, by.ptr, bi.ptr, k.count(CONTRACT_R), bd.ptr, CONTRACT_N, abi.DREG_L1, bw.ptr, 1.0, None,
           None, corrected.ptr, d_x.ptr, d_delta.ptr, 1, scr.ptr, scr.nbytes, st)
    raise AssertionError("only run_empty() runs this case")


def fit_case(k, N, P):
    from voxe_hip.runtime import lib, stream_ptr

    L, st = lib(), stream_ptr(DEV)
    x, y = _fit_inputs(N, P)
    bx, by = k.inp("x", x), k.inp("y", y)
    sums = k.out("sums", 25 * N, torch.float64)
    scr = k.scratch("scratch", L.voxe_exposure_fit_scratch_bytes(N, P))
    k.begin()
    k.call(L.voxe_exposure_fit_sums, bx.ptr, by.ptr, N, P, sums.ptr, scr.ptr, k.size(scr, "scratch"), st)
    k.bits(sums)
    ref, mag = ER.fit_sums(x, y)
    assert (np.abs(sums.cpu().numpy().reshape(N, 25) - ref) <= P * 2.0 ** -53 * mag).all()


@pytest.mark.parametrize("kind", (abi.DREG_L1, abi.DREG_L2))
def test_buffer_contract(kind):
    from contract import run_contract

    run_contract(exposure_case, kind)


def test_buffer_contract_of_the_chain_rule_and_the_fit_sums():
    from contract import run_contract

    run_contract(exposure_bwd_case)
    run_contract(fit_case, CONTRACT_N, CONTRACT_R)
    run_contract(fit_case, 2, 2500)


def test_buffer_contract_short_scratch_and_no_rays():
    from contract import run_empty, run_short

    run_short(exposure_case, "scratch", abi.DREG_L1)
    run_short(exposure_bwd_case, "scratch")
    run_short(fit_case, "scratch", 2, 2500)
    run_empty(exposure_empty_case)


# ---- 8: the trainer and the tester ---------------------------------------------------------------------------------------------
class _Capture(logging.Handler):
    def __init__(self):
        super().__init__()
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def test_trainer_learns_the_exposures_of_a_capture_that_varies(tmp_path):
    """The schedule of test_trainers_gpu.test_reconstruction_trainer_fits_synthetic_views (2 stages of 150 iterations, 4 096
    rays) on 12 views under per-channel gains in [0.7, 1.3] and biases in +-0.05, 4 views held out untouched.  Only the ordering
    is asserted.  Measured on an MI355X, without / with exposure_learning_rate = 1e-2:
        final training loss   0.201 / 0.028        training PSNR of the last batch   17.7 / 34.9 dB
        held-out cc_psnr      16.11 / 17.77 dB     held-out cc_ssim                  0.428 / 0.575
    The raw held-out PSNR is 8.0 / 7.9 dB in both arms: a run this short leaves the tester's AABB-clipped renders far from the
    photographs whatever the exposure, which is why the comparison is made on the colour-corrected figures."""
    from test_trainers_gpu import _sphere_model
    from thre3d_atom.data.datasets import InMemoryPosedImages
    from thre3d_atom.modules.testers import test_sh_vox_grid_vol_mod_with_posed_images as evaluate
    from thre3d_atom.modules.trainers import train_sh_vox_grid_vol_mod_with_posed_images
    from thre3d_atom.modules.volumetric_model import VolumetricModel, create_volumetric_model_from_saved_model
    from thre3d_atom.thre3d_reprs.renderers import SHVoxGridRenderConfig, render_sh_voxel_grid
    from thre3d_atom.thre3d_reprs.voxels import VoxelGrid, VoxelSize, create_voxel_grid_from_saved_info_dict
    from thre3d_atom.utils.imaging_utils import CameraBounds, CameraIntrinsics, pose_spherical
    from thre3d_atom.utils.logging import log

    # the synthetic views of test_trainers_gpu: 12 to train on, each under its own gain and bias; 4 held out, untouched
    torch.manual_seed(1)
    truth = _sphere_model(side=24, samples=96)
    intr = CameraIntrinsics(48, 48, 0.5 * 48 / np.tan(0.5 * 0.6911112))
    poses, images = [], []
    for i in range(16):
        pose = pose_spherical(360.0 * i / 16, 20.0 + 50.0 * ((i * 0.618) % 1.0), 4.0311)
        poses.append(torch.cat([pose.rotation, pose.translation], dim=1))
        images.append(truth.render(pose, intr, perturb_sampled_points=False).colour.permute(2, 0, 1).cpu())
    images, poses = torch.stack(images), torch.stack(poses)
    held = torch.arange(16) % 4 == 3
    rng = np.random.default_rng(7)
    gain = torch.from_numpy(rng.uniform(0.7, 1.3, (12, 3, 1, 1)).astype(np.float32))
    bias = torch.from_numpy(rng.uniform(-0.05, 0.05, (12, 3, 1, 1)).astype(np.float32))
    bounds = CameraBounds(1.8, 6.6)
    train = InMemoryPosedImages(images[~held] * gain + bias, poses[~held], intr, bounds)
    test = InMemoryPosedImages(images[held], poses[held], intr, bounds)

    def run(out, **kw):
        torch.manual_seed(5)
        g = torch.Generator().manual_seed(3)
        vg = VoxelGrid(torch.empty(24, 24, 24, 1).uniform_(-1, 1, generator=g), torch.empty(24, 24, 24, 3).uniform_(-1, 1, generator=g),
                       VoxelSize(0.125, 0.125, 0.125), density_preactivation=torch.nn.Identity(),
                       density_postactivation=torch.nn.Softplus(), expected_density_scale=100.0 / 3.0, tunable=True)
        # (the held-out views are rendered with the training's sample count, as test_trainers_gpu's models are)
        vm = VolumetricModel(vg, render_sh_voxel_grid, SHVoxGridRenderConfig(96, bounds, white_bkgd=True, render_num_samples_per_ray=96),
                             device=DEV)
        cap = _Capture()
        log.addHandler(cap)
        try:
            train_sh_vox_grid_vol_mod_with_posed_images(vm, train, out, random_initializer=lambda t: t, ray_batch_size=4096,
                                                        num_stages=2, num_iterations_per_stage=150, summary_freq=150,
                                                        save_freq=10 ** 6, fast_debug_mode=True, **kw)
        finally:
            log.removeHandler(cap)
        losses = [float(m.group(1)) for m in (re.search(r"loss:\s*([-+0-9.eE]+)", line) for line in cap.lines) if m]
        print(f"{kw}: logged losses {losses}; " + " | ".join(line for line in cap.lines if "psnr" in line))
        return vm, losses[-1], cap.lines

    plain, loss_plain, lines_plain = run(tmp_path / "plain")
    exposed, loss_exposed, lines_exposed = run(tmp_path / "exposed", exposure_learning_rate=1e-2)
    assert plain.exposure is None and not any("exposure" in line for line in lines_plain)
    assert sum("exposure_learning_rate > 0" in line and "no one-call iteration" in line for line in lines_exposed) == 1
    assert exposed.exposure.delta.shape == (12, 12) and bool(exposed.exposure.delta.detach().any())

    # the tester: cc_psnr only when asked for or when the model carries exposures; the other keys as they were
    base = evaluate(plain, test)
    assert set(base) == {"psnr", "ssim"}
    cc_plain = evaluate(plain, test, colour_corrected=True)
    cc_exposed = evaluate(exposed, test)
    print(f"tester: plain {base}; plain, colour-corrected {cc_plain}; with exposure {cc_exposed}")
    # (the renders are jittered: two evaluations of one model agree closely, not bit for bit)
    assert set(cc_plain) == set(cc_exposed) == {"psnr", "ssim", "cc_psnr", "cc_ssim"}
    assert abs(cc_plain["psnr"] - base["psnr"]) < 0.1 and abs(cc_plain["ssim"] - base["ssim"]) < 0.01
    print(f"final training loss: plain {loss_plain:.4f}, with exposure {loss_exposed:.4f}; held-out cc_psnr: plain "
          f"{cc_plain['cc_psnr']:.2f}, with exposure {cc_exposed['cc_psnr']:.2f} (psnr {cc_plain['psnr']:.2f} / {cc_exposed['psnr']:.2f})")
    assert loss_exposed < loss_plain
    assert cc_exposed["cc_psnr"] >= cc_plain["cc_psnr"]

    # both checkpoints load; the one with exposure restores delta bit for bit
    loaded, _ = create_volumetric_model_from_saved_model(tmp_path / "plain" / "saved_models" / "model_final.pth",
                                                         create_voxel_grid_from_saved_info_dict, device=DEV)
    assert loaded.exposure is None and torch.equal(loaded.thre3d_repr.densities, plain.thre3d_repr.densities)
    loaded, _ = create_volumetric_model_from_saved_model(tmp_path / "exposed" / "saved_models" / "model_final.pth",
                                                         create_voxel_grid_from_saved_info_dict, device=DEV)
    assert torch.equal(loaded.exposure.delta, exposed.exposure.delta.detach()) and not loaded.exposure.delta.requires_grad
    assert torch.equal(loaded.thre3d_repr.densities, exposed.thre3d_repr.densities)


def test_trainer_takes_the_ssim_term_on_the_corrected_colours(tmp_path):
    from test_trainers_gpu import _sphere_model
    from thre3d_atom.data.datasets import InMemoryPosedImages
    from thre3d_atom.modules.trainers import train_sh_vox_grid_vol_mod_with_posed_images
    from thre3d_atom.modules.volumetric_model import VolumetricModel
    from thre3d_atom.thre3d_reprs.renderers import SHVoxGridRenderConfig, render_sh_voxel_grid
    from thre3d_atom.thre3d_reprs.voxels import VoxelGrid, VoxelSize
    from thre3d_atom.utils.imaging_utils import CameraBounds, CameraIntrinsics, pose_spherical

    torch.manual_seed(1)
    truth = _sphere_model(side=24, samples=96)
    intr = CameraIntrinsics(48, 48, 0.5 * 48 / np.tan(0.5 * 0.6911112))
    poses, images = [], []
    for i in range(4):
        pose = pose_spherical(90.0 * i, 30.0, 4.0311)
        poses.append(torch.cat([pose.rotation, pose.translation], dim=1))
        images.append(truth.render(pose, intr, perturb_sampled_points=False).colour.permute(2, 0, 1).cpu() * (0.7 + 0.2 * i))
    bounds = CameraBounds(1.8, 6.6)
    data = InMemoryPosedImages(torch.stack(images), torch.stack(poses), intr, bounds)
    g = torch.Generator().manual_seed(3)
    vg = VoxelGrid(torch.empty(24, 24, 24, 1).uniform_(-1, 1, generator=g), torch.empty(24, 24, 24, 3).uniform_(-1, 1, generator=g),
                   VoxelSize(0.125, 0.125, 0.125), density_preactivation=torch.nn.Identity(),
                   density_postactivation=torch.nn.Softplus(), expected_density_scale=100.0 / 3.0, tunable=True)
    vm = VolumetricModel(vg, render_sh_voxel_grid, SHVoxGridRenderConfig(96, bounds, white_bkgd=True), device=DEV)
    seen = []
    real = ops.exposure_apply

    def spy(colour, ids, delta):
        out = real(colour, ids, delta)
        seen.append(out.requires_grad and delta.requires_grad)
        return out

    import thre3d_atom.modules.trainers as trainers

    orig = trainers._ops.exposure_apply
    trainers._ops.exposure_apply = spy
    try:
        train_sh_vox_grid_vol_mod_with_posed_images(vm, data, tmp_path, random_initializer=lambda t: t, ray_batch_size=4096,
                                                    num_stages=1, num_iterations_per_stage=3, fast_debug_mode=True,
                                                    exposure_learning_rate=1e-2, ssim_weight=0.2, ssim_patch_size=32)
    finally:
        trainers._ops.exposure_apply = orig
    assert seen == [True, True, True]
    assert bool(torch.isfinite(vm.exposure.delta).all()) and bool(vm.exposure.delta.detach().any())
