"""The buffer contract of voxe_vq_assign and voxe_vq_accumulate (include/voxe.h), through the guard-band / poison helpers of
tests/contract.py and tests/arena.py: every pointer comes from the arena at exactly the documented element count, between two
guard bands; nothing outside index, dist, code_norm, sum_wx and sum_w is written, the inputs stay bit-identical, every output
element is written, the result does not depend on what the buffers held, dist == NULL is accepted, N == 0 launches nothing and
every limit of the header returns its error code with the whole arena untouched."""
import numpy as np
import pytest
import torch

import vq_ref as R
from contract import DEV, K, P, Stop, run_contract, run_empty
from voxe_hip import abi

pytestmark = pytest.mark.gpu

F32, I32 = torch.float32, torch.int32


def _lib():
    from voxe_hip.runtime import lib

    return lib()


def _stream():
    from voxe_hip.runtime import stream_ptr

    return stream_ptr(DEV)


def _data(N, Kc, F, seed=0):
    rng = np.random.default_rng([N, Kc, F, seed])
    return (rng.uniform(-1, 1, (N, F)).astype(np.float32), rng.uniform(-1, 1, (Kc, F)).astype(np.float32),
            rng.uniform(0, 1, N).astype(np.float32), rng.integers(0, Kc, N).astype(np.int32))


def assign_case(k, N, Kc, F, with_dist, bad=None, status=None):
    L, st = _lib(), _stream()
    x, c, _, _ = _data(N, Kc, F)
    px, pc = k.inp("points", x), k.inp("codebook", c)
    norm, idx = k.out("code_norm", Kc), k.out("index", N, I32)
    dist = k.out("dist", N) if with_dist else None
    k.begin()
    n, f, kc = bad or (k.count(N), F, Kc)
    if status is not None:
        k._armed = status      # the refused call: its status, and the whole arena as it was
    k.call(L.voxe_vq_assign, px.ptr, n, f, pc.ptr, kc, norm.ptr, idx.ptr, P(dist), st)
    k.bits(norm)
    k.bits(idx)
    assert np.array_equal(norm.cpu().numpy(), R.code_norm32(c))
    got = idx.cpu().numpy()
    assert got.min() >= 0 and got.max() < Kc and float((R.gap(x, c, got) / R.slack(x, c)).max()) <= 1.0
    if with_dist:
        k.bits(dist)
        assert np.array_equal(dist.cpu().numpy(), R.dist32(x, c, got))


def accumulate_case(k, N, Kc, F, merge, bad=None, status=None):
    L, st = _lib(), _stream()
    x, _, w, index = _data(N, Kc, F)
    px, pw, pi = k.inp("points", x), k.inp("weights", w), k.inp("index", np.sort(index) if merge == 2 else index)
    swx, sw = k.inout("sum_wx", np.zeros(Kc * F, np.int64)), k.inout("sum_w", np.zeros(Kc, np.int64))
    k.begin()
    n, f, kc = bad or (k.count(N), F, Kc)
    if status is not None:
        k._armed = status
    assert L.voxe_vq_debug_merge(merge) == abi.OK
    try:
        k.call(L.voxe_vq_accumulate, px.ptr, pw.ptr, pi.ptr, n, f, kc, swx.ptr, sw.ptr, st)
    finally:
        L.voxe_vq_debug_merge(0)
    k.bits(swx, minus_one_ok=True)
    k.bits(sw, minus_one_ok=True)
    want_wx, want_w = R.accumulate(x, w, pi.cpu().numpy(), Kc)
    assert np.array_equal(swx.cpu().numpy().reshape(Kc, F), want_wx) and np.array_equal(sw.cpu().numpy(), want_w)


@pytest.mark.parametrize("N,Kc,F", [(257, 129, 27), (1000, 33, 3), (31, 300, 64), (1, 1, 1)])
@pytest.mark.parametrize("with_dist", [True, False])
def test_assign_contract(N, Kc, F, with_dist):
    run_contract(assign_case, N, Kc, F, with_dist)


@pytest.mark.parametrize("N,Kc,F", [(257, 129, 27), (1000, 3, 12), (63, 300, 64)])
@pytest.mark.parametrize("merge", [1, 2])
def test_accumulate_contract(N, Kc, F, merge):
    run_contract(accumulate_case, N, Kc, F, merge)


def test_no_points_launch_nothing():
    run_empty(assign_case, 257, 33, 12, True)
    run_empty(accumulate_case, 257, 33, 12, 2)


LIMITS = [(-1, 12, 33), (1 << 31, 12, 33), (257, 0, 33), (257, 65, 33), (257, 12, 0), (257, 12, 65537)]


@pytest.mark.parametrize("bad", LIMITS)
def test_every_limit_returns_bad_shape_and_touches_nothing(bad):
    for case, extra in ((assign_case, True), (accumulate_case, 1)):
        with pytest.raises(Stop):
            case(K(0xFF), 257, 33, 12, extra, bad=bad, status=abi.ERR_BAD_SHAPE)


def test_wrapper_refuses_an_index_out_of_range_before_the_launch():
    from voxe_hip import ops
    from voxe_hip.runtime import VoxeError

    x, _, w, index = _data(100, 7, 3)
    t = lambda a: torch.from_numpy(a).to(DEV)      # noqa: E731
    swx, sw = torch.zeros((7, 3), dtype=torch.int64, device=DEV), torch.zeros(7, dtype=torch.int64, device=DEV)
    for bad in (7, -1):
        index[50] = bad
        with pytest.raises(VoxeError, match="status -2"):
            ops.vq_accumulate_(t(x), t(w), t(index), swx, sw)
        assert int(swx.abs().sum()) == 0 and int(sw.sum()) == 0
        # the library itself skips such a point and stays inside the sums
        ops.vq_accumulate_(t(x), t(w), t(index), swx, sw, check_index=False)
        keep = np.arange(100) != 50
        want_wx, want_w = R.accumulate(x[keep], w[keep], index[keep], 7)
        assert np.array_equal(swx.cpu().numpy(), want_wx) and np.array_equal(sw.cpu().numpy(), want_w)
        swx.zero_()
        sw.zero_()
