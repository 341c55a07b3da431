"""What tests/test_buffer_contract_gpu.py runs every entry point of the C ABI through: one call (or one short chain of calls)
whose every pointer comes from tests/arena.py at exactly the documented size, run under two fill patterns.

A case is a function `case(k, ...)`: it declares its buffers on `k` (inp / out / inout / scratch), calls k.begin(), makes its
library calls through k.call() and records what it produced with k.bits() / k.pair() / k.tol().

    k.call()   after the call and a synchronisation: status as expected, every guard band clean (a), every input bit-identical (b)
    k.written  under the 0xFF fill no element of an output is left NaN / -1 (c), except where the caller says the value is NaN
    k.bits     run_contract() compares these bit for bit between the 0xFF and the 0x00 run (d, outputs free of atomics)
    k.pair     ... and these by relative L2 (d, outputs built with float atomics); k.tol holds them to a reference right away

run_short() / run_empty() run the same case with one size argument one byte short, or with the element count 0: the call must
answer VOXE_ERR_WORKSPACE / VOXE_OK and leave the WHOLE arena -- outputs, scratch, workspace, bands -- as it found it (e)."""
import numpy as np
import torch

from arena import Arena
from voxe_hip import abi

DEV = torch.device("cuda:0")


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


class Stop(Exception):
    """the guarded call of a short-size / empty run has been made and checked: the rest of the case does not run"""


class Buf:
    def __init__(self, t, name):
        self.t, self.name = t, name

    @property
    def ptr(self):
        return self.t.data_ptr()

    @property
    def nbytes(self):
        return self.t.numel() * self.t.element_size()

    def cpu(self):
        return self.t.detach().cpu().clone()


def P(b):
    return None if b is None else b.ptr


class K:
    def __init__(self, pattern, short=None, empty=False, capacity=None):
        self.a = Arena(DEV) if capacity is None else Arena(DEV, capacity)
        self.pattern, self.short, self.empty = pattern, short, empty
        self._loads, self._armed = [], None
        self.bits_out, self.pair_out = {}, {}

    # ---- buffers ----
    def inp(self, name, array):
        """a `const` argument: filled now, kept by fill(), watched by unchanged()"""
        t = torch.from_numpy(np.ascontiguousarray(array))
        v = self.a.carve(name, t.numel() * t.element_size(), t.dtype, input=True)
        v.copy_(t.reshape(-1))
        return Buf(v, name)

    def out(self, name, numel, dtype=torch.float32):
        """an output of exactly `numel` elements, poisoned by begin()"""
        return Buf(self.a.carve(name, int(numel) * torch.empty((), dtype=dtype).element_size(), dtype), name)

    def inout(self, name, array):
        """a documented in-place argument: loaded by begin() after the fill; only its bounds are checked"""
        t = torch.from_numpy(np.ascontiguousarray(array))
        v = self.a.carve(name, t.numel() * t.element_size(), t.dtype)
        self._loads.append((v, t.reshape(-1)))
        return Buf(v, name)

    def scratch(self, name, nbytes):
        """scratch / workspace of exactly `nbytes` bytes, poisoned by begin()"""
        return Buf(self.a.carve(name, int(nbytes), torch.uint8), name)

    def begin(self):
        self.a.fill(self.pattern)
        for v, t in self._loads:
            v.copy_(t)
        self.a.snapshot()
        torch.cuda.synchronize()

    def refill(self, *bufs):
        """poison outputs again between two calls of one case"""
        for b in bufs:
            b.t.view(torch.uint8).fill_(self.pattern)

    # ---- the arguments a short-size / empty run replaces ----
    def size(self, buf, tag, minimum=None):
        """the size argument that goes with `buf`: its exact size, or -- in the short run aimed at `tag` -- one byte less than the
        smallest size the header lets the call accept (`minimum`; None: the buffer's own, documented size)"""
        if self.short is not None and self.short == tag:
            self._armed = abi.ERR_WORKSPACE
            return (buf.nbytes if minimum is None else int(minimum)) - 1
        return buf.nbytes

    def count(self, n, tag="count"):
        """the element count R / N / B of the call: 0 in the empty run aimed at `tag`"""
        if self.empty and self.empty == tag:
            self._armed = abi.OK
            return 0
        return n

    # ---- the call ----
    def call(self, fn, *args, expect=abi.OK, exempt=()):
        guarded = self._armed
        snap = self.a.mem.clone() if guarded is not None else None
        status = fn(*args)
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:
            # a device fault: nothing else of this session may run on the card
            import pytest

            pytest.exit(f"device fault at the synchronisation after {fn.__name__}: {e}", returncode=3)
        if guarded is not None:
            assert status == guarded, (fn.__name__, status, guarded)
            dirty = torch.nonzero(self.a.mem != snap).flatten()
            assert dirty.numel() == 0, (f"{fn.__name__} returned {status} and still wrote {dirty.numel()} bytes, first at arena "
                                        f"offset {int(dirty[0])}", self.a.check())
            raise Stop()
        assert status == expect, (fn.__name__, status, expect)
        report = self.a.check()
        assert not report, (fn.__name__, report)
        report = self.a.unchanged(exempt)
        assert not report, (fn.__name__, report)
        return status

    # ---- what the call produced ----
    def written(self, buf, nan_ok=None, minus_one_ok=False):
        """(c): under the 0xFF fill, no element of an overwritten output still reads NaN (floats) / -1 (integers)"""
        if self.pattern != 0xFF:
            return
        t = buf.t
        if t.dtype.is_floating_point:
            left = torch.isnan(t)
            if nan_ok is not None:
                left = left & ~torch.as_tensor(np.asarray(nan_ok).reshape(-1), device=t.device)
            assert int(left.sum()) == 0, f"{buf.name}: {int(left.sum())} of {t.numel()} elements left NaN, first {int(torch.nonzero(left)[0])}"
        elif not minus_one_ok and t.dtype != torch.uint8:
            left = t == -1
            assert int(left.sum()) == 0, f"{buf.name}: {int(left.sum())} of {t.numel()} elements left -1, first {int(torch.nonzero(left)[0])}"

    def bits(self, buf, name=None, **kw):
        self.written(buf, **kw)
        self.bits_out[name or buf.name] = buf.cpu()

    def pair(self, buf, bound, name=None):
        self.written(buf)
        got = buf.cpu()
        assert bool(torch.isfinite(got).all()), f"{name or buf.name}: not finite"
        self.pair_out[name or buf.name] = (got, bound)

    def pair_abs(self, buf, where, atol, name=None):
        """compared between the two fills by max |difference| over the elements `where` (a bool array)"""
        got, where = buf.cpu(), np.asarray(where).reshape(-1)
        assert bool(torch.isfinite(got[torch.from_numpy(where)]).all()), f"{name or buf.name}: not finite"
        self.pair_out[name or buf.name] = (got, (where, atol))

    def tol(self, buf, ref, bound, name=None):
        """finite and within `bound` (relative L2) of the reference; also compared between the two fills at twice the bound"""
        self.pair(buf, 2 * bound, name)
        err = rel_l2(buf.cpu().numpy().reshape(-1), np.asarray(ref).reshape(-1))
        print(f"{name or buf.name}: rel-L2 {err:.2e} against the reference (bound {bound:.0e}, fill {self.pattern:#04x})")
        assert err < bound, (name or buf.name, err, bound)


def run_contract(case, *args, **kw):
    runs = []
    for pattern in (0xFF, 0x00):
        k = K(pattern)
        case(k, *args, **kw)
        runs.append(k)
    a, b = runs
    assert a.bits_out.keys() == b.bits_out.keys() and a.pair_out.keys() == b.pair_out.keys()
    assert a.bits_out or a.pair_out, "the case recorded no output"
    for name in a.bits_out:
        x, y = a.bits_out[name].view(torch.uint8), b.bits_out[name].view(torch.uint8)
        diff = torch.nonzero(x != y).flatten()
        assert diff.numel() == 0, (f"{name}: result depends on what the buffers held before the call: {diff.numel()} bytes differ "
                                   f"between the 0xFF and the 0x00 fill, first at byte {int(diff[0])}")
    for name in a.pair_out:
        (x, bound), (y, _) = a.pair_out[name], b.pair_out[name]
        if isinstance(bound, tuple):
            where, atol = bound
            err = float(np.abs(x.numpy().astype(np.float64) - y.numpy())[where].max(initial=0.0))
            assert where.sum() > 0 and err < atol, f"{name}: max |difference| {err:.2e} between the 0xFF and the 0x00 fill (bound {atol:.0e})"
            continue
        err = rel_l2(x.numpy(), y.numpy())
        assert err < bound, (f"{name}: rel-L2 {err:.2e} between the 0xFF and the 0x00 fill (bound {bound:.0e})")
    return runs


def run_short(case, tag, *args, **kw):
    k = K(0xFF, short=tag)
    try:
        case(k, *args, **kw)
    except Stop:
        return
    raise AssertionError(f"the case never used the size argument {tag!r}")


def run_empty(case, *args, tag="count", **kw):
    k = K(0xFF, empty=tag)
    try:
        case(k, *args, **kw)
    except Stop:
        return
    raise AssertionError(f"the case never used the count {tag!r}")
