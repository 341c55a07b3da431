"""tests/arena.py on CPU tensors: the layout it promises and the bite of its checks."""
import pytest
import torch

from arena import ALIGN, GUARD, TAIL, Arena

SIZES = [("a", 4 * 1499, torch.float32), ("b", 1, torch.uint8), ("c", 8 * 7, torch.int64), ("d", 513, torch.uint8),
         ("e", 4 * 1025, torch.int32)]


def _arena(pattern=0xFF):
    a = Arena("cpu", capacity=4 << 20)
    views = {n: a.carve(n, nbytes, dt, input=(n == "c")) for n, nbytes, dt in SIZES}
    a.fill(pattern)
    return a, views


def test_views_are_aligned_exact_and_typed():
    a, views = _arena()
    for n, nbytes, dt in SIZES:
        v = views[n]
        assert v.data_ptr() % ALIGN == 0
        assert v.dtype == dt and v.numel() * v.element_size() == nbytes
        assert a[n].data_ptr() == v.data_ptr()


def test_rear_band_starts_at_byte_nbytes_and_front_band_ends_at_the_view():
    a, views = _arena()
    for n, nbytes, _ in SIZES:
        rear, front = a.band(n, "rear"), a.band(n, "front")
        assert rear.data_ptr() == views[n].data_ptr() + nbytes          # (no rounding up)
        assert rear.numel() == GUARD
        assert front.numel() >= GUARD and front.data_ptr() + front.numel() == views[n].data_ptr()
    assert a.band("arena", "tail").numel() == TAIL
    # the bands and the buffers tile the arena without a hole: nothing between two buffers is unwatched
    order = [n for n, _, _ in SIZES]
    for prev, nxt in zip(order, order[1:]):
        assert a.band(prev, "rear").data_ptr() + GUARD == a.band(nxt, "front").data_ptr()
    assert a.band(order[-1], "rear").data_ptr() + GUARD == a.band("arena", "tail").data_ptr()


@pytest.mark.parametrize("pattern", [0xFF, 0x00])
def test_fill_poisons_outputs_and_bands_and_keeps_inputs(pattern):
    a = Arena("cpu", capacity=4 << 20)
    out = a.carve("out", 4 * 33, torch.float32)
    src = a.carve("src", 4 * 33, torch.float32, input=True)
    src.copy_(torch.arange(33.0))
    a.fill(pattern)
    assert a.check() == []
    assert torch.equal(src, torch.arange(33.0))
    assert a.poisoned("out") == 4 * 33
    if pattern == 0xFF:
        assert bool(torch.isnan(out).all())
        assert bool((out.view(torch.int32) == -1).all())
    else:
        assert not out.any()


@pytest.mark.parametrize("pattern", [0xFF, 0x00])
@pytest.mark.parametrize("name", ["a", "b", "d"])
@pytest.mark.parametrize("side", ["front", "rear"])
@pytest.mark.parametrize("last", [False, True])
def test_check_reports_one_dirty_byte_with_name_side_and_offset(pattern, name, side, last):
    a, _ = _arena(pattern)
    assert a.check() == []
    band = a.band(name, side)
    off = band.numel() - 1 if last else 0
    band[off] = 0x5A
    report = a.check()
    assert len(report) == 1, report
    assert report[0].startswith(f"{name}: {side} band dirty at offset {off}"), report
    assert ", 1 dirty bytes" in report[0]
    band[off] = pattern
    assert a.check() == []


def test_check_sees_the_element_right_behind_a_ragged_buffer():
    a, views = _arena()
    base = a.mem
    start = views["d"].data_ptr() - base.data_ptr()
    base[start + 513] = 0                       # what a 16-byte store over a 513-byte buffer would touch first
    base[start + 514] = 0
    assert a.check() == ["d: rear band dirty at offset 0, 2 dirty bytes of 65536"]


def test_tail_band_is_watched():
    a, _ = _arena()
    a.band("arena", "tail")[TAIL - 1] = 1
    assert a.check() == [f"arena: tail band dirty at offset {TAIL - 1}, 1 dirty bytes of {TAIL}"]


def test_unchanged_sees_one_bit():
    a, views = _arena()
    views["c"].copy_(torch.arange(7))
    a.snapshot()
    assert a.unchanged() == []
    views["c"][3] ^= 1 << 40
    report = a.unchanged()
    assert report == [f"c: input changed at byte {3 * 8 + 5}, 1 bytes differ"], report
    assert a.unchanged(exempt=("c",)) == []
    # a float input whose sign of zero flips is a change too
    b = Arena("cpu", capacity=4 << 20)
    z = b.carve("z", 16, torch.float32, input=True)
    b.fill(0xFF)
    z.zero_()
    b.snapshot()
    z[2] = -0.0
    assert b.unchanged() == ["z: input changed at byte 11, 1 bytes differ"]


def test_capacity_is_enforced():
    from arena import ArenaFull

    a = Arena("cpu", capacity=2 << 20)
    with pytest.raises(ArenaFull):
        a.carve("big", 2 << 20)
