"""Exact-size buffers between guard bands, for tests of the C ABI's buffer contract.

One `torch.uint8` tensor (the arena) is cut into buffers of exactly the byte count a caller is told to provide (include/voxe.h:
output element counts, voxe_*_scratch_bytes, voxe_workspace_bytes).  Every buffer starts on a 512-byte boundary, as torch's own
allocations do, and sits between two guard bands of GUARD bytes; the rear band starts at the very next byte after the buffer,
not after rounding up, so one element too far is one element into a band.  The arena ends in one further band of TAIL bytes, so
even a gross overrun stays in memory the test owns.

GUARD is a condition, not a measurement: several times the largest chunk any kernel moves per block (64 voxels x 49 channels x
4 B = 12.5 KB for the wide-texel passes).

    a = Arena(device)
    out = a.carve("out", n * 4, torch.float32)                # poisoned by fill()
    src = a.carve("src", n * 4, torch.float32, input=True)    # kept by fill(); snapshot() / unchanged() watch it
    a.fill(0xFF); src.copy_(...); a.snapshot()
    ... the call under test, then a synchronisation ...
    assert a.check() == [] and a.unchanged() == []

Works on CPU tensors too (tests/test_arena_host.py)."""
import torch

ALIGN = 512
GUARD = 64 << 10
TAIL = 1 << 20
DEFAULT_CAPACITY = 32 << 20


class ArenaFull(RuntimeError):
    pass


class Arena:
    def __init__(self, device="cpu", capacity=DEFAULT_CAPACITY):
        # (ALIGN spare bytes: a CPU allocation need not start on a 512-byte boundary)
        self.mem = torch.zeros(capacity + ALIGN, dtype=torch.uint8, device=device)
        self.base = self.mem.data_ptr()
        self.capacity = capacity
        self._end = 0                 # first byte behind the last rear band
        self._buffers = {}            # name -> (start, nbytes, input, view)
        self._bands = []              # (name, side, begin, end)
        self._tail = None
        self._band_mask = None
        self._snap = {}
        self.pattern = 0

    # ---- layout ----
    def carve(self, name, nbytes, dtype=torch.uint8, input=False):
        """a view of exactly `nbytes` on a 512-byte boundary with a band of >= GUARD bytes in front (it begins where the previous
        buffer's rear band ended) and one of GUARD bytes that starts at byte `nbytes`"""
        assert name not in self._buffers, name
        assert self._tail is None, "carve() after the arena was sealed by fill() / check()"
        item = torch.empty((), dtype=dtype).element_size()
        assert nbytes >= 0 and nbytes % item == 0, (name, nbytes, dtype)
        start = -(-(self.base + self._end + GUARD) // ALIGN) * ALIGN - self.base
        stop = start + nbytes
        if stop + GUARD + TAIL > self.capacity + ALIGN:
            raise ArenaFull(f"{name}: {nbytes} bytes do not fit an arena of {self.capacity}")
        self._bands.append((name, "front", self._end, start))
        self._bands.append((name, "rear", stop, stop + GUARD))
        self._end = stop + GUARD
        view = self.mem[start:stop].view(dtype)
        self._buffers[name] = (start, nbytes, bool(input), view)
        return view

    def __getitem__(self, name):
        return self._buffers[name][3]

    def names(self, input=None):
        return [k for k, v in self._buffers.items() if input is None or v[2] == input]

    def _seal(self):
        if self._tail is None:
            self._tail = ("arena", "tail", self._end, self._end + TAIL)
            self._bands.append(self._tail)
            mask = torch.zeros(self.mem.numel(), dtype=torch.bool, device=self.mem.device)
            for _, _, b, e in self._bands:
                mask[b:e] = True
            self._band_mask = mask

    def band(self, name, side):
        """the bytes of one guard band (a view: the host tests corrupt it on purpose)"""
        self._seal()
        for n, s, b, e in self._bands:
            if (n, s) == (name, side):
                return self.mem[b:e]
        raise KeyError((name, side))

    # ---- poison and checks ----
    def fill(self, pattern):
        """`pattern` (0xFF: every float a NaN, every integer -1; or 0x00) into every band and every buffer that is not an input"""
        self._seal()
        self.pattern = int(pattern)
        for _, _, b, e in self._bands:
            self.mem[b:e] = self.pattern
        for start, nbytes, is_input, _ in self._buffers.values():
            if not is_input:
                self.mem[start:start + nbytes] = self.pattern

    def check(self):
        """[] when every band still holds the pattern; else one line per dirty band: buffer, side, first dirty offset inside
        the band (for a front band also its distance in front of the buffer) and the number of dirty bytes"""
        self._seal()
        dirty = (self.mem != self.pattern) & self._band_mask
        if not bool(dirty.any()):
            return []
        report = []
        for name, side, b, e in self._bands:
            idx = torch.nonzero(dirty[b:e]).flatten()
            if idx.numel():
                first = int(idx[0])
                where = f" ({e - b - first} bytes in front of the buffer)" if side == "front" else ""
                report.append(f"{name}: {side} band dirty at offset {first}{where}, {idx.numel()} dirty bytes of {e - b}")
        return report

    def poisoned(self, name):
        """number of bytes of a buffer that still hold the fill pattern"""
        start, nbytes, _, _ = self._buffers[name]
        return int((self.mem[start:start + nbytes] == self.pattern).sum())

    def snapshot(self):
        self._snap = {k: v[3].clone() for k, v in self._buffers.items() if v[2]}

    def unchanged(self, exempt=()):
        """[] when every input buffer equals its snapshot bit for bit; else one line per changed buffer"""
        report = []
        for name, ref in self._snap.items():
            if name in exempt:
                continue
            now = self._buffers[name][3].view(torch.uint8)
            diff = torch.nonzero(now != ref.view(torch.uint8)).flatten()
            if diff.numel():
                report.append(f"{name}: input changed at byte {int(diff[0])}, {diff.numel()} bytes differ")
        return report
