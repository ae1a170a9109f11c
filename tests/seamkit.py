"""Inputs and verdicts for kernels at their 32-bit seams: offsets past 2 GiB and 4 GiB.

No kernel has to move much data to have large offsets.  The helpers here put a few units
of input at large addresses of an otherwise unwritten buffer, or let a few live frames of
a mostly-fill output fall on the large element numbers, and judge the result without an
expectation of full size.  The seam positions are parameters: tests/test_seamkit.py drives
every helper with seams of 2^15 and 2^16 against NumPy model kernels, one correct and the
others with one fault each (an offset truncated, sign-extended, the last work item above
the seam dropped, a store wrapped to the low addresses); tests/test_seams_gpu.py uses the
defaults, 2^31 and 2^32, on the device.  Buffers are NumPy arrays or torch tensors: the
helpers use only what both have (slices, comparisons, sums).

  * `places(unit, size)`               where units of `unit` bytes go in a buffer of `size` bytes;
  * `Sparse(buf, unit, places, rng)`   random units written there; `.compact()` -> (small NumPy
                                       buffer, translated index) for the NumPy references;
  * `Strided(buf, src0, stride, n, unit, rng)`   the same at src0 + k * stride;
  * `live_frames`, `dense_index`, `dense_verdict`   a dense output whose index is -1 except at the
                                       frame(-set)s that hold, precede or follow an output seam;
  * `periodic_verdict`                 an output that must repeat its first period (an odd prime
                                       number of rows or frames: no power of two is a whole number
                                       of periods, so a store that loses its high bits lands on
                                       the wrong phase).

Verdicts are guardkit's: (touched guard offsets, elements still poison, elements wrong)."""
import numpy as np

import guardkit
from guardkit import GUARD, POISON, Verdict

LOW, HIGH = 1 << 31, 1 << 32            # the seams of a byte offset
TAIL = 1 << 26                          # bytes of an input buffer behind its high seam
SIZE = HIGH + TAIL
STRIDE = (1 << 22) + 64                 # fixed stride: a multiple of 16 bytes, no power of two
OUT_ELEMS = (1 << 32) + (1 << 22)       # elements of the dense output view
CHUNK = 1 << 27                         # elements a verdict looks at in one go


def is_np(x):
    return isinstance(x, np.ndarray)


def _down(x, align):
    return x - x % align


def places(unit, size=SIZE, low=LOW, high=HIGH, align=4, odd=True):
    """Offsets of units of `unit` bytes in a buffer of `size` bytes whose seams are `low` and `high`:
    two low controls, a unit that straddles `low` and one that starts on it, units that end on, straddle
    and start on `high`, one at an odd address behind it (only with `odd`: for the entries that take byte
    addresses), one half way through the tail, one that ends 4 bytes outside the buffer, and -1.
    Mid-unit places are rounded down to `align`."""
    assert unit % align == 0 and size > high + 4 * unit + 64 and low > 4 * unit and high - low > 4 * unit
    half = _down(unit // 2, align) or align
    step = unit + (-unit) % 4
    p = [0, _down(unit + 36 + align - 1, align),
         low - half, low,
         high - unit, high - half, high]
    if odd:
        p.append(high + step + 4 * 3 + 1)
    p += [_down(high + (size - high) // 2, align), size - unit + 4, -1]
    return [int(x) for x in p]


def inside(p, unit, size):
    """Does a unit at `p` lie inside a buffer of `size` bytes?  (What the kernels ask of an index entry.)"""
    return 0 <= p <= size - unit


def _write(buf, lo, data):
    if is_np(buf):
        buf[lo:lo + data.size] = data
    else:
        import torch
        buf[lo:lo + data.size] = torch.from_numpy(data).to(buf.device)


def _read(buf, lo, hi):
    return buf[lo:hi].copy() if is_np(buf) else buf[lo:hi].cpu().numpy()


class Sparse:
    """Random units of `unit` bytes at `places` of the uint8 buffer `buf`; the rest of it stays as it was
    (uninitialised).  Units may overlap: `compact` reads back what the buffer holds in the end."""

    def __init__(self, buf, unit, at, rng):
        self.buf, self.unit, self.at = buf, unit, [int(p) for p in at]
        self.size = int(buf.shape[0])
        for p in self.at:
            if inside(p, unit, self.size):
                _write(buf, p, rng.integers(0, 256, unit, dtype=np.uint8))

    def index(self):
        return np.array(self.at, np.int64)

    def valid(self):
        """Positions in `at` of the units inside the buffer."""
        return [k for k, p in enumerate(self.at) if inside(p, self.unit, self.size)]

    def compact(self, head=8):
        """-> (small, index): the units back to back (from `head` on, at a stride that keeps each place's
        residue mod 4) in a NumPy buffer, and for every place the offset of its unit there.  -1 stays
        -1; a place whose unit does not lie inside the buffer becomes one that does not lie inside `small`."""
        stride = self.unit + (-self.unit) % 4 + 4
        small = np.zeros(head + len(self.at) * stride + 4, np.uint8)
        idx = np.empty(len(self.at), np.int64)
        for k, p in enumerate(self.at):
            if p < 0:
                idx[k] = -1
            elif not inside(p, self.unit, self.size):
                idx[k] = small.size - self.unit + 4
            else:
                o = head + k * stride + p % 4
                small[o:o + self.unit] = _read(self.buf, p, p + self.unit)
                idx[k] = o
        return small, idx


class Strided:
    """Random units of `unit` bytes at src0 + k * stride, k < n, written through a strided view."""

    def __init__(self, buf, src0, stride, n, unit, rng):
        assert src0 >= 0 and unit <= stride and src0 + (n - 1) * stride + unit <= buf.shape[0]
        self.buf, self.src0, self.stride, self.n, self.unit = buf, src0, stride, n, unit
        data = rng.integers(0, 256, (n, unit), dtype=np.uint8)
        if is_np(buf):
            np.lib.stride_tricks.as_strided(buf[src0:], (n, unit), (stride, 1))[:] = data
        else:
            import torch
            torch.as_strided(buf, (n, unit), (stride, 1), src0).copy_(torch.from_numpy(data).to(buf.device))

    def index(self):
        return self.src0 + np.arange(self.n, dtype=np.int64) * self.stride

    def crossing(self, seam):
        """The unit numbers that hold, precede and follow byte `seam` of the buffer."""
        k = (seam - self.src0) // self.stride
        return [j for j in (k - 1, k, k + 1) if 0 <= j < self.n]

    def compact(self):
        """-> (small, index): the units back to back, read back from the buffer."""
        if is_np(self.buf):
            v = np.lib.stride_tricks.as_strided(self.buf[self.src0:], (self.n, self.unit), (self.stride, 1)).copy()
        else:
            import torch
            v = torch.as_strided(self.buf, (self.n, self.unit), (self.stride, 1), self.src0).contiguous().cpu().numpy()
        return v.reshape(-1), np.arange(self.n, dtype=np.int64) * self.unit


# ---- outputs ----------------------------------------------------------------------------------------

def out_seams(item, nelem):
    """Element numbers of an output of `nelem` elements of `item` bytes at which an offset needs one bit
    more: byte offsets 2^31 .. 2^34, element numbers 2^31 and 2^32."""
    s = {b // item for b in (1 << 31, 1 << 32, 1 << 33, 1 << 34)} | {1 << 31, 1 << 32}
    return sorted(x for x in s if 0 < x < nelem)


def live_frames(frame_elems, nframes, seams):
    """The frame(-set)s of `frame_elems` output elements that hold, precede or follow each seam (an
    element number).  Every seam must fall INSIDE a frame, so that one straddles it."""
    live = set()
    for s in seams:
        assert s % frame_elems, "a frame boundary on seam {}: nothing straddles it".format(s)
        f = s // frame_elems
        assert 0 < f < nframes - 1, (s, frame_elems, nframes)
        live.update((f - 1, f, f + 1))
    return sorted(live)


def dense_index(nframes, nslot, live, sources):
    """int64 (nframes * nslot): -1 everywhere but at the live frame sets, whose slots take `sources` in turn.
    -> (index, {frame: positions in `sources` of its slots})."""
    idx = np.full(nframes * nslot, -1, np.int64)
    used, k = {}, 0
    for f in live:
        used[f] = [(k + s) % len(sources) for s in range(nslot)]
        idx[f * nslot:(f + 1) * nslot] = [sources[j] for j in used[f]]
        k += nslot
    return idx, used


def _ints(whole, item):
    """`whole` (int32 words) as signed integers of `item` bytes."""
    if is_np(whole):
        return whole.view({2: np.int16, 4: np.int32}[item])
    import torch
    return whole.view({2: torch.int16, 4: torch.int32}[item])


def _signed(pattern, item):
    return int(np.array([pattern & ((1 << 8 * item) - 1)], {2: np.uint16, 4: np.uint32}[item]).view({2: np.int16, 4: np.int32}[item])[0])


def _poison_count(x, first, item):
    """Elements of `x` (signed integers; element `first` of the allocation is x[0]) that hold the poison."""
    if item == 4:
        return int((x == _signed(POISON, 4)).sum())
    n = 0
    for parity, pat in ((0, POISON & 0xFFFF), (1, POISON >> 16)):
        n += int((x[(parity - first) % 2::2] == _signed(pat, 2)).sum())
    return n


def _nonpoison_offsets(x, first, item):
    """Positions in `x` that do not hold the poison."""
    if item == 4:
        bad = x != _signed(POISON, 4)
    else:
        bad = x != x                                    # all False, of x's kind
        for parity, pat in ((0, POISON & 0xFFFF), (1, POISON >> 16)):
            o = (parity - first) % 2
            bad[o::2] = x[o::2] != _signed(pat, 2)
    if is_np(x):
        return [int(i) for i in np.flatnonzero(bad)]
    import torch
    return [int(i) for i in torch.nonzero(bad).reshape(-1).cpu().numpy()]


def guards_touched(whole, lo, nelem, item):
    """Offsets (from the view's first element, as guardkit.Verdict.touched) of changed elements in the GUARD
    bytes before element `lo` of `whole` and behind element `lo + nelem`."""
    w = _ints(whole, item)
    g = GUARD // item
    assert lo >= g and lo + nelem + g <= w.shape[0], "the view leaves no guard"
    before = [i - g for i in _nonpoison_offsets(w[lo - g:lo], lo - g, item)]
    after = [i + nelem for i in _nonpoison_offsets(w[lo + nelem:lo + nelem + g], lo + nelem, item)]
    near = sorted(before[-guardkit.NEAREST:] + after[:guardkit.NEAREST], key=lambda off: -off if off < 0 else off - nelem + 1)
    return near[:guardkit.NEAREST]


def _bits(expected, item):
    e = np.ascontiguousarray(expected).reshape(-1)
    assert e.dtype.itemsize == item, (e.dtype, item)
    return e.view({2: np.int16, 4: np.int32}[item])


def _same(x, want):
    """Number of elements of `x` (device or NumPy) that differ from the NumPy array `want`."""
    if is_np(x):
        return int((x != want).sum())
    import torch
    return int((x != torch.from_numpy(want).to(x.device)).sum())


def dense_verdict(whole, lo, nelem, item, fill_bits, live, chunk=CHUNK):
    """A launch wrote elements [lo, lo + nelem) of `whole` (elements of `item` bytes).  `live`: list of
    (first element in the view, expected NumPy patterns).  Outside the live ranges every element must be
    `fill_bits`, inside them the expectation; no element of the view may still be poison and the guards
    must still be (the fill and the expectations hold no poison: the callers assert it).  Runs in pieces of `chunk` elements where the allocation lives."""
    w = _ints(whole, item)
    fill = _signed(fill_bits, item)
    live = sorted(((int(a), _bits(e, item)) for a, e in live), key=lambda t: t[0])
    wrong = poison = 0
    for a in range(0, nelem, chunk):
        b = min(nelem, a + chunk)
        x = w[lo + a:lo + b]
        poison += _poison_count(x, lo + a, item)
        wrong += int((x != fill).sum())
        for la, e in live:                      # what a live range adds to the count above is taken off again
            s, t = max(a, la), min(b, la + e.size)
            if s < t:
                wrong -= int((x[s - a:t - a] != fill).sum())
    end = 0
    for la, e in live:
        assert end <= la and la + e.size <= nelem, "live ranges overlap or leave the view"
        end = la + e.size
        wrong += _same(w[lo + la:lo + la + e.size], e)
    # (an element still poison is neither fill nor expected: it was counted as wrong too)
    return Verdict(guards_touched(whole, lo, nelem, item), poison, wrong - poison)


def periodic_verdict(whole, lo, nelem, item, first, chunk=CHUNK):
    """The view [lo, lo + nelem) must hold the NumPy patterns `first` (one period) over and over, the last
    repeat cut off; no poison inside, the guards untouched.  `first` (it holds no poison) goes to where the
    allocation lives once; every period is compared with it there, broadcast."""
    w = _ints(whole, item)
    first = _bits(first, item)
    P = first.size
    assert 0 < P <= nelem
    wrong = _same(w[lo:lo + P], first)
    if is_np(whole):
        head = first
    else:
        import torch
        head = torch.from_numpy(first).to(whole.device)
    per = max(1, chunk // P)
    poison = _poison_count(w[lo:lo + P], lo, item)
    for a in range(P, nelem, per * P):
        b = min(nelem, a + per * P)
        x = w[lo + a:lo + b]
        poison += _poison_count(x, lo + a, item)
        k = (b - a) // P
        if k:
            wrong += int((x[:k * P].reshape(k, P) != head.reshape(1, P)).sum())
        if (b - a) % P:
            wrong += int((x[k * P:] != head[:(b - a) % P]).sum())
    return Verdict(guards_touched(whole, lo, nelem, item), poison, wrong - poison)


def allocation(nbytes, device=None):
    """Poisoned int32 words for views of up to `nbytes` bytes with GUARD bytes either side, page-aligned;
    NumPy without `device`."""
    nwords = (2 * GUARD + nbytes + 3) // 4
    if device is None:
        block = np.empty(nwords * 4 + guardkit.PAGE, np.uint8)
        skip = -block.ctypes.data % guardkit.PAGE
        whole = block[skip:skip + nwords * 4].view(np.int32)
    else:
        import torch
        block = torch.empty(nwords + guardkit.PAGE // 4, dtype=torch.int32, device=device)
        skip = (-block.data_ptr() % guardkit.PAGE) // 4
        whole = block[skip:skip + nwords]
    guardkit.refill(whole)
    return whole


def view_of(whole, nelem, dtype, item):
    """(first element, view): `nelem` elements of `dtype` (`item` bytes each) GUARD bytes into `whole`."""
    lo = GUARD // item
    v = whole.view(dtype)[lo:lo + nelem]
    assert v.shape[0] == nelem, "the allocation is too small for this view"
    return lo, v
