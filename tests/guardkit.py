"""Poisoned, guarded outputs for the decode kernels.

`poisoned(nelem, dtype, delta_bytes)` gives an allocation filled with a poison pattern and
a view of `nelem` elements inside it, GUARD bytes from either end, whose base is as
aligned as `delta_bytes` says and no more (the allocation itself starts on a 4096-byte
boundary).  After a launch into the view, `verdict(whole, view, expected_bits)` tells the
three ways a decode can be wrong apart:

  * a store OUTSIDE the output   -> offsets of the guard elements that no longer hold poison,
  * an element NEVER stored      -> count of output elements that still hold poison,
  * a WRONG value                -> count of output elements that hold neither.

With a torch dtype the allocation is a device tensor and the comparison runs on the
device; with a NumPy dtype everything is NumPy (tests/test_guardkit.py plants the faults).

GUARD is 1 MiB: a multiple of 4096, and four times the output of the largest work item
(256 KiB: the 1-bit byte-table item of 2 waves x 16 tiles x 256 B, 32 bytes out per byte
in), so an item that lands one whole item early or late is still inside the guard.
POISON, 0x7FA5A5A5 per 32 bits, is a NaN that no level table, int8 value or test fill
value produces (its 16-bit halves 0xA5A5 / 0x7FA5 neither; tests/test_launch_expect.py
asserts both for every expected array)."""
import collections

import numpy as np

GUARD = 1 << 20
PAGE = 4096
POISON = 0x7FA5A5A5
NEAREST = 32                        # touched guard elements reported (the nearest ones)
DEVICE = 'cuda'                     # where a torch dtype's allocation lives

Verdict = collections.namedtuple('Verdict', 'touched poison_left wrong')
Verdict.__doc__ = """touched: offsets (in elements, from the view's first element: -1 is the one just before
it, view size the one just after) of guard elements that changed, nearest to the view first, at most NEAREST;
poison_left: output elements still holding poison; wrong: output elements holding something else than expected."""


def clean(v):
    return not v.touched and v.poison_left == 0 and v.wrong == 0


def describe(v, nelem):
    """One line for a failure message: which fault, and where."""
    parts = []
    if v.touched:
        parts.append("stores OUTSIDE the output at element offsets {} (output is [0, {}))".format(v.touched, nelem))
    if v.poison_left:
        parts.append("{} output elements NEVER stored".format(v.poison_left))
    if v.wrong:
        parts.append("{} output elements WRONG".format(v.wrong))
    return '; '.join(parts) or 'clean'


def _is_torch(dtype):
    return not isinstance(dtype, (np.dtype, type))


def poison_words(nwords):
    return np.full(nwords, POISON, np.uint32)


def contains_poison(expected_bits):
    """Does an expected array (float32 / uint32 / uint16 patterns) hold the poison, or one of its halves?"""
    e = np.ascontiguousarray(expected_bits)
    if e.dtype.itemsize == 4:
        return bool((e.view(np.uint32) == POISON).any())
    e = e.view(np.uint16)
    return bool(((e == (POISON & 0xFFFF)) | (e == (POISON >> 16))).any())


def poisoned(nelem, dtype, delta_bytes=0):
    """-> (whole, view).  `whole`: int32 words, all POISON, starting on a PAGE boundary; `view`: `nelem`
    elements of `dtype` starting GUARD + delta_bytes bytes into it, with at least GUARD bytes behind."""
    if _is_torch(dtype):
        import torch
        item = torch.empty(0, dtype=dtype).element_size()
    else:
        item = np.dtype(dtype).itemsize
    assert delta_bytes >= 0 and delta_bytes % item == 0, delta_bytes
    nbytes = GUARD + delta_bytes + nelem * item + GUARD
    nwords = (nbytes + 3) // 4
    if _is_torch(dtype):
        block = torch.empty(nwords + PAGE // 4, dtype=torch.int32, device=DEVICE)
        skip = (-block.data_ptr() % PAGE) // 4
        whole = block[skip:skip + nwords]
        refill(whole)
        lo = (GUARD + delta_bytes) // item
        view = whole.view(dtype)[lo:lo + nelem]
        assert whole.data_ptr() % PAGE == 0 and view.data_ptr() == whole.data_ptr() + GUARD + delta_bytes
    else:
        block = np.empty(nwords * 4 + PAGE, np.uint8)
        skip = -block.ctypes.data % PAGE
        whole = block[skip:skip + nwords * 4].view(np.int32)
        refill(whole)
        view = whole.view(np.uint8)[GUARD + delta_bytes:GUARD + delta_bytes + nelem * item].view(dtype)
    return whole, view


def refill(whole):
    """Poison every word of `whole` again (before every launch into a view of it)."""
    if isinstance(whole, np.ndarray):
        whole.view(np.uint32)[:] = POISON
    else:
        whole.fill_(POISON)


def verdict(whole, view, expected_bits):
    """Compare what a launch left in `whole` (from `poisoned`; `view` is the output inside it) with
    `expected_bits` (NumPy, the view's elements as float32 or as unsigned patterns) -> Verdict."""
    exp = np.ascontiguousarray(expected_bits).reshape(-1)
    on_cpu = isinstance(whole, np.ndarray)
    item = view.itemsize if on_cpu else view.element_size()
    assert exp.dtype.itemsize == item and exp.size == (view.size if on_cpu else view.numel()), (exp.dtype, exp.size)
    n = exp.size
    # everything as signed integers of the element's size (torch compares those on the device)
    idt = {2: np.int16, 4: np.int32}[item]
    exp = exp.view(idt)
    if on_cpu:
        pat = poison_words(whole.shape[0]).view(idt)
        w = whole.view(idt)
        lo = (view.ctypes.data - whole.ctypes.data) // item
        where = np.flatnonzero
    else:
        import torch
        tdt = {2: torch.int16, 4: torch.int32}[item]
        w = whole.view(tdt)
        lo = (view.data_ptr() - whole.data_ptr()) // item
        # (the pattern is made on the device: one word, repeated)
        pat = torch.from_numpy(poison_words(1).view(idt)).to(whole.device).repeat(whole.shape[0])
        exp = torch.from_numpy(exp).to(whole.device)

        def where(mask):
            return torch.nonzero(mask).reshape(-1).cpu().numpy()
    changed = w != pat
    got, still = w[lo:lo + n], ~changed[lo:lo + n]
    poison_left = int(still.sum())
    wrong = int(((got != exp) & ~still).sum())
    before = where(changed[:lo]) - lo                       # -1 = the element just before the view
    after = where(changed[lo + n:]) + n                     # n = the element just after it
    near = sorted([int(x) for x in before[-NEAREST:]] + [int(x) for x in after[:NEAREST]],
                  key=lambda off: -off if off < 0 else off - n + 1)
    return Verdict(near[:NEAREST], poison_left, wrong)
