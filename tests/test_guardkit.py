"""tests/guardkit.py names each fault it is there to find: planted in a NumPy allocation
(no GPU), a store before the output, one far behind it, a float4 never written and a wrong
value are each reported as that fault and as nothing else."""
import numpy as np
import pytest

import guardkit
from guardkit import GUARD, POISON, poisoned, verdict

N = 1000


def _decoded(dtype, delta):
    """A poisoned allocation whose view holds what a correct launch would have written."""
    whole, view = poisoned(N, dtype, delta)
    want = (np.arange(N) % 7 - 3).astype(np.float32)
    want = want if np.dtype(dtype) == np.float32 else want.astype(np.float16).view(np.uint16)
    view[:] = want
    return whole, view, want


def test_geometry():
    assert GUARD == 1 << 20 and GUARD % 4096 == 0 and GUARD == 4 * (2 * 16 * 256 * 32)
    f = np.array([POISON], np.uint32).view(np.float32)
    assert np.isnan(f[0])
    for delta in (0, 4, 12, 16, 4080):
        whole, view = poisoned(N, np.float32, delta)
        assert whole.ctypes.data % 4096 == 0
        assert view.ctypes.data - whole.ctypes.data == GUARD + delta and view.size == N
        assert whole.nbytes - (GUARD + delta + view.nbytes) >= GUARD
        assert (whole.view(np.uint32) == POISON).all()
        assert np.shares_memory(whole, view)
    whole, view = poisoned(N + 1, np.uint16, 16)               # a 16-bit output may end inside a word
    assert view.dtype == np.uint16 and view.size == N + 1 and whole.nbytes % 4 == 0


@pytest.mark.parametrize('dtype', [np.float32, np.uint16])
@pytest.mark.parametrize('delta', [0, 16, 4080])
def test_a_correct_launch_is_clean(dtype, delta):
    whole, view, want = _decoded(dtype, delta)
    v = verdict(whole, view, want)
    assert v == ([], 0, 0) and guardkit.clean(v) and guardkit.describe(v, N) == 'clean'


def test_untouched_output_is_all_poison():
    whole, view = poisoned(N, np.float32, 16)
    assert verdict(whole, view, np.zeros(N, np.float32)) == ([], N, 0)
    view[:] = 1.0
    guardkit.refill(whole)
    assert verdict(whole, view, np.zeros(N, np.float32)) == ([], N, 0)


@pytest.mark.parametrize('dtype', [np.float32, np.uint16])
def test_store_four_bytes_before_the_view(dtype):
    whole, view, want = _decoded(dtype, 16)
    whole.view(np.uint8)[GUARD + 16 - 4:GUARD + 16].view(np.float32)[0] = 1.0
    v = verdict(whole, view, want)
    # (a float32 1.0 is 0x3F800000: both halves differ from the poison's)
    assert v == ([-1] if dtype == np.float32 else [-1, -2], 0, 0)
    assert 'OUTSIDE' in guardkit.describe(v, N) and not guardkit.clean(v)


@pytest.mark.parametrize('dtype', [np.float32, np.uint16])
def test_store_900_kib_after_the_view(dtype):
    whole, view, want = _decoded(dtype, 4080)
    item = np.dtype(dtype).itemsize
    at = GUARD + 4080 + view.nbytes + 900 * 1024
    whole.view(np.uint8)[at:at + item].view(dtype)[0] = 3
    v = verdict(whole, view, want)
    assert v == ([N + 900 * 1024 // item], 0, 0)


def test_nearest_guard_elements_come_first():
    whole, view, want = _decoded(np.float32, 0)
    w = whole.view(np.uint8)
    for off in (-400, -3, N + 1, N + 70):
        w[GUARD + 4 * off:GUARD + 4 * off + 4] = 0
    assert verdict(whole, view, want).touched == [N + 1, -3, N + 70, -400]


def test_one_float4_left_unwritten():
    whole, view, want = _decoded(np.float32, 16)
    view.view(np.uint32)[500:504] = POISON
    v = verdict(whole, view, want)
    assert v == ([], 4, 0) and 'NEVER stored' in guardkit.describe(v, N)
    whole, view, want = _decoded(np.uint16, 16)                 # 16 bytes of 16-bit elements
    whole.view(np.uint8)[GUARD + 16 + 1000:GUARD + 16 + 1016].view(np.uint32)[:] = POISON
    assert verdict(whole, view, want) == ([], 8, 0)


@pytest.mark.parametrize('dtype', [np.float32, np.uint16])
def test_one_wrong_value(dtype):
    whole, view, want = _decoded(dtype, 0)
    view[N - 1] = view[N - 1] + 1
    v = verdict(whole, view, want)
    assert v == ([], 0, 1) and 'WRONG' in guardkit.describe(v, N)


def test_faults_are_told_apart_when_they_come_together():
    whole, view, want = _decoded(np.float32, 0)
    view[0] = 99.0
    view.view(np.uint32)[8:12] = POISON
    whole.view(np.uint32)[GUARD // 4 + N] = 0
    assert verdict(whole, view, want) == ([N], 4, 1)


def test_poison_detector():
    assert guardkit.contains_poison(np.array([1, POISON], np.uint32))
    assert guardkit.contains_poison(np.array([0x7FA5], np.uint16)) and guardkit.contains_poison(np.array([0xA5A5], np.uint16))
    assert not guardkit.contains_poison(np.array([-2.5, 1.5, 3.316505], np.float32))
