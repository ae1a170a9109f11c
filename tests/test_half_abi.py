"""16-bit output types, host side of the C ABI (no GPU): the converted level
tables, the parameter check readers plan with, the parameter block.

Expected values, no tolerance: the 16-bit pattern of the float32 level,
converted by ``ndarray.astype(float16)`` / ``Tensor.to(bfloat16)`` on the CPU
(both round to nearest even)."""
import ctypes

import numpy as np
import pytest

import test_kernels_gpu as tk      # (COMBOS / CODERS only: nothing there touches the GPU at import)


def half_bits(x, out_type):
    """float32 array -> uint16 patterns of float16 (1) / bfloat16 (2)."""
    import torch
    x = np.ascontiguousarray(x, dtype=np.float32)
    if out_type == 1:
        with np.errstate(over='ignore'):
            return x.astype(np.float16).view(np.uint16)
    return torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def test_reference_roundings_are_the_ones_the_issue_lists():
    x = np.array([3.3359, 1 / 2.95, (255 - 127.5) / 35.5], np.float32)
    assert list(half_bits(x, 1)) == [0x42AC, 0x356C, 0x432F]
    assert list(half_bits(x, 2)) == [0x4055, 0x3EAE, 0x4066]


@pytest.mark.parametrize('coder,bps', [(0, 1), (0, 2), (0, 4), (0, 8), (1, 1), (1, 2), (2, 4), (2, 8)])
def test_levels_in_the_output_types(coder, bps):
    from baseband_amd import _lib
    f32 = _lib.get_levels(coder, bps)
    same = _lib.levels_as(coder, bps, _lib.OUT_F32)
    assert same.dtype == np.float32 and np.array_equal(same.view(np.uint32), f32.view(np.uint32))
    for out_type in (_lib.OUT_F16, _lib.OUT_BF16):
        got = _lib.levels_as(coder, bps, out_type)
        assert got.dtype == np.uint16 and got.shape == (1 << bps,)
        assert np.array_equal(got, half_bits(f32, out_type)), (coder, bps, out_type)
    if coder == _lib.CODER_INT:                 # small integers are exact in both types
        for out_type, dt in ((_lib.OUT_F16, np.float16),):
            assert np.array_equal(_lib.levels_as(coder, bps, out_type).view(dt).astype(np.float32), f32)


def test_levels_as_error_codes():
    from baseband_amd import _lib
    buf = np.empty(256, np.uint16)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert _lib.lib.bb_get_levels_as(0, 2, 3, p, 256) == _lib.BB_EINVAL
    assert _lib.lib.bb_get_levels_as(0, 2, -1, p, 256) == _lib.BB_EINVAL
    assert _lib.lib.bb_get_levels_as(_lib.CODER_MARK5B, 4, _lib.OUT_F16, p, 256) == _lib.BB_ENOTSUP
    assert _lib.lib.bb_get_levels_as(0, 8, _lib.OUT_BF16, p, 4) == _lib.BB_ERANGE
    assert _lib.lib.bb_get_levels_as(0, 8, _lib.OUT_BF16, None, 256) == _lib.BB_EINVAL


def _params(coder, bps, chunk, nslot, payload, out_type):
    from baseband_amd import _lib
    p = _lib.DecodeParams()
    p.coder, p.bps, p.chunk, p.nslot, p.payload_nbytes, p.out_type = coder, bps, chunk, nslot, payload, out_type
    return p


@pytest.mark.parametrize('coder,bps', tk.COMBOS)
def test_out_check_takes_every_coder_in_every_type(coder, bps):
    from baseband_amd import _lib
    for out_type in (0, 1, 2):
        for chunk, nslot in ((1, 1), (4, 8)):
            p = _params(tk.CODERS[coder], bps, chunk, nslot, 8000, out_type)
            assert _lib.lib.bb_decode_out_check(ctypes.byref(p)) == _lib.BB_OK, (out_type, chunk, nslot)
    p = _params(tk.CODERS[coder], bps, 1, 1, 8000, 3)
    assert _lib.lib.bb_decode_out_check(ctypes.byref(p)) == _lib.BB_EINVAL
    p = _params(tk.CODERS[coder], bps, 4, 8, 8000, -1)
    assert _lib.lib.bb_decode_out_check(ctypes.byref(p)) == _lib.BB_EINVAL


def test_out_check_answers_as_the_float32_argument_checks_do():
    """What bb_decode_frames answers for these parameter blocks (pinned on the GPU
    by tests/test_kernels_gpu.py::test_abi_argument_errors and the select check of
    tests/test_abi.py), asked without a device, for every output type."""
    from baseband_amd import _lib, kernels
    import torch
    ask = lambda *a: _lib.lib.bb_decode_out_check(ctypes.byref(_params(*a)))
    for t in (0, 1, 2):
        assert ask(_lib.CODER_MARK5B, 4, 1, 1, 64, t) == _lib.BB_ENOTSUP       # no such coder / width
        assert ask(_lib.CODER_VDIF, 3, 1, 1, 64, t) == _lib.BB_ENOTSUP
        assert ask(_lib.CODER_INT, 2, 1, 1, 64, t) == _lib.BB_ENOTSUP
        assert ask(0, 2, 1, 1, 62, t) == _lib.BB_EINVAL                        # payload not whole dwords
        assert ask(0, 2, 1, 1, 0, t) == _lib.BB_EINVAL
        assert ask(0, 2, 0, 1, 64, t) == _lib.BB_EINVAL
        assert ask(0, 2, 1, 0, 64, t) == _lib.BB_EINVAL
        assert ask(0, 2, 24, 2, 8000, t) == _lib.BB_ENOTSUP                    # chunk not a power of two
        assert ask(0, 2, 24, 1, 8000, t) == _lib.BB_OK                         # ... matters with thread slots only
        assert ask(0, 8, 64, 2, 96, t) == _lib.BB_EINVAL                       # payload is not whole rows
        assert ask(0, 2, 4, 3, 640, t) == _lib.BB_OK
    assert _lib.lib.bb_decode_out_check(None) == _lib.BB_EINVAL
    # more thread slots than the 16-bit interleave kernel stages: float32 takes them
    assert ask(0, 2, 4, 4096, 640, 0) == _lib.BB_OK
    assert ask(0, 2, 4, 4096, 640, 1) == _lib.BB_ENOTSUP
    assert ask(0, 2, 4, 2048, 640, 2) == _lib.BB_OK
    assert kernels.out_supported(0, 2, 4, 8, 8000, torch.float16)
    assert kernels.out_supported(0, 2, 4, 8, 8000, torch.bfloat16)
    assert not kernels.out_supported(0, 2, 4, 4096, 640, torch.float16)


def test_parameter_block_carries_the_output_type():
    from baseband_amd import _lib
    assert ctypes.sizeof(_lib.DecodeParams) == 56
    assert _lib.DecodeParams.out_type.offset == 52 and _lib.DecodeParams.out_type.size == 4
    assert _lib.DecodeParams().out_type == 0
    assert (_lib.OUT_F32, _lib.OUT_F16, _lib.OUT_BF16) == (0, 1, 2)
    assert _lib.Mark4DecodeParams().out_type == 0 and _lib.Mark4DecodeParams.out_type.offset == 4
    import torch
    assert _lib.out_type_of(torch.float16) == _lib.OUT_F16 and _lib.out_type_of(torch.complex32) == _lib.OUT_F16
    assert _lib.out_type_of(torch.bfloat16) == _lib.OUT_BF16 and _lib.out_type_of(torch.float64) is None
