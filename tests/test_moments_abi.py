"""bb_i8_moments_check: what the parameters alone decide, without a device -- every refusal,
the order of the checks, and the parameter block against the header."""
import ctypes
import os
import re

from conftest import ROOT

CF, TF, ROWS, MKBF = 0, 1, 2, 3


def ask(layout, npol, nchan, ncomp, ntime, t_lo=0, t_hi=None, bin_rows=1, src0=0, src_stride=0):
    from baseband_amd import _lib
    return _lib.i8_moments_check(layout, npol, nchan, ncomp, ntime, t_lo, ntime if t_hi is None else t_hi,
                                 bin_rows, src0, src_stride)


def test_layout_numbers_match_the_header():
    from baseband_amd import _lib
    with open(os.path.join(ROOT, 'include', 'bbdecode.h')) as f:
        text = f.read()
    for name, value in (('GUPPI_CF', CF), ('GUPPI_TF', TF), ('ROWS', ROWS), ('MKBF', MKBF)):
        assert int(re.search(r'BB_MOMENTS_%s\s*=\s*(\d+)' % name, text).group(1)) == value == getattr(_lib, 'MOMENTS_' + name)
    # its own enum: the layouts of bb_decode_i8_tiled keep their numbers
    assert (_lib.LAYOUT_GUPPI_CF, _lib.LAYOUT_MKBF, _lib.LAYOUT_GUPPI_TF) == (0, 1, 2)


def test_struct_size_against_the_header():
    from baseband_amd import _lib
    with open(os.path.join(ROOT, 'include', 'bbdecode.h')) as f:
        text = f.read()
    body = re.search(r'typedef struct bb_moments_params \{(.*?)\} bb_moments_params;', text, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    size = {'int32_t': 4, 'uint64_t': 8, 'int64_t': 8}
    total, names = 0, []
    for kind, fields in re.findall(r'\b(int32_t|uint64_t|int64_t)\s+([^;]+);', body):
        for name in fields.split(','):
            names.append(name.strip())
            total += size[kind]
    assert names == [n for n, _ in _lib.MomentsParams._fields_]
    assert total == ctypes.sizeof(_lib.MomentsParams) == 80


def test_geometries_the_kernel_takes():
    from baseband_amd import _lib
    ok = _lib.BB_OK
    for npol in (1, 2):
        for nchan in (1, 3, 64, 65):
            assert ask(CF, npol, nchan, 2, 96) == ok
            assert ask(CF, npol, nchan, 2, 1000) == ok
    for nchan in (1, 8, 65, 4100):
        assert ask(TF, 2, nchan, 2, 96) == ok
    for npol, nchan, ncomp in ((1, 1, 1), (1, 1, 2), (2, 1, 1), (2, 1, 2), (1, 2, 2), (2, 2, 2), (2, 3, 2), (2, 65, 2),
                               (2, 4097, 2), (1, 4, 1), (3, 4, 2)):
        assert ask(ROWS, npol, nchan, ncomp, 1001) == ok, (npol, nchan, ncomp)
    assert ask(CF, 2, 4, 2, 96, 3, 91, 7, 4096, 1 << 20) == ok
    assert ask(CF, 2, 4, 2, 96, 5, 5) == ok                    # nothing asked for is not an error


def test_refusals():
    from baseband_amd import _lib
    inval, notsup = _lib.BB_EINVAL, _lib.BB_ENOTSUP
    assert _lib.lib.bb_i8_moments_check(None) == inval
    # heaps are not taken; a layout nobody knows is nonsense
    assert ask(MKBF, 2, 4, 2, 256) == notsup
    assert ask(4, 2, 4, 2, 256) == inval
    assert ask(-1, 2, 4, 2, 256) == inval
    # nonsense
    assert ask(CF, 0, 4, 2, 96) == inval
    assert ask(CF, 2, 0, 2, 96) == inval
    assert ask(CF, 2, 4, 3, 96) == inval
    assert ask(CF, 2, 4, 0, 96) == inval
    assert ask(CF, 2, 4, 2, 0, 0, 0) == inval
    assert ask(CF, 2, 4, 2, 96, 0, 97) == inval                # t_hi > ntime
    assert ask(CF, 2, 4, 2, 96, 50, 49) == inval               # t_lo > t_hi
    assert ask(CF, 2, 4, 2, 96, bin_rows=0) == inval
    assert ask(CF, 2, 4, 2, 96, src0=-4) == inval
    assert ask(CF, 2, 4, 2, 96, src_stride=-4) == inval
    # geometries
    assert ask(CF, 3, 4, 2, 96) == notsup                      # npol = 3
    assert ask(TF, 3, 4, 2, 96) == notsup
    assert ask(TF, 1, 4, 2, 96) == notsup                      # time first is two polarisations
    assert ask(CF, 2, 4, 1, 96) == notsup                      # real GUPPI samples
    assert ask(TF, 2, 4, 1, 96) == notsup
    assert ask(ROWS, 3, 1, 2, 96) == notsup                    # R = 6
    assert ask(ROWS, 1, 3, 2, 96) == notsup
    assert ask(ROWS, 1, 3, 1, 96) == notsup                    # R = 3
    assert ask(ROWS, 1, 5, 2, 96) == notsup                    # R = 10
    assert ask(ROWS, 2, (1 << 20) + 4, 2, 96) == notsup        # more channels than the kernel numbers
    assert ask(ROWS, 4, 1 << 20, 2, 96) == notsup              # R = 2^23: a row wider than BB_MOMENTS_MAX_ROW
    assert ask(ROWS, 2, 1 << 20, 2, 96) == _lib.BB_OK
    # alignment
    assert ask(CF, 2, 4, 2, 96, src0=2) == notsup
    assert ask(CF, 2, 4, 2, 96, src0=4098) == notsup
    assert ask(CF, 2, 4, 2, 96, src_stride=6) == notsup
    assert ask(ROWS, 2, 2, 2, 96, src0=1) == notsup
    assert ask(CF, 1, 4, 2, 97) == notsup                      # channel pitch 97 * 2 bytes
    assert ask(CF, 1, 4, 2, 98) == _lib.BB_OK
    assert ask(CF, 2, 4, 2, 97) == _lib.BB_OK                  # pitch 97 * 4


def test_order_of_the_checks():
    """layout, then nonsense, then geometry, then alignment: the first that fails answers."""
    from baseband_amd import _lib
    inval, notsup = _lib.BB_EINVAL, _lib.BB_ENOTSUP
    assert ask(MKBF, 0, 0, 7, 0, 5, 3, 0, -1, -1) == notsup    # heaps, whatever else is wrong
    assert ask(9, 3, 4, 2, 97, src0=2) == inval                # unknown layout before geometry and alignment
    assert ask(CF, 3, 4, 2, 96, 0, 97) == inval                # t_hi > ntime before npol = 3
    assert ask(ROWS, 3, 1, 2, 96, bin_rows=0) == inval         # bin_rows = 0 before R = 6
    assert ask(CF, 3, 4, 2, 96, src0=2) == notsup
    assert ask(CF, 1, 4, 2, 97, 0, 98) == inval                # the range before the pitch
    assert ask(CF, 2, 4, 2, 96, src0=-2) == inval              # a negative offset before its alignment


def test_supported_wrapper():
    from baseband_amd import kernels, _lib
    assert kernels.i8_moments_supported(_lib.MOMENTS_GUPPI_CF, 2, 64, 2, 1000)
    assert not kernels.i8_moments_supported(_lib.MOMENTS_MKBF, 2, 64, 2, 1024)
    assert not kernels.i8_moments_supported(_lib.MOMENTS_ROWS, 3, 1, 2, 100)
    assert not kernels.i8_moments_supported(_lib.MOMENTS_ROWS, 2, 2, 2, 100, src0=2)
    assert not kernels.i8_moments_supported(_lib.MOMENTS_ROWS, 2, 2, 2, 100, bin_rows=1 << 70)
