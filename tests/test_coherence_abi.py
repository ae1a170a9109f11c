"""bb_i8_coherence_check and the argument checks of bb_i8_coherence, without a device: every refusal, the
order of the checks, and the call's answers that come before any launch (made-up device addresses: none of
these calls gets as far as one)."""
import ctypes

CF, TF, ROWS, MKBF = 0, 1, 2, 3


def ask(layout, npol, nchan, ncomp, ntime, t_lo=0, t_hi=None, bin_rows=1, src0=0, src_stride=0):
    from baseband_amd import _lib
    return _lib.i8_coherence_check(layout, npol, nchan, ncomp, ntime, t_lo, ntime if t_hi is None else t_hi,
                                   bin_rows, src0, src_stride)


def test_the_entries_are_bound_and_declared():
    import os
    from conftest import ROOT
    from baseband_amd import _lib
    bound = dict((n, a) for n, _, a in _lib.SIGNATURES)
    assert bound['bb_i8_coherence'] == bound['bb_i8_moments'] and bound['bb_i8_coherence_check'] == bound['bb_i8_moments_check']
    with open(os.path.join(ROOT, 'include', 'bbdecode.h')) as f:
        text = f.read()
    assert 'int bb_i8_coherence(' in text and 'int bb_i8_coherence_check(const bb_moments_params *params);' in text


def test_geometries_the_kernel_takes():
    from baseband_amd import _lib
    ok = _lib.BB_OK
    for nchan in (1, 3, 64, 65):
        assert ask(CF, 2, nchan, 2, 96) == ok and ask(CF, 2, nchan, 2, 4200) == ok
    for nchan in (1, 3, 8, 65, 4100):
        assert ask(TF, 2, nchan, 2, 96) == ok
    for nchan in (1, 2, 4, 6, 66, 130, 1 << 20):
        assert ask(ROWS, 2, nchan, 2, 1001) == ok, nchan
    assert ask(CF, 2, 4, 2, 96, 3, 91, 7, 4096, 1 << 20) == ok
    assert ask(CF, 2, 4, 2, 96, 5, 5) == ok                    # nothing asked for is not an error


def test_refusals_of_the_moments_check_stay():
    from baseband_amd import _lib
    inval, notsup = _lib.BB_EINVAL, _lib.BB_ENOTSUP
    assert _lib.lib.bb_i8_coherence_check(None) == inval
    assert ask(MKBF, 2, 4, 2, 256) == notsup                   # heaps are not taken
    assert ask(4, 2, 4, 2, 256) == inval and ask(-1, 2, 4, 2, 256) == inval
    for bad in ((CF, 0, 4, 2, 96), (CF, 2, 0, 2, 96), (CF, 2, 4, 3, 96), (CF, 2, 4, 0, 96)):
        assert ask(*bad) == inval
    assert ask(CF, 2, 4, 2, 0, 0, 0) == inval
    assert ask(CF, 2, 4, 2, 96, 0, 97) == inval                # t_hi > ntime
    assert ask(CF, 2, 4, 2, 96, 50, 49) == inval               # t_lo > t_hi
    assert ask(CF, 2, 4, 2, 96, bin_rows=0) == inval
    assert ask(CF, 2, 4, 2, 96, src0=-4) == inval and ask(CF, 2, 4, 2, 96, src_stride=-4) == inval
    assert ask(CF, 3, 4, 2, 96) == notsup and ask(TF, 3, 4, 2, 96) == notsup
    assert ask(ROWS, 2, (1 << 20) + 4, 2, 96) == notsup        # more channels than the kernel numbers
    assert ask(CF, 2, 4, 2, 96, src0=2) == notsup and ask(TF, 2, 4, 2, 96, src_stride=6) == notsup
    assert ask(ROWS, 2, 2, 2, 96, src0=1) == notsup


def test_the_three_new_refusals():
    """Geometries that bb_i8_moments takes and bb_i8_coherence does not."""
    from baseband_amd import _lib
    ok, notsup = _lib.BB_OK, _lib.BB_ENOTSUP
    for geom in ((CF, 1, 4, 2, 96), (ROWS, 1, 2, 2, 96), (ROWS, 4, 4, 2, 96),          # npol != 2
                 (ROWS, 2, 2, 1, 96), (ROWS, 2, 1, 1, 96),                              # ncomp != 2
                 (ROWS, 2, 3, 2, 96), (ROWS, 2, 65, 2, 96), (ROWS, 2, 4097, 2, 96)):    # plain rows, nchan > 1 and odd
        assert _lib.i8_moments_check(*geom, 0, 96) == ok, geom
        assert ask(*geom) == notsup, geom
    assert ask(ROWS, 2, 1, 2, 96) == ok                        # one channel is a run of quads
    assert ask(TF, 2, 3, 2, 96) == ok and ask(CF, 2, 3, 2, 96) == ok   # odd nchan elsewhere: a quad is a dword


def test_order_of_the_checks():
    """layout, then nonsense, then the moments geometry and alignment, then the three of this entry."""
    from baseband_amd import _lib
    inval, notsup = _lib.BB_EINVAL, _lib.BB_ENOTSUP
    assert ask(MKBF, 0, 0, 7, 0, 5, 3, 0, -1, -1) == notsup    # heaps, whatever else is wrong
    assert ask(9, 1, 3, 1, 97, src0=2) == inval                # unknown layout before everything
    assert ask(ROWS, 1, 3, 2, 96, 0, 97) == inval              # t_hi > ntime before npol = 1
    assert ask(ROWS, 2, 3, 2, 96, bin_rows=0) == inval         # bin_rows = 0 before odd nchan
    assert ask(ROWS, 2, 3, 1, 96, src0=-2) == inval            # a negative offset before ncomp = 1
    assert ask(CF, 1, 4, 2, 97, 0, 98) == inval                # the range before the pitch and npol = 1
    # (where both refuse, both say BB_ENOTSUP: the order among them does not show)
    assert ask(CF, 1, 4, 2, 97) == notsup and ask(ROWS, 2, 3, 2, 96, src0=2) == notsup


def _call(p, d_buf=1 << 20, buf_nbytes=1 << 20, d_src=None, nframes=1, d_sums=1 << 30, sums_elems=1 << 20):
    from baseband_amd import _lib
    return _lib.lib.bb_i8_coherence(d_buf, buf_nbytes, d_src, nframes, ctypes.byref(p) if p is not None else None,
                                    d_sums, sums_elems, None)


def test_call_time_answers_before_any_launch():
    from baseband_amd import _lib
    inval, notsup, erange, ok = _lib.BB_EINVAL, _lib.BB_ENOTSUP, _lib.BB_ERANGE, _lib.BB_OK

    def params(layout=CF, npol=2, nchan=4, ncomp=2, ntime=96, t_lo=0, t_hi=96, bin_rows=8, nbins=12, first_row=0, src0=0, src_stride=0):
        return _lib.moments_params(layout, npol, nchan, ncomp, ntime, t_lo, t_hi, bin_rows, nbins, first_row, src0, src_stride)

    assert _call(None) == inval
    assert _call(params(layout=ROWS, nchan=3)) == notsup and _call(params(npol=1)) == notsup and _call(params(layout=MKBF)) == notsup
    # the sums: NULL, off 8 bytes, fewer than nbins * nchan * 4
    assert _call(params(), d_sums=None) == inval and _call(params(), d_sums=(1 << 30) + 4) == inval
    assert _call(params(), sums_elems=12 * 4 * 4 - 1) == erange
    assert _call(params(nbins=1 << 62)) == erange
    # ... what bb_i8_moments would take for these bins (npol * nchan * ncomp * 2 = 32 a bin) is not the measure
    assert _call(params(), sums_elems=12 * 4 * 4, nframes=0) == ok
    assert _call(params(first_row=(1 << 56) + 1)) == erange
    # nothing asked for: BB_OK whatever the buffer is
    assert _call(params(), nframes=0, d_buf=None) == ok and _call(params(t_lo=7, t_hi=7), d_buf=None) == ok
    # the last row's bin, before the buffer
    assert _call(params(nbins=11), d_buf=None) == erange and _call(params(first_row=1), d_buf=None) == erange
    assert _call(params(), d_buf=None) == inval
    assert _call(params(), d_buf=(1 << 20) + 2) == notsup
    assert _call(params(src0=1 << 20)) == erange               # the payload outside the buffer
    assert _call(params(src_stride=1 << 20, nbins=24), nframes=2) == erange
    # the order: a short d_sums before the last row's bin, that before a NULL buffer
    assert _call(params(nbins=11), sums_elems=8, d_buf=None) == erange and _call(params(), d_sums=None, d_buf=None) == inval


def test_supported_wrapper():
    from baseband_amd import kernels, _lib
    assert kernels.i8_coherence_supported(_lib.MOMENTS_GUPPI_CF, 64, 1000)
    assert kernels.i8_coherence_supported(_lib.MOMENTS_ROWS, 4, 1000) and kernels.i8_coherence_supported(_lib.MOMENTS_ROWS, 1, 1000)
    assert not kernels.i8_coherence_supported(_lib.MOMENTS_MKBF, 64, 1024)
    assert not kernels.i8_coherence_supported(_lib.MOMENTS_ROWS, 3, 100)
    assert not kernels.i8_coherence_supported(_lib.MOMENTS_ROWS, 2, 100, src0=2)
    assert not kernels.i8_coherence_supported(_lib.MOMENTS_ROWS, 2, 100, bin_rows=1 << 70)
