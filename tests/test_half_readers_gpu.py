"""Stream readers returning float16 / bfloat16 samples: ``read(out=<half
tensor>)`` and ``fh.sample_dtype``.  Expected values, no tolerance: ``read()``
of a plain reader converted with ``Tensor.to(dtype)`` (round to nearest even);
comparisons on the integer view.  Where the format has 16-bit decode kernels
the launch must BE one of them (`_lib.last_kernel()`): through the float32
detour the values agreed before this feature existed."""
import io
import warnings

import numpy as np
import pytest

from conftest import golden_path

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


def as_type(full, elem):
    """float32 / complex64 samples -> `elem` (complex: (re, im) pairs of it)."""
    torch = _torch()
    if full.is_complex():
        return torch.view_as_complex(torch.view_as_real(full).to(elem))
    return full.to(elem)


def bits(t):
    torch = _torch()
    if t.is_complex():
        t = torch.view_as_real(t)
    assert t.dtype in (torch.float16, torch.bfloat16), t.dtype
    return t.contiguous().view(torch.int16).cpu().numpy()


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(bits(got), bits(want))


def ran_half():
    from baseband_amd import _lib
    return _lib.last_kernel().startswith('k_decode_half_')


def vdif_1thread(**kw):
    from baseband_amd import vdif, synth
    image, h0 = synth.random_vdif(11, 96, nthread=1, nchan=1, bps=2, payload_nbytes=8000, frame_rate=1000)
    return vdif.open(io.BytesIO(image.tobytes()), 'rs', sample_rate=1000 * h0.samples_per_frame, **kw)


def vdif_8thread_complex(**kw):
    """The geometry of `smoke()`: 8 threads, 4 channels, 2-bit complex, two invalid frames."""
    from baseband_amd import vdif, synth
    image, h0 = synth.random_vdif(2024, 40, nthread=8, nchan=4, bps=2, complex_data=True, payload_nbytes=4000,
                                  frame_rate=20, thread_order=[1, 3, 5, 7, 0, 2, 4, 6],
                                  invalid=[(3, 2), (17, 5)])
    kw.setdefault('squeeze', False)
    return vdif.open(io.BytesIO(image.tobytes()), 'rs', sample_rate=20 * h0.samples_per_frame, **kw)


def vdif_channel_subset(**kw):
    return vdif_8thread_complex(subset=(slice(None), [2, 0]), **kw)


def mark5b_sample(**kw):
    from baseband_amd import mark5b
    return mark5b.open(golden_path('samples/sample.m5b'), 'rs', sample_rate=32e6, kday=56000, nchan=8, bps=2, **kw)


def dada_sample(**kw):
    from baseband_amd import dada
    return dada.open(golden_path('samples/sample.dada'), 'rs', **kw)


def gsb_rawdump(**kw):
    from baseband_amd import gsb
    return gsb.open(golden_path('samples/gsb/sample_gsb_rawdump.timestamp'), 'rs',
                    raw=golden_path('samples/gsb/sample_gsb_rawdump.dat'), samples_per_frame=8192, **kw)


def gsb_phased(**kw):
    from baseband_amd import gsb
    d = 'samples/gsb/sample_gsb_phased.'
    raw = [[golden_path(d + 'Pol-L1.dat'), golden_path(d + 'Pol-L2.dat')],
           [golden_path(d + 'Pol-R1.dat'), golden_path(d + 'Pol-R2.dat')]]
    return gsb.open(golden_path(d + 'timestamp'), 'rs', raw=raw, samples_per_frame=8, **kw)


def mark4_sample(**kw):
    from baseband_amd import mark4
    return mark4.open(golden_path('samples/sample.m4'), 'rs', ntrack=64, decade=2010, **kw)


def guppi_sample(**kw):
    from baseband_amd import guppi
    return guppi.open(golden_path('samples/sample_puppi.raw'), 'rs', **kw)


def mkbf_sample(**kw):
    from baseband_amd import dada
    return dada.open(golden_path('samples/sample_mkbf.dada'), 'rs', **kw)


DIRECT = [vdif_1thread, vdif_8thread_complex, mark5b_sample, dada_sample, gsb_rawdump, gsb_phased]
FALLBACK = [mark4_sample, guppi_sample, mkbf_sample, vdif_channel_subset]
ELEMS = ['float16', 'bfloat16']


def _skip_complex_bfloat16(fh, elem):
    torch = _torch()
    return fh.complex_data and elem == torch.bfloat16


def _walk(opener, elem, direct):
    torch = _torch()
    with opener() as ref:
        full = ref.read()
        native = ref.dtype
        if _skip_complex_bfloat16(ref, elem):
            # no complex bfloat16 in torch: refused, and said so
            with pytest.raises(ValueError, match='complex bfloat16'):
                ref.sample_dtype = elem
            with pytest.raises(ValueError, match='complex bfloat16'):
                opener(sample_dtype=elem)
            ref.seek(0)
            with pytest.raises(ValueError, match='complex bfloat16'):
                ref.read(out=torch.empty(full.shape, dtype=torch.bfloat16, device='cuda'))
            return
    assert full.dtype in (torch.float32, torch.complex64)
    want = as_type(full, elem)
    n = full.shape[0]
    check = (lambda: None) if not direct else (lambda: ran_half() or pytest.fail('float32 detour'))
    ref = opener()

    def plain(lo, count):
        """The same read on a plain reader, converted (GUPPI reads that enter a block
        continue into its overlap: a piece is compared with the same piece)."""
        ref.seek(lo)
        return as_type(ref.read(count), elem)

    try:
        # read(out=<16-bit tensor>): a direct target
        with opener() as fh:
            spf = fh.samples_per_frame
            out = torch.empty(want.shape, dtype=want.dtype, device='cuda')
            assert fh.read(out=out) is out
            check()
            assert same(out, want)
            # ... starting and stopping inside frames (head and tail through temporaries)
            lo = min(n - 2, spf // 3 + 1)
            hi = max(lo + 1, n - max(1, spf // 5))
            part = torch.empty((hi - lo,) + tuple(want.shape[1:]), dtype=want.dtype, device='cuda')
            fh.seek(lo)
            fh.read(out=part)
            assert same(part, plain(lo, hi - lo))
            # ... and float32 in between is what it always was
            fh.seek(0)
            again = fh.read()
            assert again.dtype == full.dtype and torch.equal(again, full)
            assert fh.dtype == native and fh.sample_dtype is None

        # sample_dtype at open: read() returns the type, whole file and pieces
        with opener(sample_dtype=elem) as fh:
            assert fh.sample_dtype == elem and fh.dtype == native
            got = fh.read()
            check()
            assert same(got, want)
            fh.seek(lo)
            assert same(fh.read(hi - lo), plain(lo, hi - lo))
            # a float32 `out` keeps its full precision whatever the attribute says
            fh.seek(0)
            f32 = torch.empty_like(full)
            fh.read(out=f32)
            assert torch.equal(f32, full)

        # the attribute set later; a loop of small sequential reads (the decoded read-ahead window)
        with opener() as fh:
            fh.sample_dtype = elem
            step = max(1, min(n // 7, spf // 4 + 3))
            ref.seek(0)
            reads = 0
            while fh.tell() < n and reads < 40:
                count = min(step, n - fh.tell())
                assert same(fh.read(count), as_type(ref.read(count), elem)), (reads, fh.tell())
                reads += 1
            # float32 reads that continue the loop are not served from the 16-bit window
            if fh.tell() + 2 <= n:
                fh.sample_dtype = None
                assert torch.equal(fh.read(2), ref.read(2))

        # a resident reader
        with opener(sample_dtype=elem) as fh:
            fh.stage()
            got = fh.read()
            check()
            assert same(got, want)
            fh.seek(lo)
            part = torch.empty((hi - lo,) + tuple(want.shape[1:]), dtype=want.dtype, device='cuda')
            fh.read(out=part)
            assert same(part, plain(lo, hi - lo))
    finally:
        ref.close()


@pytest.mark.parametrize('elem', ELEMS)
@pytest.mark.parametrize('opener', DIRECT, ids=[f.__name__ for f in DIRECT])
def test_readers_decode_16_bit_samples_directly(opener, elem):
    _walk(opener, getattr(_torch(), elem), True)


@pytest.mark.parametrize('elem', ELEMS)
@pytest.mark.parametrize('opener', FALLBACK, ids=[f.__name__ for f in FALLBACK])
def test_readers_without_16_bit_kernels_convert(opener, elem):
    """Mark 4, GUPPI, MKBF and a channel subset folded into the decode: float32
    decode, then the conversion -- the same values."""
    _walk(opener, getattr(_torch(), elem), False)


def test_complex_streams_give_complex32():
    torch = _torch()
    with vdif_8thread_complex(sample_dtype=torch.float16) as fh:
        got = fh.read(100)
        assert got.dtype == torch.complex32 and got.shape == (100, 8, 4)
    with dada_sample(sample_dtype='float16') as fh:            # (the name of the type is taken too)
        assert fh.read(10).dtype == torch.complex32
    with vdif_1thread() as fh:
        with pytest.raises(ValueError):
            fh.sample_dtype = torch.float64
        fh.sample_dtype = torch.float32                         # float32 is the default
        assert fh.sample_dtype is None


def test_host_results_readers_ignore_sample_dtype():
    torch = _torch()
    with vdif_1thread() as fh:
        fh.host_results = True
        fh.sample_dtype = torch.float16
        got = fh.read(1000)
        assert isinstance(got, np.ndarray) and got.dtype == np.float32
    with vdif_1thread() as ref:
        assert np.array_equal(got, ref.read(1000).cpu().numpy())


@pytest.mark.parametrize('elem', ELEMS)
def test_numpy_out_stays_float32(elem):
    torch = _torch()
    with vdif_1thread(sample_dtype=getattr(torch, elem)) as fh, vdif_1thread() as ref:
        out = np.empty((5000,), np.float32)
        fh.seek(777)
        fh.read(out=out)
        ref.seek(777)
        assert np.array_equal(out, ref.read(5000).cpu().numpy())


@pytest.mark.parametrize('elem', ELEMS)
def test_pickled_reader_keeps_sample_dtype(elem):
    import pickle
    torch = _torch()
    with mark5b_sample(sample_dtype=getattr(torch, elem)) as fh:
        fh.seek(100)
        twin = pickle.loads(pickle.dumps(fh))
        try:
            assert twin.sample_dtype == getattr(torch, elem) and twin.tell() == 100
            assert same(twin.read(50), fh.read(50))
        finally:
            twin.close()


@pytest.mark.parametrize('elem', ELEMS)
def test_repaired_file_gives_the_same_samples_in_16_bits(elem, tmp_path):
    """verify='fix' on a damaged file of the existing fixtures (tests/test_corrupt_gpu.py):
    the same samples in 16 bits as in 32 after conversion, the same warning."""
    torch = _torch()
    from baseband_amd import vdif
    from test_corrupt_gpu import CASES, _corrupt
    elem = getattr(torch, elem)
    for i, case in enumerate(CASES[:3]):
        p = tmp_path / 'corrupt{}.vdif'.format(i)
        p.write_bytes(_corrupt(case).tobytes())
        with vdif.open(str(p), 'rs', squeeze=False) as fh:
            with pytest.warns(UserWarning, match='problem loading frame'):
                full = fh.read()
        with vdif.open(str(p), 'rs', squeeze=False, sample_dtype=elem) as fh:
            with pytest.warns(UserWarning, match='problem loading frame'):
                got = fh.read()
            assert ran_half()
        assert same(got, as_type(full, elem))
        with vdif.open(str(p), 'rs', squeeze=False) as fh:
            out = torch.empty(full.shape, dtype=elem, device='cuda')
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                fh.read(out=out)
        assert same(out, as_type(full, elem))
