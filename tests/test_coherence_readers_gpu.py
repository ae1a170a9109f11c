"""``fh.coherence_series()`` / ``fh.stokes_series()`` of the GUPPI and DADA stream readers against what
torch computes in int64 / float64 from ``fh.read()`` at the same offset: the sums compare exactly, the
Stokes series to float64 equality of the same formula."""
import numpy as np
import pytest

from test_moments_readers_gpu import offsets_of, open_on

pytestmark = pytest.mark.gpu

KERNEL = ['guppi_cf_c64_ov0', 'guppi_cf_c64_ov32', 'guppi_tf_c8_ov16', 'sample_puppi', 'sample_dada', 'dada_p2_c4_cplx']
FALLBACK = ['sample_mkbf_dada', 'sample_meerkat_dada', 'guppi_real_c1', 'dada_p2_c3_real']     # heaps; real samples
ONE_POL = ['guppi_cf_c6_p1', 'dada_p1_c1_real']
FILES = KERNEL + FALLBACK


def _torch():
    import torch
    return torch


def from_read(fh, b, n):
    """(coherence, stokes) of the next `n` samples in bins of `b`, from read(); the offset is put back."""
    torch = _torch()
    offset = fh.tell()
    data = fh.read(n)
    fh.seek(offset)
    if fh.complex_data:
        z = torch.view_as_real(data).to(torch.int64)
        xr, xi, yr, yi = z[:, 0, ..., 0], z[:, 0, ..., 1], z[:, 1, ..., 0], z[:, 1, ..., 1]
        v = torch.stack((xr * xr + xi * xi, yr * yr + yi * yi, xr * yr + xi * yi, xi * yr - xr * yi), -1)
    else:
        x, y = data[:, 0].to(torch.int64), data[:, 1].to(torch.int64)
        v = torch.stack((x * x, y * y, x * y, 0 * x), -1)
    nbins = -(-n // b)
    pad = torch.zeros((nbins * b - n,) + tuple(v.shape[1:]), dtype=torch.int64, device=v.device)
    c = torch.cat([v, pad]).reshape((nbins, b) + tuple(v.shape[1:])).sum(1)
    return c, stokes_of(c, b, n)


def stokes_of(c, b, n):
    torch = _torch()
    nbins = c.shape[0]
    cnt = torch.full((nbins,), b, dtype=torch.int64, device=c.device)
    if nbins:
        cnt[-1] = n - (nbins - 1) * b
    s = torch.stack((c[..., 0] + c[..., 1], c[..., 0] - c[..., 1], 2 * c[..., 2], 2 * c[..., 3]), -1)
    return s.double() / cnt.double().reshape((nbins,) + (1,) * (s.dim() - 1))


def test_the_polarisation_counts(manifest):
    for names, npol in ((FILES, 2), (ONE_POL, 1)):
        for name in names:
            with open_on(manifest, name, squeeze=False) as fh:
                assert fh.sample_shape[0] == npol and len(fh.sample_shape) == 2 and fh.bps == 8, name
                assert fh.complex_data == (manifest[name]['dtype'] == 'complex64') and (name not in KERNEL or fh.complex_data)


@pytest.mark.parametrize('squeeze', [True, False])
@pytest.mark.parametrize('name', FILES)
def test_against_read(manifest, name, squeeze):
    torch = _torch()
    with open_on(manifest, name, squeeze=squeeze) as fh:
        total = fh.shape[0]
        nchan = tuple(fh.sample_shape)[1:]
        assert nchan == (() if squeeze and manifest[name]['shape'][2] == 1 else (manifest[name]['shape'][2],))
        for offset in offsets_of(fh):
            left = total - offset
            for n in (left, min(left, 333)):
                for b in (1, 7, 100, n):
                    fh.seek(offset)
                    want_c, want_s = from_read(fh, b, n)
                    got_c = fh.coherence_series(b, n)
                    assert fh.tell() == offset
                    got_s = fh.stokes_series(b, n)
                    assert fh.tell() == offset
                    assert got_c.dtype == torch.int64 and got_s.dtype == torch.float64
                    assert got_c.shape == got_s.shape == (-(-n // b),) + nchan + (4,)
                    assert torch.equal(got_c, want_c), (offset, n, b)
                    assert torch.equal(got_s, want_s) and torch.equal(got_s, stokes_of(got_c, b, n)), (offset, n, b)
        # count=None: the rest of the file
        fh.seek(7)
        assert torch.equal(fh.coherence_series(64), from_read(fh, 64, total - 7)[0])
        assert torch.equal(fh.stokes_series(64), from_read(fh, 64, total - 7)[1])
        if not fh.complex_data:
            assert not fh.coherence_series(64)[..., 3].any() and fh.coherence_series(64)[..., 2].any()


@pytest.mark.parametrize('name', FILES)
def test_paths(manifest, name, monkeypatch):
    """packed=True answers where the check takes the geometry and refuses elsewhere; the
    fallback gives the same numbers everywhere and launches no coherence kernel."""
    torch = _torch()
    from baseband_amd import _lib, kernels
    launches = []
    native = kernels.i8_coherence

    def counted(*args, **kw):
        launches.append(args[2])
        return native(*args, **kw)

    monkeypatch.setattr(kernels, 'i8_coherence', counted)
    with open_on(manifest, name) as fh:
        n = fh.shape[0] - 3
        fh.seek(3)
        by_default = fh.coherence_series(50, n)
        assert bool(launches) == (name in KERNEL)
        by_default_stokes = fh.stokes_series(50, n, packed=None)
        del launches[:]
        assert torch.equal(fh.coherence_series(50, n, packed=False), by_default)
        assert torch.equal(fh.stokes_series(50, n, packed=False), by_default_stokes)
        assert not launches
        if name in KERNEL:
            got = fh.coherence_series(50, n, packed=True)
            assert launches and _lib.last_kernel().startswith('k_i8_coherence')
            assert torch.equal(got, by_default)
            assert torch.equal(fh.stokes_series(50, n, packed=True), by_default_stokes)
        else:
            with pytest.raises(NotImplementedError):
                fh.coherence_series(50, n, packed=True)
            with pytest.raises(NotImplementedError):
                fh.stokes_series(50, n, packed=True)
            assert not launches
        assert fh.tell() == 3


@pytest.mark.parametrize('name', KERNEL)
def test_the_powers_are_those_of_moment_series(manifest, name):
    torch = _torch()
    with open_on(manifest, name, squeeze=False) as fh:
        n = fh.shape[0] - 4
        fh.seek(4)
        c = fh.coherence_series(37, n)
        sq = fh.moment_series(37, n)[..., 1].sum(-1)            # (bin, pol, chan)
        assert torch.equal(c[..., 0], sq[:, 0]) and torch.equal(c[..., 1], sq[:, 1])


@pytest.mark.parametrize('name', ONE_POL)
def test_one_polarisation_is_refused(manifest, name):
    for squeeze in (True, False):
        with open_on(manifest, name, squeeze=squeeze) as fh:
            for packed in (None, False, True):
                with pytest.raises(ValueError, match='two polarisations'):
                    fh.coherence_series(10, packed=packed)
                with pytest.raises(ValueError, match='two polarisations'):
                    fh.stokes_series(10, packed=packed)


@pytest.mark.parametrize('name,subset', [('guppi_cf_c64_ov0', (slice(None), [1, 3, 60])), ('guppi_cf_c64_ov32', (slice(None), slice(8, 40, 3))),
                                         ('guppi_tf_c8_ov16', ([0, 1], slice(None))), ('dada_p2_c4_cplx', (slice(None), [3, 1])),
                                         ('sample_puppi', (slice(None), [2])), ('sample_mkbf_dada', (slice(None), [5, 900])),
                                         ('dada_p2_c3_real', (slice(None), 2))])
def test_a_channel_subset_is_the_full_answer_indexed(manifest, name, subset):
    torch = _torch()
    with open_on(manifest, name, squeeze=False) as fh:
        n = min(fh.shape[0], 700) - 2
        fh.seek(2)
        full_c, full_s = fh.coherence_series(33, n), fh.stokes_series(33, n)
    with open_on(manifest, name, subset=subset) as fh:
        fh.seek(2)
        index = torch.as_tensor(subset[1], device='cuda') if isinstance(subset[1], list) else subset[1]
        got_c, got_s = fh.coherence_series(33, n), fh.stokes_series(33, n)
        assert got_c.shape[1:-1] == tuple(fh.sample_shape)[1:]
        assert torch.equal(got_c, full_c[:, index]) and torch.equal(got_s, full_s[:, index])
        want_c, want_s = from_read(fh, 33, n)
        assert torch.equal(got_c, want_c) and torch.equal(got_s, want_s)
        assert torch.equal(fh.coherence_series(33, n, packed=False), want_c)


@pytest.mark.parametrize('subset', [(0,), (1, [0, 2]), ([1, 0],), ([0, 1], [0, 2]), ([0],), (slice(0, 1),)])
def test_a_polarisation_subset_is_refused(manifest, subset):
    for name in ('dada_p2_c4_cplx', 'guppi_cf_c64_ov0', 'dada_p2_c3_real'):
        with open_on(manifest, name, subset=subset) as fh:
            for packed in (None, False):
                with pytest.raises(ValueError, match='both polarisations'):
                    fh.coherence_series(10, 50, packed=packed)
            with pytest.raises(ValueError, match='both polarisations'):
                fh.stokes_series(10, 50)


@pytest.mark.parametrize('name', ['guppi_cf_c64_ov32', 'guppi_tf_c8_ov16', 'dada_p2_c4_cplx', 'sample_dada', 'dada_p2_c3_real'])
def test_sources(manifest, name):
    """A file on disk (staging windows, short ones too), io.BytesIO, a device tensor, a staged file,
    and the frame that a small read has left on the device: the same answers."""
    torch = _torch()
    answers = []
    for how in ('file', 'bytes', 'device', 'staged'):
        with open_on(manifest, name, how) as fh:
            n = fh.shape[0] - 9
            fh.seek(9)
            answers.append((fh.coherence_series(40, n), fh.stokes_series(40, n), fh.coherence_series(40, 17)))
            if how == 'file':
                want = from_read(fh, 40, n)
                assert torch.equal(answers[0][0], want[0]) and torch.equal(answers[0][1], want[1])
                fh.window_bytes = fh._frame_nbytes                  # a window per frame
                assert torch.equal(fh.coherence_series(40, n), want[0])
                fh.seek(20)
                fh.read(10)                                        # (leaves its frame staged)
                assert torch.equal(fh.coherence_series(3, 25), from_read(fh, 3, 25)[0])
    for a in answers[1:]:
        assert all(torch.equal(x, y) for x, y in zip(a, answers[0]))


def test_errors(manifest, tmp_path):
    from baseband_amd import dada
    with open_on(manifest, 'guppi_cf_c64_ov32') as fh:
        total = fh.shape[0]
        for method in (fh.coherence_series, fh.stokes_series):
            with pytest.raises(ValueError):
                method(0)
            with pytest.raises(ValueError):
                method(-3, 10)
            with pytest.raises(EOFError):
                method(8, total + 1)
            fh.seek(10)
            with pytest.raises(EOFError):
                method(8, total - 9)
            fh.seek(0)
            assert method(8, 0).shape == (0, 64, 4)
        assert fh.tell() == 0
    for method in (fh.coherence_series, fh.stokes_series):
        with pytest.raises(ValueError, match='closed'):
            method(8)
    # float32 DADA samples are not int8
    h = dada.DADAHeader.fromvalues(time=np.datetime64('2020-02-02T02:02:02'), sample_rate=1e6, bps=32, complex_data=True,
                                   npol=2, nchan=3, samples_per_frame=100)
    p = tmp_path / 'f32.dada'
    with open(str(p), 'wb') as fw:
        h.tofile(fw)
        fw.write(np.zeros(100 * 2 * 3 * 2, np.float32).tobytes())
    with dada.open(str(p), 'rs') as fh:
        assert fh.bps == 32
        for packed in (None, False, True):
            with pytest.raises(NotImplementedError):
                fh.coherence_series(10, packed=packed)
            with pytest.raises(NotImplementedError):
                fh.stokes_series(10, packed=packed)


def test_odd_channels_in_plain_dada_fall_back(tmp_path):
    """Two complex polarisations of three channels as plain DADA stores them: the check refuses (the Y half
    of a row begins inside a dword), the fallback answers."""
    torch = _torch()
    from baseband_amd import dada, kernels, _lib
    assert not kernels.i8_coherence_supported(_lib.MOMENTS_ROWS, 3, 100)
    h = dada.DADAHeader.fromvalues(time=np.datetime64('2020-02-02T02:02:02'), sample_rate=1e6, bps=8, complex_data=True,
                                   npol=2, nchan=3, samples_per_frame=100)
    p = tmp_path / 'c3.dada'
    raw = np.random.default_rng(9).integers(-128, 128, 100 * 2 * 3 * 2, dtype=np.int8)
    with open(str(p), 'wb') as fw:
        h.tofile(fw)
        fw.write(raw.tobytes())
    with dada.open(str(p), 'rs') as fh:
        assert tuple(fh.sample_shape) == (2, 3) and fh.shape[0] == 100
        got = fh.coherence_series(30)
        assert torch.equal(got, from_read(fh, 30, 100)[0]) and got.shape == (4, 3, 4)
        with pytest.raises(NotImplementedError):
            fh.coherence_series(30, packed=True)
