"""``fh.state_counts()`` / ``fh.state_levels`` of the VDIF and Mark 5B stream readers
against a NumPy count over the file's payload bytes and against ``fh.read()``: exact."""
import io
import os
import tempfile

import numpy as np
import pytest

from conftest import golden_path, load_file
from packedkit import _torch, unpack_codes

pytestmark = pytest.mark.gpu


# -- the files -------------------------------------------------------------------------
def sample_vdif():
    from baseband_amd import vdif
    return load_file('samples/sample.vdif'), vdif.open, {}


def sample_m5b():
    from baseband_amd import mark5b
    return load_file('samples/sample.m5b'), mark5b.open, dict(sample_rate=32e6, kday=56000, nchan=8, bps=2)


def threads_complex():
    """8 threads out of order, 4 channels, 2-bit complex, two frames flagged invalid."""
    from baseband_amd import vdif, synth
    image, h0 = synth.random_vdif(2024, 12, nthread=8, nchan=4, bps=2, complex_data=True, payload_nbytes=4000,
                                  frame_rate=20, thread_order=[1, 3, 5, 7, 0, 2, 4, 6], invalid=[(3, 2), (7, 5)])
    return image, vdif.open, dict(sample_rate=20 * h0.samples_per_frame)


_written = {}


def written_vdif():
    """A 2-bit, 2-thread file from the package's own writer; three headers then get their
    invalid bit."""
    from baseband_amd import vdif
    if 'image' not in _written:
        torch = _torch()
        spf, nsets = 4000, 9
        gen = torch.Generator().manual_seed(7)
        data = (torch.randn((nsets * spf, 2, 1), generator=gen) * 2.2).cuda()
        with tempfile.TemporaryDirectory() as tmp:
            name = os.path.join(tmp, 'written.vdif')
            with vdif.open(name, 'ws', sample_rate=spf * 50., nthread=2, edv=0, bps=2, nchan=1,
                           samples_per_frame=spf, station='ab', time=np.datetime64('2020-01-01T00:00:00'),
                           squeeze=False) as fw:
                fw.write(data)
            image = np.fromfile(name, dtype=np.uint8)
        frame = 32 + spf * 2 // 8
        assert len(image) == nsets * 2 * frame
        for k in (1, 6, 13):
            image[k * frame + 3] |= 0x80
        _written['image'] = image
    return _written['image'], vdif.open, dict(sample_rate=4000 * 50.)


FILES = [sample_vdif, sample_m5b, threads_complex, written_vdif]


def open_on(image, opener, kw, how='file', **more):
    """'file': a host file object (windows go through the staging pipeline); 'staged':
    the same, `stage()`d; 'device': a reader on a device tensor."""
    kw = dict(kw, squeeze=False, **more)
    if how == 'device':
        return opener(_torch().from_numpy(image.copy()).cuda(), 'rs', **kw)
    fh = opener(io.BytesIO(image.tobytes()), 'rs', **kw)
    return fh.stage() if how == 'staged' else fh


# -- the expectation -------------------------------------------------------------------
def numpy_counts(fh, image, start, stop):
    """Count the codes of samples [start, stop) from the file's bytes: frames at the fixed
    stride, placed by where they stand, flagged (VDIF) or fill-pattern (Mark 5B) frames
    left out."""
    is_vdif = hasattr(fh, '_file_threads')
    bps, spf = fh.bps, fh.samples_per_frame
    if is_vdif:
        h0 = fh.header0
        frame, header, off0 = h0.frame_nbytes, h0.nbytes, 0
        chunk = h0.nchan * (2 if fh.complex_data else 1)
        threads, per_set = [int(t) for t in fh._thread_ids], len(fh._file_threads)
    else:
        frame, header, off0 = 10016, 16, fh._file_offset0
        chunk, threads, per_set = fh.sample_shape[-1] if fh.sample_shape else 1, [0], 1
    out = np.zeros((len(threads), chunk, 1 << bps), np.int64)
    nfr = (len(image) - off0) // frame
    pos = (np.arange(spf * chunk) % chunk) << bps
    for k in range(nfr):
        fr = image[off0 + k * frame:off0 + (k + 1) * frame]
        w = fr[:16].copy().view('<u4')
        if is_vdif:
            invalid, thread = bool(w[0] >> 31), int((w[3] >> 16) & 0x3ff)
        else:
            invalid, thread = bool((fr[header:].view('<u4') == 0x11223344).all()), 0
        f = k // per_set
        r0, r1 = max(start, f * spf) - f * spf, min(stop, (f + 1) * spf) - f * spf
        if invalid or thread not in threads or r0 >= r1:
            continue
        key = pos + unpack_codes(fr[header:], bps)
        out[threads.index(thread)] += np.bincount(key[r0 * chunk:r1 * chunk],
                                                  minlength=chunk << bps).reshape(chunk, 1 << bps)
    return out


def shaped(fh, flat):
    """(slot, chunk, level) -> the reader's documented shape."""
    if not hasattr(fh, '_file_threads'):
        return flat[0]
    if fh.complex_data:
        return flat.reshape(flat.shape[0], -1, 2, flat.shape[-1])
    return flat


def weighted_sum_equals_read(fh, counts, count=None):
    """(counts * levels).sum(-1) is the sum of the samples read() gives with fill 0: both
    are exact in float64 (levels of 24 bits, far fewer than 2^29 samples)."""
    torch = _torch()
    data = fh.read(count)
    if data.is_complex():
        data = torch.view_as_real(data)
    want = data.double().sum(0).cpu().numpy()
    got = (counts.cpu().numpy() * fh.state_levels.astype(np.float64)).sum(-1)
    return got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize('how', ['file', 'staged', 'device'])
@pytest.mark.parametrize('make', FILES)
def test_state_counts_of_a_file(make, how):
    torch = _torch()
    image, opener, kw = make()
    with open_on(image, opener, kw, how) as fh:
        total, spf = fh.shape[0], fh.samples_per_frame
        levels = fh.state_levels
        assert levels.dtype == np.float32 and levels.shape == (1 << fh.bps,)
        counts = fh.state_counts()
        assert fh.tell() == 0
        assert counts.is_cuda and counts.dtype == torch.int64
        want = shaped(fh, numpy_counts(fh, image, 0, total))
        assert tuple(counts.shape) == want.shape
        assert np.array_equal(counts.cpu().numpy(), want)
        assert weighted_sum_equals_read(fh, counts)
        # from inside the first frame to inside a later one
        count = min(total - 124, spf + 776) | 1
        fh.seek(123)
        counts = fh.state_counts(count)
        assert fh.tell() == 123
        assert np.array_equal(counts.cpu().numpy(), shaped(fh, numpy_counts(fh, image, 123, 123 + count)))
        assert int(counts.sum()) <= count * int(np.prod(counts.shape[:-1]))
        assert weighted_sum_equals_read(fh, counts, count)
        assert fh.tell() == 123 + count
        # nothing left, nothing counted
        fh.seek(0, 2)
        assert int(fh.state_counts().sum()) == 0
        with pytest.raises(EOFError):
            fh.state_counts(1)


@pytest.mark.parametrize('make', FILES)
def test_short_staging_windows_give_the_same_counts(make):
    """Windows of two frame sets: the range's first and last window carry its row limits."""
    image, opener, kw = make()
    with open_on(image, opener, kw) as fh:
        fh.window_bytes = 2 * fh._set_nbytes
        total = fh.shape[0]
        fh.seek(123)
        counts = fh.state_counts(total - 123 - 77)
        assert np.array_equal(counts.cpu().numpy(), shaped(fh, numpy_counts(fh, image, 123, total - 77)))


def test_invalid_frames_are_left_out():
    image, opener, kw = written_vdif()
    with open_on(image, opener, kw) as fh:
        counts = fh.state_counts()
        spf = fh.samples_per_frame
        per_thread = counts.sum((1, 2)).cpu().numpy()
        nsets = fh.shape[0] // spf
        assert per_thread.tolist() == [(nsets - 1) * spf, (nsets - 2) * spf]     # frames 6 | 1 and 13
        # a written stream of Gaussian noise: the high states are there, below the low ones
        c = counts.cpu().numpy().reshape(2, 4)
        assert (c > 0).all() and (c[:, [0, 3]].sum(1) < c[:, [1, 2]].sum(1)).all()


def test_thread_selection():
    image, opener, kw = threads_complex()
    with open_on(image, opener, kw) as fh:
        every = fh.state_counts().cpu().numpy()
        assert every.shape == (8, 4, 2, 4)
    for pick in ([5, 2], [3]):
        with open_on(image, opener, kw, 'staged', subset=(pick,)) as fh:
            counts = fh.state_counts()
            assert np.array_equal(counts.cpu().numpy(), every[pick])
            assert np.array_equal(counts.cpu().numpy(), shaped(fh, numpy_counts(fh, image, 0, fh.shape[0])))
    # a channel subset is not applied: all channels of the picked threads
    with open_on(image, opener, kw, subset=([1, 6], [2, 0])) as fh:
        assert np.array_equal(fh.state_counts().cpu().numpy(), every[[1, 6]])


def test_a_sample_wider_than_the_kernel_takes_is_refused():
    from baseband_amd import vdif, synth
    image, h0 = synth.random_vdif(3, 4, nthread=1, nchan=32, bps=8, payload_nbytes=4096, frame_rate=100)
    with vdif.open(io.BytesIO(image.tobytes()), 'rs', sample_rate=100 * h0.samples_per_frame) as fh:
        with pytest.raises(NotImplementedError, match='chunk \\* bps <= 128'):
            fh.state_counts()
        assert fh.state_levels.shape == (256,)
        assert fh.tell() == 0
    image, h0 = synth.random_vdif(3, 4, nthread=1, nchan=16, bps=8, payload_nbytes=4096, frame_rate=100)
    with vdif.open(io.BytesIO(image.tobytes()), 'rs', sample_rate=100 * h0.samples_per_frame) as fh:
        assert int(fh.state_counts().sum()) == 4 * 4096


def test_readers_without_packed_fields_say_so():
    from baseband_amd import mark4
    with mark4.open(golden_path('samples/sample.m4'), 'rs', ntrack=64, decade=2010) as fh:
        with pytest.raises(NotImplementedError):
            fh.state_counts()
