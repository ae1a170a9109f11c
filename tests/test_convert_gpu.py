"""baseband_amd.convert on the sample files: the repack path (packed bytes rearranged on the
GPU, nothing decoded) and the decode / encode loop write identical files, the result reads
back equal to the original (the tutorial's assertion, docs/tutorials/
using_baseband.rst:560-593), invalid frames travel as invalid frames, a tail shorter than a
frame stays pending in the writer, and what the repack path does not take is refused by
name with ``packed=True`` and converted by the loop with ``packed=None``."""
import numpy as np
import pytest

from conftest import golden_path, load_file

pytestmark = pytest.mark.gpu

T_M5B = np.datetime64('2014-06-13T05:30:01')


def _bb():
    import baseband_amd
    return baseband_amd


def open_m5b():
    return _bb().mark5b.open(golden_path('samples/sample.m5b'), 'rs', sample_rate=32e6, kday=56000, nchan=8, bps=2)


def open_vdif(path=None, **kw):
    return _bb().vdif.open(golden_path('samples/sample.vdif') if path is None else path, 'rs', **kw)


def vdif_writer(path, fr, nthread, nchan, samples_per_frame, sample_rate, **kw):
    return _bb().vdif.open(path, 'ws', sample_rate=sample_rate, nthread=nthread, nchan=nchan, edv=0, bps=fr.bps,
                           complex_data=fr.complex_data, samples_per_frame=samples_per_frame, station='cv',
                           time=fr.start_time, **kw)


def m5b_writer(path, nchan, **kw):
    return _bb().mark5b.open(path, 'ws', sample_rate=32e6, nchan=nchan, bps=2, time=T_M5B, **kw)


# name -> (open the reader, open the writer for it, open the result)
CONVERSIONS = {
    'm5b -> vdif 1 x 8': (open_m5b, lambda p, fr: vdif_writer(p, fr, 1, 8, 4000, 32e6),
                          lambda p: open_vdif(p, sample_rate=32e6)),
    'm5b -> vdif 8 x 1': (open_m5b, lambda p, fr: vdif_writer(p, fr, 8, 1, 4000, 32e6),
                          lambda p: open_vdif(p, sample_rate=32e6)),
    'vdif 8 x 1 -> vdif 1 x 8': (open_vdif, lambda p, fr: vdif_writer(p, fr, 1, 8, 8000, 32e6),
                                 lambda p: open_vdif(p, sample_rate=32e6)),
    'vdif 8 x 1 -> m5b': (open_vdif, lambda p, fr: m5b_writer(p, 8),
                          lambda p: _bb().mark5b.open(p, 'rs', sample_rate=32e6, kday=56000, nchan=8, bps=2)),
    'vdif 1 bit, other frames': (lambda: open_vdif(golden_path('samples/sample_bps1.vdif'), sample_rate=8e6),
                                 lambda p, fr: vdif_writer(p, fr, 1, 16, 1600, 8e6),
                                 lambda p: open_vdif(p, sample_rate=8e6)),
    'vdif 8 bit complex, other frames': (lambda: open_vdif(golden_path('samples/sample_mwa.vdif'), sample_rate=1.28e6),
                                         lambda p, fr: vdif_writer(p, fr, 1, 2, 160, 1.28e6),
                                         lambda p: open_vdif(p, sample_rate=1.28e6)),
}


def run(tmp_path, tag, reader, writer, packed, count=None, seek=0):
    path = str(tmp_path / tag)
    with reader() as fr:
        fr.seek(seek)
        with writer(path, fr) as fw:
            n = _bb().convert(fr, fw, count, packed=packed)
            assert n == (fr.shape[0] - seek if count is None else count)
            assert fr.tell() == seek + n and fw.tell() == n
    return path


@pytest.mark.parametrize('name', sorted(CONVERSIONS))
def test_both_paths_write_the_same_file_and_it_reads_back_equal(name, tmp_path):
    import torch
    reader, writer, result = CONVERSIONS[name]
    a = run(tmp_path, 'packed', reader, writer, True)
    b = run(tmp_path, 'loop', reader, writer, False)
    c = run(tmp_path, 'auto', reader, writer, None)
    raw = open(a, 'rb').read()
    assert len(raw) > 0 and raw == open(b, 'rb').read() == open(c, 'rb').read()
    with reader() as old, result(a) as new:
        want, got = old.read(), new.read()
        assert new.shape[0] == old.shape[0]
        assert torch.equal(got.reshape(want.shape), want)
        assert bool((want != 0).any())


def invalid_sample_vdif(tmp_path, frame):
    """A copy of sample.vdif with the invalid bit set in the header of one frame."""
    raw = load_file('samples/sample.vdif').copy()
    assert raw.size == 16 * 5032
    raw[frame * 5032 + 3] |= 0x80
    path = str(tmp_path / 'invalid.vdif')
    raw.tofile(path)
    return path


@pytest.mark.parametrize('nthread,nchan', [(1, 8), (8, 1)])
def test_invalid_frames_travel(nthread, nchan, tmp_path):
    """Frame 11 of 16 (frame set 1: samples 20000 .. 40000) invalid -> output frames of 3200
    samples: frames 6 .. 12 draw from it (6 holds samples 19200 .. 22400), frames 0 .. 5 do not."""
    import torch
    src = invalid_sample_vdif(tmp_path, 11)
    spf = 3200
    assert 40000 % spf != 0                                   # a tail of 1600 samples on top
    paths = {}
    for packed in (True, False):
        path = paths[packed] = str(tmp_path / 'out{}.vdif'.format(int(packed)))
        with open_vdif(src) as fr, vdif_writer(path, fr, nthread, nchan, spf, 32e6) as fw:
            assert fr.frames_valid(40000, spf).tolist() == [True] * 6 + [False] * 7
            assert _bb().convert(fr, fw, 12 * spf, packed=packed) == 12 * spf
    raw = np.fromfile(paths[True], np.uint8)
    assert np.array_equal(raw, np.fromfile(paths[False], np.uint8))
    payload = spf * nchan * 2 // 8
    frame = 32 + payload                                      # EDV 0 of the writer: 32-byte headers
    assert raw.size == 12 * nthread * frame
    invalid = (raw[3::frame] >> 7).reshape(12, nthread)
    assert invalid.tolist() == [[0] * nthread] * 6 + [[1] * nthread] * 6
    with open_vdif(src) as old, open_vdif(paths[True], sample_rate=32e6) as new:
        want, got = old.read(12 * spf), new.read()
        got = got.reshape(want.shape)
        assert torch.equal(got[:6 * spf], want[:6 * spf]) and bool((want[:6 * spf] != 0).all())
        assert bool((got[6 * spf:] == 0).all())                # read back as the fill value


def test_a_tail_stays_pending_in_the_writer(tmp_path):
    import torch
    count = 2 * 4000 + 1236
    pending = {}
    for packed in (True, False):
        path = str(tmp_path / 'tail{}.vdif'.format(int(packed)))
        with open_m5b() as fr:
            fw = vdif_writer(path, fr, 8, 1, 4000, 32e6)
            assert _bb().convert(fr, fw, count, packed=packed) == count
            assert fr.tell() == count and fw.tell() == count
            assert fw._npending == 1236 and fw._nframes_written == 2
            pending[packed] = torch.cat([d for d, _ in fw._pending]).clone(), [ok for _, ok in fw._pending]
            fw.write(fr.read(4000 - 1236).reshape((-1,) + fw.sample_shape))
            fw.close()
    assert torch.equal(pending[True][0], pending[False][0]) and pending[True][1] == pending[False][1]
    a, b = (open(str(tmp_path / 'tail{}.vdif'.format(k)), 'rb').read() for k in (1, 0))
    assert a == b and len(a) == 3 * 8 * (32 + 1000)
    with open_m5b() as old, open_vdif(str(tmp_path / 'tail1.vdif'), sample_rate=32e6) as new:
        assert torch.equal(new.read().reshape(12000, 8), old.read(12000))


def refusals(tmp_path):
    """name -> (reader, writer, seek, word of the reason)"""
    bb = _bb()

    def mark4():
        return bb.mark4.open(golden_path('samples/sample.m4'), 'rs', ntrack=64, decade=2010)

    def m5b_half():
        return bb.mark5b.open(golden_path('samples/sample.m5b'), 'rs', sample_rate=32e6, kday=56000, nchan=8, bps=2,
                              subset=[0, 1, 2, 3])

    def vdif4(path, fr):                                    # 4-bit frames for 2-bit samples
        return bb.vdif.open(path, 'ws', sample_rate=32e6, nthread=8, nchan=1, edv=0, bps=4, complex_data=False,
                            samples_per_frame=4000, station='cv', time=fr.start_time)

    return {
        'mark4': (mark4, lambda p, fr: vdif_writer(p, fr, 1, fr.sample_shape[0], 4000, 32e6), 0, 'VDIF or Mark 5B'),
        'subset': (m5b_half, lambda p, fr: vdif_writer(p, fr, 1, 4, 4000, 32e6), 0, 'subset'),
        'offset': (open_vdif, lambda p, fr: vdif_writer(p, fr, 8, 1, 4000, 32e6), 4002, 'byte boundary'),
        'bps': (open_vdif, vdif4, 0, 'bits per sample'),
    }


@pytest.mark.parametrize('name', ['mark4', 'subset', 'offset', 'bps'])
def test_what_the_repack_path_does_not_take(name, tmp_path):
    import torch
    reader, writer, seek, word = refusals(tmp_path)[name]
    count = 8000
    with reader() as fr, writer(str(tmp_path / 'refused'), fr) as fw:
        fr.seek(seek)
        with pytest.raises(NotImplementedError, match=word):
            _bb().convert(fr, fw, count, packed=True)
        assert fr.tell() == seek and fw.tell() == 0
        fw.write(fr.read(4000).reshape((4000,) + fw.sample_shape))
    path = run(tmp_path, 'auto', reader, writer, None, count=count, seek=seek)
    assert open(path, 'rb').read() == open(run(tmp_path, 'loop', reader, writer, False, count=count, seek=seek), 'rb').read()
    with reader() as old, open_vdif(path, sample_rate=32e6) as new:
        old.seek(seek)
        want, got = old.read(count), new.read()
        assert got.shape[0] == count and bool((want != 0).any())
        got = got.reshape(want.shape)
        if name == 'mark4':
            # the samples a Mark 4 header overwrote read as 0.0, which no 2-bit code holds: the
            # encoder gives them code 2, level 1.0 (base/encoding.py:77-102); all others are exact
            gone = want == 0
            assert bool(gone.any()) and bool((got[gone] == 1.0).all())
            assert torch.equal(got[~gone], want[~gone])
        elif name != 'bps':                                 # (2-bit levels are not 4-bit levels: that one rescales)
            assert torch.equal(got, want)
