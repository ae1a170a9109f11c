"""``fr.read_packed(..., bps=, scale=)`` on files: the payloads of another sample width, or
of the same width with a gain, made on the packed bytes through a code table
(bb_requant_frames), against the package's own decode, float32 product and encoder put
into payload order; invalid frames are reported and hold the (scaled) fill code; a damaged
file is answered as ``read()`` answers it; and what the table route does not take is
refused by name."""
import numpy as np
import pytest

from conftest import golden_path
from packedkit import unpack_codes
from test_convert_gpu import T_M5B, invalid_sample_vdif, open_m5b, open_vdif

pytestmark = pytest.mark.gpu

VDIF, MARK5B = 0, 1


def _bb():
    import baseband_amd
    return baseband_amd


@pytest.fixture(scope='module')
def vdif8(tmp_path_factory):
    """An 8-bit VDIF file of one thread of 8 channels, 20 frames of 1000 samples of noise,
    written with this package's writer."""
    import torch
    path = str(tmp_path_factory.mktemp('requant') / 'noise8.vdif')
    g = torch.Generator().manual_seed(8)
    data = (torch.randn((20000, 8), generator=g) * 1.2).cuda()
    with _bb().vdif.open(path, 'ws', sample_rate=32e6, nthread=1, nchan=8, edv=0, bps=8, complex_data=False,
                         samples_per_frame=1000, station='cv', time=T_M5B) as fw:
        fw.write(data.reshape((20000,) + fw.sample_shape))
    return path


def open_mwa():
    return open_vdif(golden_path('samples/sample_mwa.vdif'), sample_rate=1.28e6)


def fill_code(value, coder, bps):
    from baseband_amd.conversion import _fill_code
    return _fill_code(value, coder, bps)


def payloads_of(x, nslot, chunk, spf, coder, bps):
    """float32 samples (n, ...) -> what a writer of `nslot` threads of `chunk` codes per sample and
    `spf` samples per frame encodes them to: uint8 (n // spf, nslot, payload)."""
    from baseband_amd import kernels
    n = x.shape[0]
    x = x.reshape(n // spf, spf, nslot, chunk).permute(0, 2, 1, 3).contiguous()
    return kernels.encode_flat(x.reshape(-1), coder, bps).reshape(n // spf, nslot, -1)


def expected(fr, n, spf, coder, bps, scale):
    """The loop's arithmetic on the next `n` samples of `fr` (the offset is put back)."""
    import torch
    g = fr._packed_geometry()
    at = fr.tell()
    x = fr.read(n)
    fr.seek(at)
    x = torch.view_as_real(x) if x.is_complex() else x
    x = x.reshape(n, g.nslot, g.chunk).float()
    if scale is not None:
        x = x * float(np.float32(scale))
    return payloads_of(x, g.nslot, g.chunk, spf, coder, bps)


# name -> (open the reader, coder and bits per sample of the output, samples per output frame, scale)
CASES = {
    'vdif 8 x 1, 2 -> 1': (open_vdif, VDIF, 1, 8000, None),
    'vdif 8 x 1, 2 -> 4': (open_vdif, VDIF, 4, 4000, None),
    'vdif 8 x 1, 2 -> 8': (open_vdif, VDIF, 8, 4000, None),
    'vdif 8 x 1, 2 -> 8, frames re-cut': (open_vdif, VDIF, 8, 3200, None),
    'm5b -> vdif 1 x 8, 2 -> 4': (open_m5b, VDIF, 4, 4000, None),
    'm5b -> vdif 1 x 8, 2 -> 8': (open_m5b, VDIF, 8, 4000, None),
    'vdif 8 -> vdif 2': (None, VDIF, 2, 4000, None),
    'vdif 8 -> m5b 2, scale 0.9': (None, MARK5B, 2, 5000, 0.9),
    'vdif 8 -> m5b 1': (None, MARK5B, 1, 10000, None),
    'vdif 2 -> 2, scale 0.5': (open_vdif, VDIF, 2, 4000, 0.5),
    'vdif 2 -> 2, scale -1.0': (open_vdif, VDIF, 2, 4000, -1.0),
    'vdif 2 -> m5b 2, scale 1.0': (open_vdif, MARK5B, 2, 4000, 1.0),
    'vdif complex 8 -> 4, scale 2': (open_mwa, VDIF, 4, 160, 2.0),
    'vdif complex 8 -> 2': (open_mwa, VDIF, 2, 160, None),
}


@pytest.mark.parametrize('name', sorted(CASES))
def test_payloads_are_decode_scale_encode(name, vdif8):
    import torch
    reader, coder, bps, spf, scale = CASES[name]
    if reader is None:
        reader = lambda: open_vdif(vdif8, sample_rate=32e6)
    with reader() as fr:
        g = fr._packed_geometry()
        nchan = g.chunk // (2 if fr.complex_data else 1)
        gain = np.float32(1.) if scale is None else np.float32(scale)
        fill = fill_code(np.float32(fr.fill_value) * gain, coder, bps)
        for seek in (0, spf):                                     # whole file, and from inside it to the end
            fr.seek(seek)
            n = (fr.shape[0] - seek) // spf * spf
            assert n > 0
            want = expected(fr, n, spf, coder, bps, scale)
            got, valid = fr.read_packed(n, coder, g.nslot, nchan, spf, fill, bps=bps, scale=scale)
            assert fr.tell() == seek + n
            assert got.dtype == torch.uint8 and tuple(got.shape) == (n // spf, g.nslot, spf * g.chunk * bps // 8)
            assert valid.dtype == bool and valid.all() and valid.shape == (n // spf,)
            assert torch.equal(got, want)
            assert len(torch.unique(got)) > 1


def test_invalid_frames_are_reported_and_hold_the_scaled_fill_code(tmp_path):
    """Frame 11 of 16 (frame set 1: samples 20000 .. 40000 of one thread) invalid -> output frames
    of 3200 samples: frames 6 .. 12 draw from it, frames 7 .. 11 wholly.  The fill value 3.0 times
    the scale 0.5 is 1.5, whose 4-bit code fills that frame's thread there."""
    import bb_oracle_np as orc
    import torch
    src = invalid_sample_vdif(tmp_path, 11)
    spf, scale = 3200, 0.5
    code = int(orc.encode_codes(np.float32([3.]) * np.float32(scale), 'vdif', 4)[0])
    assert code != int(orc.encode_codes(np.float32([3.]), 'vdif', 4)[0])
    with open_vdif(src, fill_value=3.) as fr:
        assert fill_code(np.float32(3.) * np.float32(scale), VDIF, 4) == code
        want = expected(fr, 12 * spf, spf, VDIF, 4, scale)
        got, valid = fr.read_packed(12 * spf, VDIF, 8, 1, spf, code, bps=4, scale=scale)
        assert valid.tolist() == [True] * 6 + [False] * 6
        assert torch.equal(got, want)
    frames = got.cpu().numpy()
    filled = (frames == (code | code << 4)).all(-1)           # (output frame, thread): nothing but the fill code
    thread = [t for t in range(8) if filled[7, t]]
    assert len(thread) == 1                                   # the one thread of frame 11
    mask = np.zeros((12, 8), bool)
    mask[7:, thread[0]] = True
    assert np.array_equal(filled, mask)
    cut = unpack_codes(frames[6, thread[0]], 4)
    assert (cut[800:] == code).all() and not (cut[:800] == code).all()


def test_a_damaged_file_is_answered_as_read_answers_it():
    """A file that lost frames: under ``verify='fix'`` the payloads are those of the repaired
    read, under ``verify=True`` the call raises what the read raises and the offset stays."""
    import torch
    from test_packed_damaged_gpu import oracle, quietly, what_read_raises
    o = oracle('vdif', 0)
    assert o.case['kind'] == 'frames'
    spf, scale = 4000, 0.5
    n = o.n // spf * spf
    code = fill_code(0., VDIF, 8)
    x = torch.from_numpy(np.ascontiguousarray(o.data[:n])).cuda().reshape(n, 8, 1) * scale
    want = payloads_of(x, 8, 1, spf, VDIF, 8)
    with o.open('file', verify='fix') as fr:
        got, valid = quietly(fr.read_packed, n, VDIF, 8, 1, spf, code, bps=8, scale=scale)
        assert fr.tell() == n
        assert torch.equal(got, want)
        assert not valid.all() and valid.any()
        assert np.array_equal(valid, quietly(lambda: (fr.seek(0), fr.frames_valid(n, spf))[1]))
    error = what_read_raises(o)
    with o.open('file', verify=True) as fr:
        with pytest.raises(Exception) as met:
            quietly(fr.read_packed, o.n // spf * spf, VDIF, 8, 1, spf, code, bps=8, scale=scale)
        assert met.type is error and fr.tell() == 0


def test_what_the_table_route_does_not_take():
    with open_vdif() as fr:
        with pytest.raises(NotImplementedError, match='thread structure'):      # 8 x 1 -> 1 x 8 with a width change
            fr.read_packed(8000, VDIF, 1, 8, 4000, 0, bps=4)
        with pytest.raises(NotImplementedError, match='thread structure'):      # ... with a scale
            fr.read_packed(8000, VDIF, 1, 8, 4000, 0, scale=0.5)
        with pytest.raises(ValueError, match='32-bit words'):
            fr.read_packed(8008, VDIF, 8, 1, 4004, 0, bps=1)
        with pytest.raises(ValueError, match='whole number of frames'):
            fr.read_packed(8001, VDIF, 8, 1, 4000, 0, bps=4)
        with pytest.raises(ValueError):
            fr.read_packed(8000, VDIF, 8, 1, 4000, 0, bps=4, scale=np.inf)
        assert fr.tell() == 0
        fr.seek(4002)                                       # 2 -> 8 bits: the narrower width decides, 4 samples a byte
        with pytest.raises(ValueError, match='whole bytes'):
            fr.read_packed(8000, VDIF, 8, 1, 4000, 0, bps=8)
        assert fr.tell() == 4002
        fr.seek(4004)
        got, valid = fr.read_packed(8000, VDIF, 8, 1, 4000, 0, bps=8)
        assert fr.tell() == 12004 and valid.all()
    with open_vdif() as fr:                                 # bps of the reader and no scale: the repack call, as before
        a, _ = fr.read_packed(8000, VDIF, 8, 1, 4000, 2, bps=2)
        fr.seek(0)
        b, _ = fr.read_packed(8000, VDIF, 8, 1, 4000, 2)
        import torch
        assert torch.equal(a, b)
