"""``fr.read_packed(..., bps=, scale=, regroup=True)`` where the thread structure changes as well
as the sample width (bb_recode_frames): small files written with the package's own writers, read
as the payloads of another geometry, against the payloads of the file that the loop
``fw.write(fr.read(n) * scale)`` makes with a stream writer of that geometry -- byte for
byte.  `valid` and the offset agree with the equal-structure path, a damaged file is
answered as ``read()`` answers it, mismatched component counts are refused by name, and
without ``regroup=True`` the request is refused as it was before."""
import numpy as np
import pytest

from packedkit import unpack_codes
from test_convert_gpu import T_M5B, invalid_sample_vdif, m5b_writer, open_vdif
from test_requant_read_packed_gpu import fill_code, payloads_of

pytestmark = pytest.mark.gpu

VDIF, MARK5B = 0, 1
NAMES = {VDIF: 'vdif', MARK5B: 'mark5b'}
RATE = 32e6


def _bb():
    import baseband_amd
    return baseband_amd


def vdif_writer(path, nthread, nchan, bps, spf, complex_data=False):
    return _bb().vdif.open(path, 'ws', sample_rate=RATE, nthread=nthread, nchan=nchan, edv=0, bps=bps,
                           complex_data=complex_data, samples_per_frame=spf, station='cv', time=T_M5B)


def write_codes(path, seed, nsets, nthread, nchan, bps, spf, complex_data=False):
    """A VDIF file of `nsets` frame sets whose samples are the levels of uniformly random codes."""
    import bb_oracle_np as orc
    import torch
    rng = np.random.default_rng(seed)
    n = nsets * spf
    codes = rng.integers(0, 1 << bps, (n, nthread, nchan) + ((2,) if complex_data else ()))
    x = torch.from_numpy(np.float32(orc.code_levels('vdif', bps))[codes])
    x = torch.view_as_complex(x) if complex_data else x
    with vdif_writer(path, nthread, nchan, bps, spf, complex_data) as fw:
        fw.write(x.cuda().reshape((n,) + fw.sample_shape))
    return path


def file_payloads(path, coder, nthread, payload):
    """The payload bytes of a file of this package's writers: (frames, threads, payload)."""
    header = 16 if coder == MARK5B else 32                  # (Mark 5B; VDIF with EDV 0)
    raw = np.fromfile(path, np.uint8)
    return raw.reshape(-1, nthread, header + payload)[:, :, header:]


# name -> (input: nthread, nchan, bps, samples per frame, frame sets, complex, subset;
#          output: coder, nthread, nchan, bps, samples per frame; scale)
CASES = {
    'vdif 8 bit 8 x 1 -> vdif 2 bit 1 x 8': ((8, 1, 8, 1000, 24, False, None), (VDIF, 1, 8, 2, 1600), 0.9),
    'vdif 8 bit 8 x 1 -> mark5b 2 bit, 8 channels': ((8, 1, 8, 1000, 24, False, None), (MARK5B, 1, 8, 2, 5000), 0.9),
    'vdif 4 bit 4 x 1 -> vdif 2 bit 1 x 4': ((4, 1, 4, 2000, 16, False, None), (VDIF, 1, 4, 2, 4000), 1.5),
    'vdif 2 bit 1 x 8 -> vdif 8 bit 8 x 1': ((1, 8, 2, 2000, 8, False, None), (VDIF, 8, 1, 8, 1600), 0.5),
    'vdif complex 8 bit 2 x 1 -> vdif 2 bit 1 x 2': ((2, 1, 8, 500, 32, True, None), (VDIF, 1, 2, 2, 800), 0.9),
    'vdif 8 bit, threads 1 2 5 6 of 8 -> vdif 2 bit 1 x 4': ((8, 1, 8, 1000, 24, False, ([1, 2, 5, 6],)),
                                                             (VDIF, 1, 4, 2, 1600), None),
}


@pytest.mark.parametrize('name', sorted(CASES))
def test_payloads_are_those_of_the_file_the_loop_writes(name, tmp_path):
    """The expected bytes: ``fw.write(fr.read(n) * scale)`` with a stream writer of the target
    geometry, its file's payloads.  The scale is one at which the input's codes reach every
    output code (where the output is the narrower side; every input code a code of its own
    where it is the wider one): asserted on the CPU from the file's codes and the levels."""
    import bb_oracle_np as orc
    import torch
    (nthread, nchan, bps_in, spf_in, nsets, cplx, subset), (coder, nthread_out, nchan_out, bps, spf), scale = CASES[name]
    src = write_codes(str(tmp_path / 'in.vdif'), len(name), nsets, nthread, nchan, bps_in, spf_in, cplx)
    chunk_in, chunk_out = nchan * (2 if cplx else 1), nchan_out * (2 if cplx else 1)
    # every output code occurs: a condition on the input
    present = np.unique(unpack_codes(file_payloads(src, VDIF, nthread, spf_in * chunk_in * bps_in // 8), bps_in))
    gain = np.float32(1.) if scale is None else np.float32(scale)
    reached = orc.encode_codes(np.float32(orc.code_levels('vdif', bps_in))[present] * gain, NAMES[coder], bps)
    assert len(set(reached.tolist())) == 1 << min(bps, bps_in)

    kw = {} if subset is None else dict(subset=subset)
    payload_out = spf * chunk_out * bps // 8
    with open_vdif(src, sample_rate=RATE, **kw) as fr:
        g = fr._packed_geometry()
        assert (g.nslot, g.chunk) != (nthread_out, chunk_out) and g.nslot * g.chunk == nthread_out * chunk_out
        fill = fill_code(np.float32(fr.fill_value) * gain, coder, bps)
        for k, seek in enumerate((0, spf)):                     # the whole file, and from inside it to the end
            n = (fr.shape[0] - seek) // spf * spf
            assert n > 0
            # the loop, through a stream writer of the target geometry
            path = str(tmp_path / 'loop{}'.format(k))
            fw = (m5b_writer(path, nchan_out) if coder == MARK5B
                  else vdif_writer(path, nthread_out, nchan_out, bps, spf, cplx))
            with fw:
                fr.seek(seek)
                x = fr.read(n)
                fw.write((x if scale is None else x * float(gain)).reshape((n,) + fw.sample_shape))
            want = torch.from_numpy(np.ascontiguousarray(file_payloads(path, coder, nthread_out, payload_out))).cuda()
            fr.seek(seek)
            got, valid = fr.read_packed(n, coder, nthread_out, nchan_out, spf, fill, bps=bps, scale=scale, regroup=True)
            assert fr.tell() == seek + n
            assert got.dtype == torch.uint8 and tuple(got.shape) == (n // spf, nthread_out, payload_out)
            assert valid.dtype == bool and valid.all() and valid.shape == (n // spf,)
            assert torch.equal(got, want)
            assert len(np.unique(unpack_codes(got.cpu().numpy(), bps))) == 1 << min(bps, bps_in)


def test_valid_and_the_offset_agree_with_the_equal_structure_path(tmp_path):
    """Frame 11 of 16 of sample.vdif (frame set 1, one thread) invalid, output frames of 3200
    samples: frames 6 .. 11 draw from it.  The fill value 3.0 times the scale 0.5 is 1.5,
    whose 4-bit code fills that thread's component there -- in the one thread of 8 channels
    as in the 8 threads of one."""
    import torch
    src = invalid_sample_vdif(tmp_path, 11)
    spf, scale = 3200, 0.5
    code = fill_code(np.float32(3.) * np.float32(scale), VDIF, 4)
    with open_vdif(src, fill_value=3.) as fr:
        at = fr.tell()
        x = fr.read(12 * spf).reshape(12 * spf, 1, 8).float() * scale
        fr.seek(at)
        want = payloads_of(x, 1, 8, spf, VDIF, 4)
        same, valid_same = fr.read_packed(12 * spf, VDIF, 8, 1, spf, code, bps=4, scale=scale)   # bb_requant_frames
        assert fr.tell() == at + 12 * spf
        fr.seek(at)
        got, valid = fr.read_packed(12 * spf, VDIF, 1, 8, spf, code, bps=4, scale=scale,
                                    regroup=True)                                                # bb_recode_frames
        assert fr.tell() == at + 12 * spf
        assert valid.tolist() == valid_same.tolist() == [True] * 6 + [False] * 6
        assert torch.equal(got, want)
    # the same codes, thread t of the one a channel of the other
    a = unpack_codes(same.cpu().numpy(), 4).reshape(12, 8, spf)
    b = unpack_codes(got.cpu().numpy(), 4).reshape(12, spf, 8)
    assert np.array_equal(a.transpose(0, 2, 1), b)
    filled = (b == code).all(1)                               # (output frame, channel): nothing but the fill code
    channel = [c for c in range(8) if filled[7, c]]
    assert len(channel) == 1
    mask = np.zeros((12, 8), bool)
    mask[7:, channel[0]] = True
    assert np.array_equal(filled, mask)
    assert (b[6, 800:, channel[0]] == code).all() and not (b[6, :800, channel[0]] == code).all()


def test_a_damaged_file_is_answered_as_read_answers_it():
    """A file that lost frames: under ``verify='fix'`` the payloads are those of the loop on the
    repaired read, with the fill code in the holes; under ``verify=True`` the call raises
    what the read raises and the offset stays."""
    import torch
    from test_packed_damaged_gpu import oracle, quietly, what_read_raises
    from test_corrupt_gpu import CASES as DAMAGE
    picks = [next(i for i, c in enumerate(DAMAGE) if c['kind'] == kind) for kind in ('frames', 'bytes')]
    for i in picks:                                         # frames dropped; bytes removed
        o = oracle('vdif', i)
        spf, scale = 4000, 0.5
        n = o.n // spf * spf
        code = fill_code(0., VDIF, 4)
        x = torch.from_numpy(np.ascontiguousarray(o.data[:n])).cuda().reshape(n, 1, 8) * scale
        want = payloads_of(x, 1, 8, spf, VDIF, 4)
        with o.open('file', verify='fix') as fr:
            got, valid = quietly(fr.read_packed, n, VDIF, 1, 8, spf, code, bps=4, scale=scale, regroup=True)
            assert fr.tell() == n
            assert torch.equal(got, want)
            assert not valid.all() and valid.any()
            assert np.array_equal(valid, quietly(lambda: (fr.seek(0), fr.frames_valid(n, spf))[1]))
        error = what_read_raises(o)
        with o.open('file', verify=True) as fr:
            with pytest.raises(Exception) as met:
                quietly(fr.read_packed, n, VDIF, 1, 8, spf, code, bps=4, scale=scale, regroup=True)
            assert met.type is error and fr.tell() == 0


def test_what_the_recode_route_does_not_take():
    import torch
    with open_vdif() as fr:                                 # 8 threads of one 2-bit channel
        for nthread, nchan in ((1, 4), (4, 1), (2, 8), (16, 1)):
            with pytest.raises(NotImplementedError, match=r'number of components \(8 x 1 codes -> {} x {}\)'
                               .format(nthread, nchan)):
                fr.read_packed(8000, VDIF, nthread, nchan, 4000, 0, bps=4, regroup=True)
            with pytest.raises(NotImplementedError, match='number of components'):
                fr.read_packed(8000, VDIF, nthread, nchan, 4000, 0, scale=0.5, regroup=True)
        with pytest.raises(ValueError, match='32-bit words'):
            fr.read_packed(8002, VDIF, 1, 8, 4001, 0, bps=1, regroup=True)
        with pytest.raises(ValueError, match='whole number of frames'):
            fr.read_packed(8001, VDIF, 1, 8, 4000, 0, bps=4, regroup=True)
        assert fr.tell() == 0
        fr.seek(4002)                                       # 8 x 1 at 2 bits: four samples to a byte of a thread
        with pytest.raises(ValueError, match='whole bytes'):
            fr.read_packed(8000, VDIF, 1, 8, 4000, 0, bps=8, regroup=True)
        assert fr.tell() == 4002
        fr.seek(4004)
        got, valid = fr.read_packed(8000, VDIF, 1, 8, 4000, 0, bps=8, regroup=True)
        assert fr.tell() == 12004 and valid.all() and tuple(got.shape) == (2, 1, 32000)
    with open_vdif() as fr:                                 # without regroup=True: refused, as it always was
        with pytest.raises(NotImplementedError, match='thread structure'):
            fr.read_packed(8000, VDIF, 1, 8, 4000, 0, bps=4)
        with pytest.raises(NotImplementedError, match='regroup=True'):
            fr.read_packed(8000, VDIF, 1, 8, 4000, 0, scale=0.5)
        assert fr.tell() == 0
        a, _ = fr.read_packed(8000, VDIF, 8, 1, 4000, 0, bps=4)                  # equal structures: the flag changes nothing
        fr.seek(0)
        b, _ = fr.read_packed(8000, VDIF, 8, 1, 4000, 0, bps=4, regroup=True)
        assert torch.equal(a, b)
    with open_vdif() as fr:                                 # no width and no scale: the repack call, as before
        a, _ = fr.read_packed(8000, VDIF, 1, 8, 4000, 2)
        fr.seek(0)
        b, _ = fr.read_packed(8000, VDIF, 1, 8, 4000, 2, bps=2)
        fr.seek(0)
        c, _ = fr.read_packed(8000, VDIF, 1, 8, 4000, 2, scale=1.0, regroup=True)   # the table of scale 1: the same bytes
        assert torch.equal(a, b) and torch.equal(a, c)
