"""``fr.read_packed(..., scale=<array>)``: one gain per (thread, channel) in front of the
requantizer, on the packed bytes (bb_recode_frames_tables).  Small files written with the
package's own writers, read as the payloads of another geometry, against the payloads of the
file that the loop ``fw.write(fr.read(n) * scale)`` -- a broadcast torch float32 product --
makes with a stream writer of that geometry, byte for byte.  The gains are ones at which the
components' tables differ, asserted on the CPU from the file's codes and the NumPy oracle.
An invalid frame, a damaged file, the scalar routes (unchanged) and the refusals."""
import numpy as np
import pytest

from packedkit import unpack_codes
from test_convert_gpu import invalid_sample_vdif, m5b_writer, open_m5b, open_vdif
from test_requant_read_packed_gpu import fill_code, payloads_of
from test_recode_read_packed_gpu import VDIF, MARK5B, NAMES, RATE, file_payloads, vdif_writer, write_codes

pytestmark = pytest.mark.gpu

LADDER = np.float32(0.8) * np.float32(1.25) ** np.arange(8, dtype=np.float32)      # 0.8 .. 3.8
# name -> (input: nthread, nchan, bps, samples per frame, frame sets, complex, subset;
#          output: coder, nthread, nchan, bps, samples per frame; gains, in the reader's (nthread, nchan); regroup;
#          every component's table its own, reaching every output code)
CASES = {
    'vdif 8 bit 8 x 1 -> vdif 2 bit 1 x 8': ((8, 1, 8, 1000, 24, False, None), (VDIF, 1, 8, 2, 1600),
                                             LADDER.reshape(8, 1), True, True),
    'vdif 8 bit 8 x 1 -> mark5b 2 bit, 8 channels': ((8, 1, 8, 1000, 24, False, None), (MARK5B, 1, 8, 2, 5000),
                                                     LADDER.reshape(8, 1), True, True),
    'vdif 4 bit 4 x 1 -> vdif 2 bit 1 x 4': ((4, 1, 4, 2000, 16, False, None), (VDIF, 1, 4, 2, 4000),
                                             LADDER[:4].reshape(4, 1), True, False),
    'vdif 2 bit 1 x 8 -> vdif 8 bit 8 x 1': ((1, 8, 2, 2000, 8, False, None), (VDIF, 8, 1, 8, 1600),
                                             (np.float32(0.5) * np.float32(1.6) ** np.arange(8, dtype=np.float32)).reshape(1, 8),
                                             True, False),
    'vdif complex 8 bit 2 x 1 -> vdif 2 bit 1 x 2': ((2, 1, 8, 500, 32, True, None), (VDIF, 1, 2, 2, 800),
                                                     np.float32([[0.8], [2.5]]), True, False),
    'vdif 8 bit, threads 1 2 5 6 of 8 -> vdif 2 bit 1 x 4': ((8, 1, 8, 1000, 24, False, ([1, 2, 5, 6],)),
                                                             (VDIF, 1, 4, 2, 1600), LADDER[[0, 2, 4, 6]].reshape(4, 1),
                                                             True, False),
    'vdif 8 bit 8 x 1 -> vdif 4 bit 8 x 1, without regroup': ((8, 1, 8, 1000, 24, False, None), (VDIF, 8, 1, 4, 1600),
                                                              LADDER.reshape(8, 1), False, False),
}


def oracle_tables(gains, coder, bps_in, bps):
    """Table per gain as the loop's arithmetic makes it, from the NumPy oracle: (ngain, 1 << bps_in)."""
    import bb_oracle_np as orc
    levels = np.float32(orc.code_levels('vdif', bps_in))
    return np.stack([orc.encode_codes(levels * np.float32(g), NAMES[coder], bps) for g in np.ravel(gains)])


@pytest.mark.parametrize('name', sorted(CASES))
def test_payloads_are_those_of_the_file_the_loop_writes(name, tmp_path):
    import torch
    (nthread, nchan, bps_in, spf_in, nsets, cplx, subset), (coder, nthread_out, nchan_out, bps, spf), gains, regroup, \
        strict = CASES[name]
    src = write_codes(str(tmp_path / 'in.vdif'), len(name), nsets, nthread, nchan, bps_in, spf_in, cplx)
    chunk_in, chunk_out = nchan * (2 if cplx else 1), nchan_out * (2 if cplx else 1)
    # the tables are not degenerate: conditions on the gains and on the input, from the file's codes and the oracle
    tables = oracle_tables(gains, coder, bps_in, bps)
    assert len({t.tobytes() for t in tables}) >= min(4, gains.size)         # (a complex channel's (re, im) share a gain)
    present = np.unique(unpack_codes(file_payloads(src, VDIF, nthread, spf_in * chunk_in * bps_in // 8), bps_in))
    if strict:
        assert len({t.tobytes() for t in tables}) == gains.size
        for t in tables:
            assert len(set(t[present].tolist())) == 1 << bps

    kw = dict(squeeze=False) if subset is None else dict(squeeze=False, subset=subset)
    payload_out = spf * chunk_out * bps // 8
    with open_vdif(src, sample_rate=RATE, **kw) as fr:
        g = fr._packed_geometry()
        assert ((g.nslot, g.chunk) != (nthread_out, chunk_out)) == regroup and g.nslot * g.chunk == nthread_out * chunk_out
        assert tuple(gains.shape) == (g.nslot, nchan)
        fill = fill_code(np.float32(0.), coder, bps)
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
                assert tuple(x.shape) == (n, g.nslot, nchan)
                y = x * torch.from_numpy(gains).cuda()
                assert y.dtype == x.dtype
                fw.write(y.reshape((n,) + fw.sample_shape))
            want = torch.from_numpy(np.ascontiguousarray(file_payloads(path, coder, nthread_out, payload_out))).cuda()
            fr.seek(seek)
            scale = gains if k == 0 else torch.from_numpy(gains)            # (an array, and a tensor)
            got, valid = fr.read_packed(n, coder, nthread_out, nchan_out, spf, fill, bps=bps, scale=scale,
                                        **(dict(regroup=True) if regroup else {}))
            assert fr.tell() == seek + n
            assert got.dtype == torch.uint8 and tuple(got.shape) == (n // spf, nthread_out, payload_out)
            assert valid.dtype == bool and valid.all() and valid.shape == (n // spf,)
            assert torch.equal(got, want)


def test_a_mark5b_reader_takes_a_gain_per_channel(tmp_path):
    """Mark 5B has no threads: the gains broadcast to (nchan,)."""
    import torch
    gains = np.float32(0.5) * np.float32(1.6) ** np.arange(8, dtype=np.float32)
    with open_m5b() as fr:
        n = 5000
        x = fr.read(n)
        assert tuple(x.shape) == (n, 8)
        want = payloads_of((x * torch.from_numpy(gains).cuda()).reshape(n, 1, 8), 1, 8, 2500, VDIF, 4)
        fr.seek(0)
        got, valid = fr.read_packed(n, VDIF, 1, 8, 2500, fill_code(0., VDIF, 4), bps=4, scale=gains)
        assert valid.all() and torch.equal(got, want)
        fr.seek(0)
        with pytest.raises(ValueError, match=r'\(8, 1\).*\(8,\)'):
            fr.read_packed(n, VDIF, 1, 8, 2500, 0, bps=4, scale=gains.reshape(8, 1))
        assert fr.tell() == 0


def test_an_invalid_frame_is_reported_and_holds_the_fill_code(tmp_path):
    """Frame 11 of 16 of sample.vdif (frame set 1, one thread) invalid, output frames of 3200
    samples: frames 6 .. 11 draw from it.  With ``fill_value=0`` the loop encodes ``0 * gain[k]``
    there, one code whatever the gain, which fills that thread's component -- `valid` and the
    filled component as with a scalar scale."""
    import torch
    src = invalid_sample_vdif(tmp_path, 11)
    spf = 3200
    gains = (np.float32(0.5) * np.float32(1.2) ** np.arange(8, dtype=np.float32)).reshape(8, 1)
    code = fill_code(np.float32(0.), VDIF, 4)
    with open_vdif(src, fill_value=0., squeeze=False) as fr:
        at = fr.tell()
        x = fr.read(12 * spf) * torch.from_numpy(gains).cuda()
        fr.seek(at)
        want = payloads_of(x.reshape(12 * spf, 1, 8), 1, 8, spf, VDIF, 4)
        got, valid = fr.read_packed(12 * spf, VDIF, 1, 8, spf, code, bps=4, scale=gains, regroup=True)
        assert fr.tell() == at + 12 * spf
        fr.seek(at)
        _, valid_scalar = fr.read_packed(12 * spf, VDIF, 1, 8, spf, code, bps=4, scale=0.5, regroup=True)
        assert valid.tolist() == valid_scalar.tolist() == [True] * 6 + [False] * 6
        assert torch.equal(got, want)
    b = unpack_codes(got.cpu().numpy(), 4).reshape(12, spf, 8)
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
    i = next(i for i, c in enumerate(DAMAGE) if c['kind'] == 'frames')
    o = oracle('vdif', i)
    spf = 4000
    n = o.n // spf * spf
    gains = (np.float32(0.5) * np.float32(1.2) ** np.arange(8, dtype=np.float32)).reshape(8, 1)
    code = fill_code(0., VDIF, 4)
    x = torch.from_numpy(np.ascontiguousarray(o.data[:n])).cuda().reshape(n, 8, 1) * torch.from_numpy(gains).cuda()
    want = payloads_of(x.reshape(n, 1, 8), 1, 8, spf, VDIF, 4)
    with o.open('file', verify='fix') as fr:
        got, valid = quietly(fr.read_packed, n, VDIF, 1, 8, spf, code, bps=4, scale=gains, regroup=True)
        assert fr.tell() == n
        assert torch.equal(got, want)
        assert not valid.all() and valid.any()
        assert np.array_equal(valid, quietly(lambda: (fr.seek(0), fr.frames_valid(n, spf))[1]))
    error = what_read_raises(o)
    with o.open('file', verify=True) as fr:
        with pytest.raises(Exception) as met:
            quietly(fr.read_packed, n, VDIF, 1, 8, spf, code, bps=4, scale=gains, regroup=True)
        assert met.type is error and fr.tell() == 0


def test_a_scalar_scale_goes_the_way_it_went(monkeypatch):
    """Scalar `scale` and ``scale=None``: bb_requant_frames / bb_recode_frames with the one table
    of `requant_table`, never the per-component kernel -- and the bytes of equal gains in an array."""
    import torch
    from baseband_amd import kernels
    calls = []

    def spy(name):
        real = getattr(kernels, name)

        def wrapped(*a, **kw):
            calls.append((name, a, kw))
            return real(*a, **kw)
        monkeypatch.setattr(kernels, name, wrapped)

    for name in ('requant_frames', 'recode_frames', 'recode_frames_tables', 'repack_frames'):
        spy(name)
    with open_vdif() as fr:                                 # 8 threads of one 2-bit channel
        for args, kw, route, table_at in (((VDIF, 1, 8, 4000, 0), dict(bps=4, scale=0.5, regroup=True), 'recode_frames', 10),
                                          ((VDIF, 8, 1, 4000, 0), dict(bps=4, scale=0.5), 'requant_frames', 8),
                                          ((VDIF, 8, 1, 4000, 0), dict(bps=4), 'requant_frames', 8),
                                          ((VDIF, 1, 8, 4000, 2), dict(), 'repack_frames', None)):
            del calls[:]
            fr.seek(0)
            a, _ = fr.read_packed(8000, *args, **kw)
            assert calls and {c[0] for c in calls} == {route}
            if table_at is not None:
                table = kernels.requant_table(VDIF, 2, VDIF, 4, kw.get('scale'))
                assert all(np.array_equal(c[1][table_at], table) for c in calls)
            if 'scale' in kw:
                del calls[:]
                fr.seek(0)
                b, _ = fr.read_packed(8000, *args, **dict(kw, scale=np.full((8, 1), kw['scale'])))
                assert {c[0] for c in calls} == {'recode_frames_tables'}
                assert torch.equal(a, b)


def test_what_the_tables_route_does_not_take():
    gains = LADDER.reshape(8, 1)
    with open_vdif() as fr:                                 # 8 threads of one 2-bit channel
        for bad in (LADDER[:4], LADDER.reshape(1, 8)[:, :7], np.ones((2, 8, 1), np.float32), np.ones((8, 2), np.float32)):
            with pytest.raises(ValueError, match=r'scale of shape \({}.*reader\'s \(8, 1\)'
                               .format(', '.join(map(str, bad.shape)))):
                fr.read_packed(8000, VDIF, 1, 8, 4000, 0, bps=4, scale=bad, regroup=True)
        for bad in (np.nan, np.inf, -np.inf):
            g = gains.copy()
            g[3, 0] = bad
            with pytest.raises(ValueError, match='finite'):
                fr.read_packed(8000, VDIF, 1, 8, 4000, 0, bps=4, scale=g, regroup=True)
        with pytest.raises(NotImplementedError, match='regroup=True'):      # a structure change: refused with the same words
            fr.read_packed(8000, VDIF, 1, 8, 4000, 0, bps=4, scale=gains)
        with pytest.raises(NotImplementedError, match='thread structure'):
            fr.read_packed(8000, VDIF, 1, 8, 4000, 0, scale=gains)
        with pytest.raises(NotImplementedError, match=r'number of components \(8 x 1 codes -> 1 x 4\)'):
            fr.read_packed(8000, VDIF, 1, 4, 4000, 0, bps=4, scale=gains, regroup=True)
        assert fr.tell() == 0
        # gains that broadcast: one row for all threads, a scalar in an array
        import torch
        a, _ = fr.read_packed(8000, VDIF, 1, 8, 4000, 0, bps=4, scale=np.float32([0.5]), regroup=True)
        fr.seek(0)
        b, _ = fr.read_packed(8000, VDIF, 1, 8, 4000, 0, bps=4, scale=0.5, regroup=True)
        assert torch.equal(a, b)
