"""The caller's memory before and after a call: what a stream writer keeps of
the samples it was given, and what a reader's results share with the reader.

* Every stream writer encodes whole frames at once and keeps what does not
  fill one for the next ``write()`` or ``close()``.  A caller who refills one
  device buffer in place between writes (``buf.copy_(next); fw.write(buf)``)
  or changes a tensor right after handing it over must get the samples as they
  were at the call: the file equals the one written from fresh NumPy arrays
  (the path tests/test_encode_gpu.py pins against the reference's writers).
* A result changed in place must not change any later result -- neither the
  views of the decoded read-ahead window (results of 1 MiB and more) nor the
  copies cut out of it (smaller ones); ``read(out=buf)`` with one buffer
  reused; a resident reader that repairs damage leaves the caller's bytes as
  they were."""
import hashlib
import io
import os
import warnings

import numpy as np
import pytest

import bb_oracle_np as orc
from conftest import golden_path, bits_equal

pytestmark = pytest.mark.gpu

T0 = np.datetime64('2021-03-04T05:06:07')


def _open_writer(kind, d, tag):
    """(stream writer, names of every file it writes) for one writer kind;
    frames are a few KiB to a few MiB."""
    import baseband_amd as bb
    p = os.path.join(d, tag)
    if kind.startswith('vdif'):
        nthread = 8 if kind.startswith('vdif8') else 1
        fw = bb.vdif.open(p + '.vdif', 'ws', sample_rate=1024 * 100., nthread=nthread, edv=0, bps=2,
                          nchan=4 if nthread == 1 else 1, samples_per_frame=1024,
                          complex_data=kind.endswith('cplx'), station='ab', time=T0, squeeze=False)
        return fw, [p + '.vdif']
    if kind == 'mark5b':
        fw = bb.mark5b.open(p + '.m5b', 'ws', sample_rate=32e6, nchan=8, bps=2,
                            time=np.datetime64('2014-06-13T05:30:01'))
        return fw, [p + '.m5b']
    if kind == 'mark4':
        fw = bb.mark4.open(p + '.m4', 'ws', sample_rate=32e6, ntrack=32, fanout=4, bps=2,
                           time=np.datetime64('2015-03-02T04:05:06.25'))
        return fw, [p + '.m4']
    if kind == 'dada':
        from baseband_amd.dada.header import DADAHeader
        h0 = DADAHeader.fromvalues(time=T0, offset=0., sample_rate=16e6, bps=8, complex_data=True,
                                   npol=2, nchan=1, payload_nbytes=4096 * 4, start_time=T0,
                                   telescope='GMRT')
        return bb.dada.open(p + '.dada', 'ws', header0=h0), [p + '.dada']
    if kind == 'guppi':
        g = np.load(golden_path('block_writer_cases.npz'))
        h0 = bb.guppi.GUPPIHeader.fromfile(io.BytesIO(g['guppi_cf_file'].tobytes()))
        return bb.guppi.open(p + '.raw', 'ws', header0=h0), [p + '.raw']
    if kind == 'gsb_rawdump':
        ts, raw = p + '.timestamp', p + '.dat'
        fw = bb.gsb.open(ts, 'ws', raw=raw, time=T0, samples_per_frame=4096, sample_rate=1e6)
        return fw, [ts, raw]
    assert kind == 'gsb_phased'
    ts = p + '.timestamp'
    raws = [[p + '.%d%d.dat' % (pol, part) for part in range(2)] for pol in range(2)]
    fw = bb.gsb.open(ts, 'ws', raw=raws, header_mode='phased', time=T0, seq_nr=9998, mem_block=6,
                     samples_per_frame=256, nchan=16, sample_rate=1e6)
    return fw, [ts] + raws[0] + raws[1]


WRITERS = ['vdif1_real', 'vdif1_cplx', 'vdif8_real', 'vdif8_cplx', 'mark5b', 'mark4',
           'dada', 'guppi', 'gsb_rawdump', 'gsb_phased']


def _plan(spf):
    """(piece length, valid): exactly one frame on a frame boundary, 1.5 frames
    from a boundary (the whole piece is the pending block: its tail is a view
    of the caller's tensor), less than a frame, whole frames and more that
    start inside a frame, pieces flagged invalid, and a partial last frame
    that close() pads.  The frame that holds the tail of the 1.5 frames is
    valid: Mark 5B replaces the payload of an invalid frame with a pattern."""
    return [(spf, True), (spf + spf // 2, True), (spf // 3, True), (spf, True),
            (spf // 3 + 1, False), (2 * spf + spf // 4, True), (spf // 2 + 3, False)]


def _samples(fw, n, seed):
    """Samples for writer `fw`: off-level values (rounding and clipping) in
    the encoders' useful range."""
    rng = np.random.default_rng(seed)
    shape = (n,) + tuple(fw.sample_shape)
    scale = 30. if fw.bps >= 4 else 1.7
    x = (rng.standard_normal(shape) * scale).astype(np.float32)
    if fw.complex_data:
        x = (x + 1j * (rng.standard_normal(shape) * scale)).astype(np.complex64)
    return x


def _write_file(kind, d, tag, feed):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')             # (the padded last frame)
        fw, names = _open_writer(kind, d, tag)
        with fw:
            spf = fw.samples_per_frame
            plan = _plan(spf)
            feed(fw, plan, _samples(fw, sum(n for n, _ in plan), seed=len(kind)))
    return [open(n, 'rb').read() for n in names]


def _from_numpy(fw, plan, data):
    a = 0
    for n, ok in plan:
        fw.write(data[a:a + n].copy(), valid=ok)
        a += n


def _reused_buffer(fw, plan, data):
    """One device buffer, refilled in place (device to device: nothing syncs)
    before every write."""
    import torch
    src = torch.from_numpy(data).cuda()
    buf = torch.empty((max(n for n, _ in plan),) + src.shape[1:], dtype=src.dtype, device='cuda')
    a = 0
    for n, ok in plan:
        buf[:n].copy_(src[a:a + n])
        fw.write(buf[:n], valid=ok)
        a += n


def _changed_after_write(fw, plan, data):
    """A fresh tensor per write, changed on the same stream right after
    write() returns, no sync in between."""
    import torch
    src = torch.from_numpy(data).cuda()
    a = 0
    for n, ok in plan:
        piece = src[a:a + n].clone()
        fw.write(piece, valid=ok)
        piece.mul_(-3.).add_(0.5)
        a += n
    src.zero_()


@pytest.mark.parametrize('feed', ['reused_buffer', 'changed_after_write'])
@pytest.mark.parametrize('kind', WRITERS)
def test_stream_writer_keeps_samples_as_they_were_at_the_call(kind, feed, tmp_path):
    want = _write_file(kind, str(tmp_path), 'np', _from_numpy)
    got = _write_file(kind, str(tmp_path), 'dev',
                      _reused_buffer if feed == 'reused_buffer' else _changed_after_write)
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w), (k, len(g), len(w))
        if g != w:
            diff = np.nonzero(np.frombuffer(g, np.uint8) != np.frombuffer(w, np.uint8))[0]
            raise AssertionError("{} file {}: {} bytes differ from the NumPy-fed file, first at byte {}"
                                 .format(kind, k, diff.size, int(diff[0])))


def test_whole_frame_writes_keep_nothing_of_the_caller(tmp_path):
    """What stays pending after write() is the writer's own memory; pieces of
    whole frames leave nothing pending."""
    import torch
    fw, _ = _open_writer('vdif1_real', str(tmp_path), 'w')
    spf = fw.samples_per_frame
    x = torch.randn((3 * spf + spf // 2,) + fw.sample_shape, device='cuda')
    lo, hi = x.data_ptr(), x.data_ptr() + x.numel() * x.element_size()
    for part in (x[:spf], x[spf:spf + spf // 2], x[spf + spf // 2:]):
        fw.write(part)
        for t, _ in fw._pending:
            assert not lo <= t.data_ptr() < hi, "pending samples alias the caller's tensor"
    assert fw._npending == spf // 2
    fw.write(torch.zeros((spf - spf // 2,) + fw.sample_shape, device='cuda'))
    assert fw._pending == [] and fw._npending == 0
    fw.close()


# ---- readers ------------------------------------------------------------------
NSETS = 600
SPF = 32000


@pytest.fixture(scope='module')
def vdif_file(tmp_path_factory):
    """600 frames of single-thread 2-bit VDIF (4.8 MB) on disk, and the
    oracle's decode of it."""
    from baseband_amd import synth
    image, h0 = synth.random_vdif(41, NSETS, payload_nbytes=8000, frame_rate=1000)
    path = str(tmp_path_factory.mktemp('cb') / 'r.vdif')
    image.tofile(path)
    exp, _ = orc.vdif_read(image, frame_rate=1000)
    return path, image, exp.reshape(exp.shape[0], -1)


def _open_reader(path, **kw):
    from baseband_amd import vdif
    return vdif.open(path, 'rs', sample_rate=SPF * 1000., squeeze=False, **kw)


def _check(got, exp, lo, what):
    g = got.cpu().numpy().reshape(got.shape[0], -1) if hasattr(got, 'cpu') else got.reshape(got.shape[0], -1)
    assert bits_equal(g, exp[lo:lo + g.shape[0]]), what


@pytest.mark.parametrize('count', [10 * SPF, SPF // 4], ids=['view_1MiB_plus', 'copy_below_1MiB'])
def test_results_changed_in_place_change_no_later_result(vdif_file, count):
    import torch
    path, image, exp = vdif_file
    with _open_reader(path) as fh:
        results = []
        for k in range(12):
            lo = fh.tell()
            got = fh.read(count)
            results.append((lo, got.clone()))
            got.fill_(12345.)                   # the caller's result, changed in place
            got.view(torch.int32)[::7] = -1
            del got
        # the read-ahead served these from a decoded window: views of it from 1 MiB on, copies below
        probe = fh.read(count)
        assert fh._decoded is not None
        window = fh._decoded[2]
        shares = probe.untyped_storage().data_ptr() == window.untyped_storage().data_ptr()
        assert shares == (count * 4 >= fh.decode_ahead_copy_below), (count, shares)
        results.append((fh.tell() - count, probe.clone()))
        probe.zero_()
        for lo, got in results:
            _check(got, exp, lo, ('sequential', lo))
        # back to a range read before: the same samples, not what the caller left there
        for lo in (results[3][0], results[10][0], 0):
            fh.seek(lo)
            _check(fh.read(count), exp, lo, ('again', lo))
            _check(fh.read(count), exp, lo + count, ('after again', lo))


@pytest.mark.parametrize('sizes', [(SPF // 4, SPF // 4 + 3), (10 * SPF, 10 * SPF + 17)],
                         ids=['small', 'large'])
def test_read_into_one_reused_out_buffer(vdif_file, sizes):
    import torch
    path, image, exp = vdif_file
    buf = torch.empty((max(sizes), 1, 1), dtype=torch.float32, device='cuda')
    kept = []
    with _open_reader(path) as fh:
        for k in range(14):
            n = sizes[k % 2]
            lo = fh.tell()
            out = fh.read(out=buf[:n])
            assert out.data_ptr() == buf.data_ptr()
            kept.append((lo, buf[:n].clone()))          # queued: no sync between the reads
            buf.fill_(-1.)
        fh.seek(5 * SPF + 3)
        kept.append((5 * SPF + 3, fh.read(out=buf[:sizes[1]]).clone()))
    for lo, got in kept:
        _check(got, exp, lo, lo)


@pytest.mark.parametrize('damage', ['invariant', 'misplaced'])
def test_resident_reader_repairs_without_touching_the_callers_bytes(damage):
    """verify='fix' over damaged headers in a device tensor the caller owns:
    the read relocates frames and fills what it cannot use; the bytes of the
    tensor are those the caller gave (digest before and after)."""
    import torch
    from baseband_amd import synth, vdif
    nsets = 2200                                        # 17.7 MB: the side-stream scan
    image, h0 = synth.random_vdif(23, nsets, payload_nbytes=8000, frame_rate=1000)
    fn = h0.frame_nbytes
    w = image.view('<u4').reshape(nsets, fn // 4)
    if damage == 'invariant':
        w[500, 2] ^= 0x10
    else:
        w[900, 1] = (w[900, 1] & 0xff000000) | ((int(w[900, 1]) & 0xffffff) + 3)
    dev = torch.from_numpy(image.copy()).cuda()
    before = hashlib.sha256(dev.cpu().numpy().tobytes()).hexdigest()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        with vdif.open(dev, 'rs', sample_rate=SPF * 1000., verify='fix') as fh:
            got = fh.read()
            fh.seek(400 * SPF + 5)
            part = fh.read(600 * SPF)
    assert any('problem loading frame' in str(c.message) for c in caught)
    torch.cuda.synchronize()
    assert hashlib.sha256(dev.cpu().numpy().tobytes()).hexdigest() == before
    assert np.array_equal(dev.cpu().numpy(), image)
    bad = 500 if damage == 'invariant' else 900
    flat = got.cpu().numpy().reshape(-1)
    assert np.all(flat[bad * SPF:(bad + 1) * SPF] == 0)
    for k in (0, bad - 1, bad + 1, nsets - 1):
        good = orc.decode_flat(image.reshape(nsets, fn)[k, 32:], 'vdif', 2)
        assert bits_equal(flat[k * SPF:(k + 1) * SPF], good), k
    assert bits_equal(part.cpu().numpy().reshape(-1), flat[400 * SPF + 5:1000 * SPF + 5])
