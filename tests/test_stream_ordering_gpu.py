"""Every wait between streams and threads of the asynchronous read and write
paths, checked with one stream made late on purpose.

`stall(stream, ms)` queues a spin kernel (``torch.cuda._sleep``, calibrated
to milliseconds once per session with events) on a stream; the work queued
behind it runs that much later.  Each test asserts that its stall was still
running when the calls under test had returned (`assert_late`) -- where a call
reads a verdict back on the caller's stream, the host waits there and the
test asserts the stall at the moment each call was issued.  The results are
compared bit for bit with the NumPy oracle's decode of the same bytes, files
with the same samples written synchronously (``staging._WRITE_ASYNC =
False``).  A missing wait shows as stale or foreign samples."""
import warnings

import numpy as np
import pytest

import bb_oracle_np as orc

pytestmark = pytest.mark.gpu

STEP_MS = 15            # stall in front of each call of a burst


# ---- the stall ------------------------------------------------------------------
_cycles_per_ms = []


def cycles_per_ms():
    """Spin cycles of ``torch.cuda._sleep`` per millisecond, measured once."""
    import torch
    if not _cycles_per_ms:
        n = 1 << 16
        torch.cuda._sleep(n)                            # (first launch: module load)
        torch.cuda.synchronize()
        while True:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            torch.cuda._sleep(n)
            b.record()
            b.synchronize()
            ms = a.elapsed_time(b)
            if ms >= 10. or n >= 1 << 40:
                break
            n = int(n * min(64., max(2., 20. / max(ms, 1e-3))))
        _cycles_per_ms.append(n / ms)
    return _cycles_per_ms[0]


def _fallback_stall(ms):
    """Without ``torch.cuda._sleep``: a chain of elementwise ops on a scratch
    tensor, calibrated the same way."""
    import torch
    x = torch.ones(1 << 22, device='cuda')
    if not _cycles_per_ms:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(64):
            x.mul_(1.0000001)
        b.record()
        b.synchronize()
        _cycles_per_ms.append(64 / a.elapsed_time(b))
    for _ in range(max(1, int(ms * _cycles_per_ms[0]))):
        x.mul_(1.0000001)


def stall(stream, ms=STEP_MS):
    """Queue `ms` milliseconds of spinning on `stream` (at most 100)."""
    import torch
    assert 0 < ms <= 100
    with torch.cuda.stream(stream):
        if hasattr(torch.cuda, '_sleep'):
            torch.cuda._sleep(max(1, int(ms * cycles_per_ms())))
        else:
            _fallback_stall(ms)


def assert_late(stream, what):
    assert not stream.query(), (
        "the stall on {} was over before {}: the test proved nothing".format(stream, what))


def test_stall_helper_is_calibrated():
    import torch
    s = torch.cuda.Stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(s)
    stall(s, 40)
    b.record(s)
    assert_late(s, 'the host looked')
    b.synchronize()
    ms = a.elapsed_time(b)
    print("stall: {:.0f} cycles per ms; 40 ms asked, {:.1f} ms measured".format(cycles_per_ms(), ms))
    assert 20. <= ms <= 100., ms


# ---- stream images in HBM and their oracle decodes -------------------------------------
class Img:
    """A file image, its reader, its oracle decode (on the device, one row
    per sample) and its geometry."""

    def __init__(self, fmt):
        import torch
        import baseband_amd as bb
        from baseband_amd import synth
        self.fmt = fmt
        if fmt in ('vdif1', 'vdif1_item'):
            big = fmt == 'vdif1_item'               # frames of 16 KB: a 16 MiB request has < 2048 records
            self.nframes = 1300 if big else 2400
            pn = 16000 if big else 8000
            image, h0 = synth.random_vdif(51, self.nframes, bps=8, payload_nbytes=pn, frame_rate=1000)
            self.spf, self.fn = h0.samples_per_frame, h0.frame_nbytes
            self.op, self.kw = bb.vdif.open, dict(sample_rate=self.spf * 1000.)
            exp, _ = orc.vdif_read(image, frame_rate=1000)
        elif fmt == 'vdif8':
            self.nframes = 2400                     # frame sets
            image, h0 = synth.random_vdif(52, self.nframes, nthread=8, bps=8, payload_nbytes=1000,
                                          frame_rate=1000, thread_order=[1, 3, 5, 7, 0, 2, 4, 6])
            self.spf, self.fn = h0.samples_per_frame, 8 * h0.frame_nbytes
            self.op, self.kw = bb.vdif.open, dict(sample_rate=self.spf * 1000.)
            exp, _ = orc.vdif_read(image, frame_rate=1000)
        elif fmt == 'mark5b':
            self.nframes = 2400
            rng = np.random.default_rng(8)
            words = rng.integers(0, 2 ** 32, (self.nframes, 2504), dtype=np.uint64).astype(np.uint32)
            from baseband_amd.mark5b.header import frame_header_words
            words[:, :4] = frame_header_words(np.datetime64('2014-06-13T05:30:01'), 6400, 0, self.nframes)
            image = words.view(np.uint8).reshape(-1)
            self.spf, self.fn = 5000, 10016
            self.op, self.kw = bb.mark5b.open, dict(kday=56000, nchan=8, bps=2, sample_rate=6400 * 5000.)
            exp, _ = orc.mark5b_read(image, 8, 2, frame_rate=6400)
        else:
            assert fmt == 'mark4'
            self.nframes = 130
            image, h0 = synth.random_mark4(3, self.nframes, ntrack=64, fanout=4, frame_rate=400)
            self.spf, self.fn = 80000, 160000
            self.op, self.kw = bb.mark4.open, dict(ntrack=64, decade=2010, sample_rate=400 * 80000.)
            exp, _ = orc.mark4_read(image, 64, frame_rate=400)
        self.image = np.ascontiguousarray(image)
        exp = np.ascontiguousarray(exp)
        self.exp = torch.from_numpy(exp.view(np.float32).reshape(exp.shape[0], -1)).cuda()
        self.dev = torch.from_numpy(self.image.copy()).cuda()
        # (frames in a request of >= 16 MiB: the scan goes to the side stream)
        self.nmin = -(-(16 << 20) // self.fn) + 2
        if fmt == 'mark5b':
            self.nmin = 2050                        # (2048 records and more: the verdict comes on the side stream)
        # verdicts of fewer than 2048 scan records are read on the caller's stream
        self.syncs = (self.nmin * self.fn // {'vdif8': 1032}.get(fmt, self.fn)) < 2048

    def open(self, src=None, **kw):
        return self.op(self.dev if src is None else src, 'rs', squeeze=False, **dict(self.kw, **kw))

    def plan(self, seed, n):
        """`n` requests (first frame, frames) of mixed sizes, all >= 16 MiB."""
        rng = np.random.default_rng(seed)
        out = []
        for _ in range(n):
            nf = int(rng.integers(self.nmin, self.nmin + (self.nframes - self.nmin) // 2))
            out.append((int(rng.integers(0, self.nframes - nf - 1)), nf))
        return out

    def mismatch(self, got, f0):
        """Device count of samples that differ from the oracle (queued on the
        current stream, no sync)."""
        import torch
        want = self.exp[f0 * self.spf:f0 * self.spf + got.shape[0]]
        return (got.reshape(got.shape[0], -1).view(torch.int32) != want.view(torch.int32)).sum()


@pytest.fixture(scope='module')
def img():
    made = {}

    def get(fmt):
        if fmt not in made:
            made[fmt] = Img(fmt)
        return made[fmt]
    yield get
    made.clear()                # (the images and oracle decodes leave the device with the module)


def _warm(fh, im):
    """One read of the largest size: the side stream exists, the scratch sets
    are large enough for every later request."""
    import torch
    fh.seek(0)
    fh.read((im.nmin + (im.nframes - im.nmin) // 2) * im.spf)
    torch.cuda.synchronize()
    assert fh._scan_stream is not None, "the request did not take the side-stream scan"


def _all_zero(counts, plan):
    import torch
    torch.cuda.synchronize()
    bad = [(k, p, int(c)) for k, (p, c) in enumerate(zip(plan, counts)) if int(c)]
    assert not bad, "reads that differ from the oracle (k, (frame, frames), samples): {}".format(bad[:4])


# ---- 1. side-stream scans of resident bytes --------------------------------------
@pytest.mark.parametrize('fmt', ['vdif1', 'vdif8', 'mark5b', 'mark4'])
def test_scratch_sets_rotate_under_a_late_caller(img, fmt):
    """2 x _NSCRATCH + 1 reads of mixed sizes, each behind a stall of the
    caller's stream: the scans of later requests refill scratch sets whose
    decodes have not run yet unless they wait for them."""
    import torch
    from baseband_amd import kernels
    im = img(fmt)
    cur = torch.cuda.current_stream()
    plan = im.plan(3, 2 * kernels._NSCRATCH + 1)
    counts = []
    with im.open() as fh:
        _warm(fh, im)
        for k, (f0, nf) in enumerate(plan):
            stall(cur)
            fh.seek(f0 * im.spf)
            if im.syncs:
                assert_late(cur, 'read {} was issued'.format(k))
            got = fh.read(nf * im.spf)
            counts.append(im.mismatch(got, f0))
            del got
        if not im.syncs:
            assert_late(cur, 'the last read returned')
    _all_zero(counts, plan)


@pytest.mark.parametrize('fmt', ['vdif1', 'mark5b'])
def test_decode_waits_for_its_scan_on_a_late_side_stream(img, fmt):
    """The side stream itself is late: each decode must wait for its own scan
    (a decode that does not reads the index a scan of four requests ago left)."""
    import torch
    from baseband_amd.base import base as bbase
    im = img(fmt)
    plan = im.plan(4, 9)
    counts = []
    with im.open() as fh:
        _warm(fh, im)
        side = bbase._scan_streams[im.dev.device.index]
        assert fh._scan_stream is side
        for k, (f0, nf) in enumerate(plan):
            fh.seek(f0 * im.spf)
            stall(side)
            assert_late(side, 'read {} was issued'.format(k))
            got = fh.read(nf * im.spf)
            counts.append(im.mismatch(got, f0))
            del got
    _all_zero(counts, plan)


def test_two_readers_take_turns_on_the_shared_side_stream(img):
    import torch
    im = img('vdif1')
    cur = torch.cuda.current_stream()
    plan = im.plan(5, 12)
    counts = []
    fhs = [im.open(), im.open()]
    try:
        for fh in fhs:
            _warm(fh, im)
        assert fhs[0]._scan_stream is fhs[1]._scan_stream
        for k, (f0, nf) in enumerate(plan):
            fh = fhs[k % 2 if k < 6 else (k // 3) % 2]
            stall(cur)
            fh.seek(f0 * im.spf)
            got = fh.read(nf * im.spf)
            counts.append(im.mismatch(got, f0))
            del got
        assert_late(cur, 'the last read returned')
    finally:
        for fh in fhs:
            fh.close()
    _all_zero(counts, plan)


def test_reads_move_to_another_current_stream(img):
    """First read on the default stream, the later ones inside
    ``torch.cuda.stream(s)`` with `s` late, results consumed on `s`.  The side
    stream waits for the caller's stream only when what it reads changes
    (`_scan_ready_for`): the scratch rotation must follow the new stream."""
    import torch
    im = img('vdif1')
    plan = im.plan(6, 10)
    counts = []
    s = torch.cuda.Stream()
    with im.open() as fh:
        fh.seek(plan[0][0] * im.spf)
        got = fh.read(plan[0][1] * im.spf)
        counts.append(im.mismatch(got, plan[0][0]))
        del got
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for f0, nf in plan[1:]:
                stall(s)
                fh.seek(f0 * im.spf)
                got = fh.read(nf * im.spf)
                counts.append(im.mismatch(got, f0))
                del got
            assert_late(s, 'the last read returned')
    _all_zero(counts, plan)


# ---- 2. verdicts --------------------------------------------------------------------
def _damaged(im, frame):
    """Copy of the image on the device with the frame-length bits of one
    header changed (the invariant every header of the stream shares)."""
    import torch
    image = im.image.copy()
    w = image.reshape(im.nframes, im.fn)[frame, :16].view('<u4')
    w[2] ^= 0x10
    return torch.from_numpy(image).cuda()


@pytest.mark.parametrize('verify', ['fix', True])
@pytest.mark.parametrize('fmt', ['vdif1', 'vdif1_item'])
def test_verdict_belongs_to_the_read_that_meets_the_damage(img, fmt, verify):
    """One damaged header inside read k of a run behind stalls: under
    verify='fix' read k (and no other) warns and fills that frame, the rest is
    the oracle's; under verify=True read k raises.  `vdif1`: verdicts over
    2048 records, fetched on the side stream; `vdif1_item`: fewer, read back
    on the caller's stream."""
    import torch
    im = img(fmt)
    cur = torch.cuda.current_stream()
    bad = im.nframes - 50
    n0 = im.nmin + 3
    plan = [(f, n0) for f in (0, 40, 80, 20)] + [(bad - n0 + 7, n0)] + [(f, n0) for f in (60, 10)]
    k_bad = 4
    assert all(not f0 <= bad <= f0 + nf for k, (f0, nf) in enumerate(plan) if k != k_bad)
    dev = _damaged(im, bad)
    counts, warned = [], []
    with im.open(dev, verify=verify) as fh:
        _warm(fh, im)
        for k, (f0, nf) in enumerate(plan):
            stall(cur)
            fh.seek(f0 * im.spf)
            if im.syncs or k == k_bad:
                # (a read that meets damage goes back to the bytes on the host's side)
                assert_late(cur, 'read {} was issued'.format(k))
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter('always')
                if verify is True and k == k_bad:
                    with pytest.raises(AssertionError):
                        fh.read(nf * im.spf)
                    break
                got = fh.read(nf * im.spf)
            warned.append(any('problem loading frame' in str(c.message) for c in caught))
            if k == k_bad:
                lo = (bad - f0) * im.spf
                fill = got[lo:lo + im.spf]
                assert_zero = (fill.reshape(-1) != 0).sum()
                got = torch.cat([got[:lo], got[lo + im.spf:]])
                counts.append(assert_zero + im.mismatch(got[:lo], f0)
                              + im.mismatch(got[lo:], bad + 1))
            else:
                counts.append(im.mismatch(got, f0))
            del got
        if not im.syncs and verify == 'fix':
            assert_late(cur, 'the last read returned')
    if verify == 'fix':
        assert warned == [k == k_bad for k in range(len(plan))], warned
    else:
        assert len(warned) == k_bad and not any(warned)
    _all_zero(counts, plan[:len(counts)])


# ---- 3. file windows --------------------------------------------------------------
@pytest.fixture(scope='module')
def vdif_path(tmp_path_factory):
    path = str(tmp_path_factory.mktemp('ord') / 'w.vdif')
    return path


def _file_img(img, path):
    im = img('vdif1')
    import os
    if not os.path.exists(path):
        im.image.tofile(path)
    return im


@pytest.mark.parametrize('keep_staged', [False, True])
@pytest.mark.parametrize('late', ['caller', 'copy_stream'])
def test_file_windows_lap_a_late_stream(img, vdif_path, monkeypatch, late, keep_staged):
    """A read through more 1 MiB windows than the pipeline has buffers
    (`_NBUF` = 2).  `caller`: every window's decode is queued behind a stall,
    so host staging runs ahead of the decodes that read the buffers;
    `copy_stream`: every host-to-device copy is."""
    import torch
    from baseband_amd import staging
    im = _file_img(img, vdif_path)
    monkeypatch.setattr(staging, '_NBUF', 2)
    real_run, real_stage = staging.WindowPipeline.run, staging._stage
    where = {}

    def run(self, ranges, process, sink=None):
        def process_late(target, i):
            stall(torch.cuda.current_stream(), 6)
            return process(target, i)
        where['pipe'] = self
        return real_run(self, ranges, process_late if late == 'caller' else process, sink)

    def stage(*a):
        p = where['pipe']
        if late == 'copy_stream' and p._copy_stream is not None:
            stall(p._copy_stream, 6)
        return real_stage(*a)
    monkeypatch.setattr(staging.WindowPipeline, 'run', run)
    monkeypatch.setattr(staging, '_stage', stage)
    counts, plan = [], [(3, 2000), (2100, 290), (100, 1900)]
    with im.open(vdif_path, verify=False) as fh:
        fh.keep_staged = keep_staged
        fh.pipeline_window_bytes = 1 << 20
        fh.decode_ahead = False
        for k, (f0, nf) in enumerate(plan):
            fh.seek(f0 * im.spf)
            got = fh.read(nf * im.spf)
            if k == 0:
                p = where['pipe']
                assert p.nbuf == 2 and p._count > 4 * p.nbuf
                assert_late(torch.cuda.current_stream() if late == 'caller' else p._copy_stream,
                            'the read returned')
            counts.append(im.mismatch(got, f0))
            del got
    _all_zero(counts, plan)


# ---- 4. the small pinned ring -------------------------------------------------------
def test_small_random_reads_reuse_the_pinned_ring_behind_a_late_caller(img, vdif_path):
    import torch
    im = _file_img(img, vdif_path)
    cur = torch.cuda.current_stream()
    rng = np.random.default_rng(9)
    plan = [(int(f), int(n)) for f, n in zip(rng.permutation(im.nframes - 10)[:10], rng.integers(1, 6, 10))]
    counts = []
    with im.open(vdif_path, verify=False) as fh:
        for f0, nf in plan:
            stall(cur, 10)
            fh.seek(f0 * im.spf)
            got = fh.read(nf * im.spf)
            counts.append(im.mismatch(got, f0))
            del got
        assert_late(cur, 'the last read returned')
    _all_zero(counts, plan)


# ---- 5. block formats: the next block on its way -------------------------------------
def _block_file(fmt, d):
    """A GUPPI or DADA file of 8 blocks written by our writer, its bytes and
    the oracle's decode (float32 view, one row per sample)."""
    import torch
    import baseband_amd as bb
    t0 = np.datetime64('2013-07-02T01:39:20')
    if fmt == 'dada':
        from baseband_amd.dada.header import DADAHeader
        h0 = DADAHeader.fromvalues(time=t0, offset=0., sample_rate=16e6, bps=8, complex_data=True, npol=2,
                                   nchan=1, payload_nbytes=1 << 20, start_time=t0, telescope='GMRT')
        path = str(d / 'b.dada')
        fw = bb.dada.open(path, 'ws', header0=h0)
    else:
        import io
        from conftest import golden_path
        g = np.load(golden_path('block_writer_cases.npz'))
        h0 = bb.guppi.GUPPIHeader.fromfile(io.BytesIO(g['guppi_cf_file'].tobytes()))
        path = str(d / 'b.raw')
        fw = bb.guppi.open(path, 'ws', header0=h0)
    with fw:
        n = 8 * fw.samples_per_frame
        x = torch.randn((n,) + fw.sample_shape + (2,), generator=torch.Generator().manual_seed(3)) * 40.
        fw.write(torch.view_as_complex(x.contiguous()).cuda())
    raw = np.fromfile(path, np.uint8)
    exp = orc.dada_read(raw)[0] if fmt == 'dada' else orc.guppi_read(raw)[0]
    exp = np.ascontiguousarray(exp)
    return path, torch.from_numpy(exp.view(np.float32).reshape(exp.shape[0], -1)).cuda()


@pytest.mark.parametrize('late', ['caller', 'default_stream'])
@pytest.mark.parametrize('fmt', ['guppi', 'dada'])
def test_block_prefetch_behind_a_late_stream(fmt, late, tmp_path):
    """Sequential reads of a third of a block: the next block is staged on a
    worker thread (its copies go to the default stream).  `caller`: the
    caller's (default) stream is late; `default_stream`: the caller reads on
    a stream of its own while the default stream, where the prefetch copies
    go, is late."""
    import torch
    import baseband_amd as bb
    path, exp = _block_file(fmt, tmp_path)
    mod = getattr(bb, fmt)
    default = torch.cuda.default_stream()
    s = torch.cuda.Stream() if late == 'default_stream' else default
    bad = []
    with mod.open(path, 'rs', squeeze=False) as fh, torch.cuda.stream(s):
        spf = fh.samples_per_frame
        step = spf // 3 + 1
        assert fh.prefetch_next
        prefetched = 0
        while fh.tell() + step <= fh.shape[0]:
            stall(default, 4)
            lo = fh.tell()
            got = fh.read(step)
            prefetched += fh._prefetch is not None
            g = (torch.view_as_real(got) if got.is_complex() else got).reshape(step, -1)
            bad.append((lo, (g.view(torch.int32) != exp[lo:lo + step].view(torch.int32)).sum()))
            del got, g
        assert prefetched > 4
        assert_late(default, 'the last read returned')
    torch.cuda.synchronize()
    wrong = [lo for lo, c in bad if int(c)]
    assert not wrong, wrong[:5]


# ---- 6. writers ------------------------------------------------------------------------
@pytest.mark.parametrize('target', ['file', 'sequence'])
def test_writer_pieces_come_from_late_work(target, tmp_path, monkeypatch):
    """The samples of every write() come out of an op queued behind a stall of
    the caller's stream, and the frame bytes the sink copies to the host are
    themselves made behind one (`write_device_bytes` wrapped: write() reads a
    header back on the caller's stream, which absorbs the first stall).  The
    file(s) must equal those written synchronously from the same samples."""
    import os
    import torch
    import baseband_amd as bb
    from baseband_amd import staging
    from baseband_amd.vdif import VDIFHeader
    h0 = VDIFHeader.fromvalues(edv=0, time=np.datetime64('2014-06-13T05:30:01'), nchan=1, bps=2,
                               complex_data=False, thread_id=0, samples_per_frame=32000, station='AA')
    src = torch.randn(15 * 32000, generator=torch.Generator().manual_seed(4)).mul_(2.).cuda()
    cuts = [0, 7, 8, 13, 15]
    real = staging.write_device_bytes

    def write(sub, late):
        d = tmp_path / sub
        d.mkdir()
        monkeypatch.setattr(staging, '_WRITE_ASYNC', late)

        def write_device_bytes(fh, dev, *a, **kw):
            stall(torch.cuda.current_stream(), 20)
            return real(fh, dev.clone(), *a, **kw)
        monkeypatch.setattr(staging, 'write_device_bytes', write_device_bytes if late else real)
        name = str(d / ('f{file_nr:03d}.vdif' if target == 'sequence' else 'one.vdif'))
        kw = dict(file_size=3 * 8032) if target == 'sequence' else {}
        fw = bb.vdif.open(name, 'ws', header0=h0, sample_rate=32e6, nthread=1, **kw)
        cur = torch.cuda.current_stream()
        with fw:
            for a, b in zip(cuts[:-1], cuts[1:]):
                if late:
                    stall(cur)
                piece = src[a * 32000:b * 32000] * 1.0 + 0.0            # made behind the stall
                fw.write(piece)
                del piece
            if late:
                assert_late(cur, 'the last write() returned')
        monkeypatch.setattr(staging, 'write_device_bytes', real)
        return {f: open(str(d / f), 'rb').read() for f in sorted(os.listdir(str(d)))}

    want = write('sync', False)
    got = write('late', True)
    assert sorted(got) == sorted(want) and len(want) == (5 if target == 'sequence' else 1)
    for f in want:
        assert got[f] == want[f], f
