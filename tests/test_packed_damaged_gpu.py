"""The reader methods that work on the packed bytes -- ``state_counts``, ``state_series``,
``power_series``, ``frames_valid``, ``read_packed`` and ``baseband_amd.convert`` -- on files
that lost frames or bytes: the 14 VDIF and 27 Mark 5B file-surgery cases that
test_corrupt_gpu.py pins to the reference's decoded output.

The expectation is not a count at the fixed stride.  Every case records the SHA-256 of the
array the reference decoded (fill 0.0).  That array is rebuilt here (VDIF: the intact file's
samples with the recorded frame-slots zeroed, in NumPy; Mark 5B: one ``read()`` of a reader
of its own), checked against the digest, and everything else follows from it in NumPy: no
1- or 2-bit level is 0.0, so ``sample != 0`` is "valid" and the level names the raw code.

Each answer must be the same whichever way the reader gets at its bytes (host file through
staging windows, short windows, `stage()`d, device tensor) and whether or not it has read
the file before; strict readers raise what their ``read()`` raises where the method stands
in for a read, and give the lenient answer where it is documented not to raise."""
import functools
import json
import hashlib
import warnings

import numpy as np
import pytest

from conftest import golden_path, load_expected, load_file
from packedkit import _torch, pack_codes
from test_corrupt_gpu import CASES, _corrupt, FIXED, _fixed_blob
from test_repack_kernels_gpu import MAPS, FILL_CODE, VDIF, MARK5B
from test_states_readers_gpu import open_on
from test_convert_gpu import vdif_writer, m5b_writer

pytestmark = pytest.mark.gpu

T_FAKE = np.datetime64('2010-11-12T13:14:15')
ALL = ([('vdif', i) for i in range(len(CASES))]
       + [(g, i) for g in ('m5b_sample', 'm5b_fake') for i in range(len(FIXED[g]))])
IDS = ['%s-%s%d' % (g, (CASES[i] if g == 'vdif' else FIXED[g][i])['kind'], i) for g, i in ALL]
assert len(ALL) == 41 and not any('error' in (CASES[i] if g == 'vdif' else FIXED[g][i]) for g, i in ALL)

# group -> the targets of read_packed and convert: (coder, nthread, nchan, samples per frame); frames_valid is
# asked for the same frame lengths.  GEOMETRY: group -> (coder of the file, samples per frame, frame-slots per set)
TARGETS = {
    'vdif': [(VDIF, 1, 8, 8000), (MARK5B, 1, 8, 5000), (VDIF, 8, 1, 12000)],     # merge, coder map, re-cut
    'm5b_fake': [(VDIF, 1, 2, 4000), (VDIF, 2, 1, 4000)],                       # ... and split
    'm5b_sample': [(VDIF, 1, 8, 2000)],
}
GEOMETRY = {'vdif': (VDIF, 20000, 8), 'm5b_fake': (MARK5B, 20000, 1), 'm5b_sample': (MARK5B, 5000, 1)}
WAYS = [(how, before) for how in ('file', 'staged', 'device', 'short windows') for before in ('fresh', 'after a read')]


with open(golden_path('levels.json')) as _f:
    _LEVELS = json.load(_f)
# float32 level of raw code 0 .. 3 (the first field of bytes 0 .. 3 of the recorded byte tables)
LEVELS = {coder: np.array([_LEVELS[name][c][0] for c in range(4)], np.uint32).view(np.float32)
          for coder, name in ((VDIF, 'vdif_lut2bit'), (MARK5B, 'mark5b_lut2bit'))}


def opener_of(group):
    from baseband_amd import vdif, mark5b
    if group == 'vdif':
        return vdif.open, {}
    if group == 'm5b_sample':
        return mark5b.open, dict(sample_rate=32e6, kday=56000, nchan=8, bps=2)
    return mark5b.open, dict(nchan=2, sample_rate=100e3, ref_time=T_FAKE)


class Oracle:
    """One damaged file and all that is expected of it, from the reference's decoded array."""

    def __init__(self, group, case, blob, data):
        self.group, self.case, self.blob = group, case, blob
        assert list(data.shape) == case['shape'] and data.dtype == np.float32
        assert hashlib.sha256(data.tobytes()).hexdigest() == case['sha256']
        self.coder, self.spf, self.nslot = GEOMETRY[group]
        self.sample_shape = data.shape[1:]
        self.n = data.shape[0]
        self.data = data.reshape(self.n, -1)
        self.ncomp = self.data.shape[1]
        self.chunk = self.ncomp // self.nslot
        self.unit = max(1, 8 // (self.chunk * 2))               # samples in a byte of a thread's stream
        self.nsets = self.n // self.spf
        assert self.nsets * self.spf == self.n
        levels = LEVELS[self.coder]
        order = np.argsort(levels)
        self.valid = self.data != 0
        at = np.searchsorted(levels[order], self.data).clip(0, 3)
        self.codes = order[at].astype(np.uint8)
        assert np.array_equal(levels[self.codes][self.valid], self.data[self.valid])
        # frame-slots that read as fill, as the case lists them
        self.zeroed = np.zeros((self.nsets, self.nslot), bool)
        for idx in case['zeroed']:
            self.zeroed[idx // self.nslot, idx % self.nslot] = True
        byslot = self.valid.reshape(self.nsets, self.spf, self.nslot, self.chunk)
        assert np.array_equal(~byslot.any((1, 3)), self.zeroed) and np.array_equal(~byslot.all((1, 3)), self.zeroed)

    # -- what the statistics must give
    def counts(self, lo, hi):
        key = (np.arange(self.ncomp) * 4 + self.codes[lo:hi])[self.valid[lo:hi]]
        return np.bincount(key, minlength=self.ncomp * 4).reshape(self.sample_shape + (4,))

    def series(self, lo, hi, bin_samples):
        nbins = -(-(hi - lo) // bin_samples)
        b = (np.arange(hi - lo) // bin_samples)[:, None]
        key = ((b * self.ncomp + np.arange(self.ncomp)) * 4 + self.codes[lo:hi])[self.valid[lo:hi]]
        return np.bincount(key, minlength=nbins * self.ncomp * 4).reshape((nbins,) + self.sample_shape + (4,))

    def power(self, lo, hi, bin_samples):
        """float64 mean of x**2 over the valid samples of a bin; the squares of float32 are exact
        in float64 and each bin is summed pairwise along a contiguous axis."""
        n = hi - lo
        nbins, full = -(-n // bin_samples), n // bin_samples
        x = self.data[lo:hi].astype(np.float64)
        x2 = np.ascontiguousarray((x * x).T)
        ok = np.ascontiguousarray(self.valid[lo:hi].T)
        total = np.zeros((self.ncomp, nbins))
        number = np.zeros((self.ncomp, nbins))
        cut = full * bin_samples
        total[:, :full] = x2[:, :cut].reshape(self.ncomp, full, bin_samples).sum(-1)
        number[:, :full] = ok[:, :cut].reshape(self.ncomp, full, bin_samples).sum(-1)
        if nbins > full:
            total[:, full], number[:, full] = x2[:, cut:].sum(-1), ok[:, cut:].sum(-1)
        with np.errstate(invalid='ignore', divide='ignore'):
            mean = total / number
        return mean.T.reshape((nbins,) + self.sample_shape)

    def wholly_zeroed(self, lo, hi, bin_samples):
        """Bins, by component, that lie wholly inside frame-slots that read as fill."""
        nbins = -(-(hi - lo) // bin_samples)
        a = lo + np.arange(nbins) * bin_samples
        b = np.minimum(a + bin_samples, hi)
        s0, s1 = a // self.spf, (b - 1) // self.spf
        upto = np.concatenate([np.zeros((1, self.nslot), int), np.cumsum(self.zeroed, 0)])
        gone = (upto[s1 + 1] - upto[s0]) == (s1 - s0 + 1)[:, None]             # (bin, slot)
        return np.repeat(gone, self.chunk, axis=1).reshape((nbins,) + self.sample_shape)

    # -- ... and the packed reads
    def frames_valid(self, lo, hi, spf_out):
        nout = -(-(hi - lo) // spf_out)
        a = lo + np.arange(nout) * spf_out
        b = np.minimum(a + spf_out, hi)
        upto = np.concatenate([[0], np.cumsum(self.zeroed.any(1))])
        return (upto[(b - 1) // self.spf + 1] - upto[a // self.spf]) == 0

    def payloads(self, lo, hi, target):
        """The samples [lo, hi) as the payloads of `target`'s writer: codes through the coder
        pair's map, `fill_code` in the samples of frame-slots that read as fill (per slot,
        whatever the validity of the output frame), rows of one thread's channels, LSB first."""
        coder, nthread, nchan, spf_out = target
        table = np.array(MAPS[(self.coder, coder)][2], np.uint8)
        c = np.where(self.valid[lo:hi], table[self.codes[lo:hi]], np.uint8(FILL_CODE[(coder, 2)]))
        nout = (hi - lo) // spf_out
        c = c.reshape(nout, spf_out, nthread, nchan).transpose(0, 2, 1, 3)
        return pack_codes(np.ascontiguousarray(c), 2).reshape(nout, nthread, spf_out * nchan * 2 // 8)

    def converted(self, spf_out):
        """What the converted file reads back as: the array, samples of output frames that
        draw from a frame-slot that reads as fill set to 0."""
        want = self.data.copy()
        for k in np.nonzero(~self.frames_valid(0, self.n, spf_out))[0]:
            want[k * spf_out:(k + 1) * spf_out] = 0.
        return want

    # -- readers
    def image(self):
        return np.frombuffer(self.blob, np.uint8) if isinstance(self.blob, bytes) else self.blob

    def open(self, how='file', **more):
        opener, kw = opener_of(self.group)
        if how == 'short windows':
            fh = open_on(self.image(), opener, kw, 'file', **more)
            fh.window_bytes = 2 * fh._set_nbytes
            return fh
        return open_on(self.image(), opener, kw, how, **more)

    def range(self):
        """From inside the first frame to inside the last one, on whole bytes: every damaged
        frame of these files lies in between or is cut by an end of the range."""
        lo = self.spf // 3 // self.unit * self.unit
        return lo, self.n - self.spf // 5 // self.unit * self.unit


@functools.lru_cache(maxsize=None)
def oracle(group, i):
    if group == 'intact':
        case = dict(kind='intact', shape=[120000, 8, 1], zeroed=[])
        data = load_expected('vdif_triple')
        case['sha256'] = hashlib.sha256(data.tobytes()).hexdigest()
        return Oracle('vdif', case, load_file('synth/vdif_triple.bin'), data)
    if group == 'vdif':
        case = CASES[i]
        data = load_expected('vdif_triple').copy()
        assert case['shape'][0] == data.shape[0]
        for idx in case['zeroed']:
            s, t = divmod(idx, 8)
            data[s * 20000:(s + 1) * 20000, t] = 0.
        return Oracle(group, case, _corrupt(case), data)
    case = FIXED[group][i]
    blob = _fixed_blob(group, case)
    opener, kw = opener_of(group)
    import io
    with opener(io.BytesIO(blob), 'rs', squeeze=False, **kw) as fh, warnings.catch_warnings():
        warnings.simplefilter('ignore')
        data = fh.read().cpu().numpy()
    return Oracle(group, case, blob, data)


def quietly(call, *args, **kw):
    """Warnings are not what is tested here: recorded, never errors."""
    with warnings.catch_warnings(record=True):
        warnings.simplefilter('always')
        return call(*args, **kw)


# -- the assertions of tests 1-4, each on an open reader; they return what the reader gave -----
def check_counts(o, fh):
    torch = _torch()
    got = []
    for lo, hi in ((0, o.n), o.range()):
        fh.seek(lo)
        counts = quietly(fh.state_counts, None if hi == o.n else hi - lo)
        assert fh.tell() == lo
        assert counts.dtype == torch.int64 and tuple(counts.shape) == o.sample_shape + (4,)
        want = o.counts(lo, hi)
        print('state_counts', (lo, hi), 'differing counters:', int((counts.cpu().numpy() != want).sum()))
        assert np.array_equal(counts.cpu().numpy(), want), (lo, hi)
        got.append(counts)
    fh.seek(0)
    return got


def bins_of(o):
    return [o.unit, 1000, o.spf, o.spf * 5 // 2, o.n]


def check_series(o, fh):
    got = []
    lo, hi = o.range()
    for a, b, bin_samples in [(0, o.n, n) for n in bins_of(o)] + [(lo, hi, 1000)]:
        fh.seek(a)
        count = None if b == o.n else b - a
        series = quietly(fh.state_series, bin_samples, count)
        power = quietly(fh.power_series, bin_samples, count)
        counts = quietly(fh.state_counts, count)
        assert fh.tell() == a
        want = o.series(a, b, bin_samples)
        s = series.cpu().numpy()
        print('state_series', (a, b, bin_samples), 'differing counters:', int((s != want).sum()) if s.shape == want.shape else s.shape)
        assert s.shape == want.shape and np.array_equal(s, want), (a, b, bin_samples)
        assert np.array_equal(series.sum(0).cpu().numpy(), counts.cpu().numpy())
        p, pw = power.cpu().numpy(), o.power(a, b, bin_samples)
        assert p.dtype == np.float64 and p.shape == pw.shape
        assert np.array_equal(np.isnan(p), o.wholly_zeroed(a, b, bin_samples)), (a, b, bin_samples)
        assert np.array_equal(np.isnan(pw), np.isnan(p))
        there = ~np.isnan(pw)
        err = np.abs(p[there] - pw[there]) / pw[there]
        print('power_series', (a, b, bin_samples), 'largest relative error:', err.max() if err.size else 0.)
        assert (err <= 1e-12).all(), (a, b, bin_samples)
        got += [series, power]
    fh.seek(0)
    return got


def check_frames_valid(o, fh):
    got = []
    for _, _, _, spf_out in TARGETS[o.group]:
        assert o.n % spf_out == 0 and spf_out != o.spf          # (whole output frames that are not the input's)
        fh.seek(0)
        valid = quietly(fh.frames_valid, o.n, spf_out)
        assert fh.tell() == 0
        assert valid.dtype == bool and np.array_equal(valid, o.frames_valid(0, o.n, spf_out)), spf_out
        got.append(_torch().from_numpy(valid))
    return got


def check_read_packed(o, fh):
    from baseband_amd import _lib
    assert (_lib.CODER_VDIF, _lib.CODER_MARK5B) == (VDIF, MARK5B)
    got = []
    for target in TARGETS[o.group]:
        coder, nthread, nchan, spf_out = target
        fh.seek(0)
        payloads, valid = quietly(fh.read_packed, o.n, coder, nthread, nchan, spf_out, FILL_CODE[(coder, 2)])
        assert fh.tell() == o.n
        want = o.payloads(0, o.n, target)
        p = payloads.cpu().numpy()
        print('read_packed', target, 'differing bytes:', int((p != want).sum()) if p.shape == want.shape else p.shape)
        assert p.dtype == np.uint8 and p.shape == want.shape and np.array_equal(p, want), target
        assert np.array_equal(valid, o.frames_valid(0, o.n, spf_out)), target
        got += [payloads, _torch().from_numpy(valid)]
    fh.seek(0)
    return got


CHECKS = [check_counts, check_series, check_frames_valid, check_read_packed]


def fresh(o, check, how='file'):
    with o.open(how) as fh:
        shape = tuple(fh.shape)
        assert list(shape) == o.case['shape']
        got = check(o, fh)
        assert tuple(fh.shape) == shape
    return got


# -- 1-4: each method on a reader that has read nothing -----------------------------------------
@pytest.mark.parametrize('group,i', ALL, ids=IDS)
def test_state_counts(group, i):
    fresh(oracle(group, i), check_counts)


@pytest.mark.parametrize('group,i', ALL, ids=IDS)
def test_state_series_and_power_series(group, i):
    fresh(oracle(group, i), check_series)


@pytest.mark.parametrize('group,i', ALL, ids=IDS)
def test_frames_valid(group, i):
    fresh(oracle(group, i), check_frames_valid)


@pytest.mark.parametrize('group,i', ALL, ids=IDS)
def test_read_packed(group, i):
    fresh(oracle(group, i), check_read_packed)


@pytest.mark.parametrize('check', CHECKS, ids=[c.__name__ for c in CHECKS])
def test_the_intact_file_is_the_control(check):
    fresh(oracle('intact', 0), check)


# -- 5: convert ---------------------------------------------------------------------------------
def writer_for(path, fr, target):
    coder, nthread, nchan, spf_out = target
    if coder == MARK5B:
        return m5b_writer(path, nchan)
    return vdif_writer(path, fr, nthread, nchan, spf_out, spf_out * 2000.)


def read_back(path, target):
    from baseband_amd import vdif, mark5b
    coder, nthread, nchan, spf_out = target
    if coder == MARK5B:
        return mark5b.open(path, 'rs', sample_rate=32e6, kday=56000, nchan=nchan, bps=2, squeeze=False)
    return vdif.open(path, 'rs', sample_rate=spf_out * 2000., squeeze=False)


def invalid_frames(raw, target):
    """Output frames marked invalid in the file: the invalid bit of VDIF headers (32-byte
    headers of the writer's EDV 0), the fill pattern in Mark 5B payloads."""
    coder, nthread, nchan, spf_out = target
    if coder == MARK5B:
        frames = raw.reshape(-1, 10016)[:, 16:]
        return (np.ascontiguousarray(frames).view('<u4') == 0x11223344).all(1)
    frame = 32 + spf_out * nchan * 2 // 8
    bit = (raw[3::frame] >> 7).reshape(-1, nthread)
    assert (bit == bit[:, :1]).all()
    return bit[:, 0].astype(bool)


@pytest.mark.parametrize('group,i', ALL, ids=IDS)
def test_convert(group, i, tmp_path):
    import baseband_amd
    o = oracle(group, i)
    for t, target in enumerate(TARGETS[o.group]):
        files = {}
        for packed in (True, False):
            path = str(tmp_path / 'out{}_{}'.format(t, int(packed)))
            with o.open('file') as fr, writer_for(path, fr, target) as fw:
                n = quietly(baseband_amd.convert, fr, fw, packed=packed)        # (an EOFError is a failure)
                assert n == o.n and fr.tell() == o.n and fw.tell() == o.n, (target, packed)
            files[packed] = np.fromfile(path, np.uint8)
        assert files[True].size > 0 and np.array_equal(files[True], files[False]), target
        spf_out = target[3]
        want_invalid = ~o.frames_valid(0, o.n, spf_out)
        assert np.array_equal(invalid_frames(files[True], target), want_invalid), target
        with read_back(str(tmp_path / 'out{}_1'.format(t)), target) as new:
            got = quietly(new.read).cpu().numpy()
        assert got.shape[0] == o.n
        assert np.array_equal(got.reshape(o.n, -1), o.converted(spf_out)), target


# -- 6: the same answer however the reader got there -----------------------------------------------
def same(a, b):
    torch = _torch()
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(torch.nan_to_num(a.cpu(), nan=-1.),
                                                                     torch.nan_to_num(b.cpu(), nan=-1.))


@pytest.mark.parametrize('group,i', ALL, ids=IDS)
def test_every_answer_is_the_same_however_the_reader_got_there(group, i):
    o = oracle(group, i)
    first = None
    for how, before in WAYS:
        with o.open(how) as fh:
            shape = tuple(fh.shape)
            assert list(shape) == o.case['shape'], (how, before)
            if before == 'after a read':
                quietly(fh.read)
                fh.seek(0)
            got = [t for check in CHECKS for t in check(o, fh)]
            assert tuple(fh.shape) == shape, (how, before)
        if first is None:
            first = got
        assert len(got) == len(first) and all(same(a, b) for a, b in zip(got, first)), (how, before)


# -- 7: strict readers -----------------------------------------------------------------------------
STRICT = [('vdif', 0), ('vdif', 6), ('vdif', 12), ('m5b_fake', 16), ('m5b_fake', 17)]
assert [CASES[i]['kind'] for g, i in STRICT[:3]] == ['frames', 'bytes', 'overwrite']
assert [FIXED[g][i]['kind'] for g, i in STRICT[3:]] == ['middle', 'middle']


def what_read_raises(o):
    with o.open('file', verify=True) as twin:
        with pytest.raises(Exception) as met:
            quietly(twin.read, o.n)
    return met.type


@pytest.mark.parametrize('group,i', STRICT, ids=['%s%d' % s for s in STRICT])
def test_strict_readers_raise_what_their_read_raises(group, i, tmp_path):
    import baseband_amd
    o = oracle(group, i)
    error = what_read_raises(o)
    assert error in (ValueError, OSError, EOFError, AssertionError)
    target = TARGETS[o.group][0]
    coder, nthread, nchan, spf_out = target
    with o.open('file', verify=True) as fh:
        with pytest.raises(Exception) as met:
            quietly(fh.read_packed, o.n, coder, nthread, nchan, spf_out, FILL_CODE[(coder, 2)])
        assert met.type is error and fh.tell() == 0
    with o.open('file', verify=True) as fh:
        with pytest.raises(Exception) as met:
            quietly(fh.frames_valid, o.n, spf_out)
        assert met.type is error and fh.tell() == 0
    for packed in (True, False):
        with o.open('file', verify=True) as fr, writer_for(str(tmp_path / 'refused{}'.format(int(packed))), fr, target) as fw:
            with pytest.raises(Exception) as met:
                quietly(baseband_amd.convert, fr, fw, packed=packed)
            assert met.type is error, packed


@pytest.mark.parametrize('how', ['file', 'staged'])
@pytest.mark.parametrize('group,i', STRICT, ids=['%s%d' % s for s in STRICT])
def test_strict_readers_count_as_lenient_ones_and_stay_strict(group, i, how):
    o = oracle(group, i)
    error = what_read_raises(o)
    with o.open(how, verify=True) as fh:
        check_counts(o, fh)
        check_series(o, fh)
        assert fh.tell() == 0 and list(fh.shape) == o.case['shape']
        with pytest.raises(Exception) as met:           # bad frames do not raise in the statistics; reads go on raising
            quietly(fh.read, o.n)
        assert met.type is error
