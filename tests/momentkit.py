"""What the tests of bb_i8_moments (k_i8_moments) share, all of it NumPy and plain Python:

  * `oracle`: the plain int64 reference, frame by frame (with `samples`, `row_bytes`);
  * `series_oracle`: the same answer from prefix sums of the whole buffer, for launches of thousands of
    overlapping payloads (tests/test_momentkit.py pins it to `oracle`);
  * `split`: the host's work split (moments_params_check and bb_i8_moments in csrc/bb_packed.inc) restated:
    mode, items, items of a wave's range, ranges, grid, and item number -> (unit, frame, segment);
  * `model`: a model kernel at work-item granularity that walks every wave's range as k_moments.h does --
    incremental (unit, frame, segment) counter, int32 partials with real wraparound that stand for a wave's
    added-up lanes, folds, flushes when the (unit, bin) changes and at the range's end -- and can be told
    to get one of these things wrong (`FAULTS`);
  * `crossings`: what the ranges of a launch cross; `indexed` and `strided`: the inputs of the range tests.

A unit is a run (run form) or a block of 64 lane columns (row form)."""
import numpy as np

CF, TF, ROWS = 0, 1, 2

# csrc/k_moments.h and csrc/bb_packed.inc (tests/test_momentkit.py reads them there)
WAVE = 64
WAVES_PER_BLOCK = 4
GRID_WAVES = 4096                   # BB_MOMENTS_GRID * BB_WAVES_PER_BLOCK
U = 4                               # BB_MOM_U
STEP = 1024                         # BB_MOM_STEP
RUN_STEPS = 16                      # BB_MOM_RUN_STEPS
ROW_STEPS = 32                      # BB_MOM_ROW_STEPS
RUN_FOLD = 64                       # BB_MOM_RUN_FOLD
ROW_FOLD = 1 << 16                  # BB_MOM_ROW_FOLD

FAULTS = ('stuck_counter', 'no_unit_flush', 'first_bin', 'drop_last', 'no_fold', 'fold_x8')


def row_bytes(layout, npol, nchan, ncomp):
    return npol * nchan * ncomp


def samples(payload, layout, npol, nchan, ncomp, ntime):
    """int64 (time, pol, chan, comp) of one stored payload."""
    x = payload.view(np.int8).astype(np.int64)
    if layout == CF:
        return x.reshape(nchan, ntime, npol, 2).transpose(1, 2, 0, 3)
    if layout == TF:
        return x.reshape(ntime, nchan, npol, 2).transpose(0, 2, 1, 3)
    return x.reshape(ntime, npol, nchan, ncomp)


def oracle(buf, offsets, layout, npol, nchan, ncomp, ntime, t_lo, t_hi, bin_rows, nbins, first_row=0, sums=None):
    """What bb_i8_moments adds for the frames at `offsets` of the NumPy byte buffer `buf`."""
    if sums is None:
        sums = np.zeros((nbins, npol, nchan, ncomp, 2), np.int64)
    pay, nt = ntime * row_bytes(layout, npol, nchan, ncomp), t_hi - t_lo
    for f, so in enumerate(offsets):
        so = int(so)
        if so < 0 or so + pay > buf.size or so % 4 or nt == 0:
            continue
        x = samples(buf[so:so + pay], layout, npol, nchan, ncomp, ntime)[t_lo:t_hi]
        bins = (first_row + f * nt + np.arange(nt)) // bin_rows
        starts = np.r_[0, np.flatnonzero(np.diff(bins)) + 1]
        sums[bins[starts], ..., 0] += np.add.reduceat(x, starts, axis=0)
        sums[bins[starts], ..., 1] += np.add.reduceat(x * x, starts, axis=0)
    return sums


def strided_prefix(buf, step):
    """T, int64 (size + step or more, 2): T[j] = the sum of (x, x * x) over the bytes j - step, j - 2 step, ...
    of `buf` as int8.  The bytes o + k * step, a <= k < b, then add up to T[o + b * step] - T[o + a * step]."""
    x = buf.view(np.int8).astype(np.int64)
    n = -(-x.size // step)
    v = np.zeros((n + 1, step, 2), np.int64)
    flat = np.zeros(n * step, np.int64)
    flat[:x.size] = x
    v[1:, :, 0] = flat.reshape(n, step)
    v[1:, :, 1] = v[1:, :, 0] ** 2
    np.cumsum(v, axis=0, out=v)
    return v.reshape(-1, 2)


def valid_sources(offsets, size, pay, align=4):
    """Which frames count: the source inside the buffer and on `align` bytes."""
    so = np.asarray(offsets, np.int64)
    return (so >= 0) & (so <= size - pay) & (so % align == 0)


def series_oracle(buf, offsets, layout, npol, nchan, ncomp, ntime, t_lo, t_hi, bin_rows, nbins, first_row=0, sums=None,
                  chunk=1 << 22):
    """`oracle` for many frames: the same sums from prefix sums of the whole buffer along the stride from
    one time to the next, differenced at the bin edges of every frame."""
    if sums is None:
        sums = np.zeros((nbins, npol, nchan, ncomp, 2), np.int64)
    R = row_bytes(layout, npol, nchan, ncomp)
    pay, nt = ntime * R, t_hi - t_lo
    if nt == 0:
        return sums
    pol, chan, comp = np.meshgrid(np.arange(npol), np.arange(nchan), np.arange(ncomp), indexing='ij')
    if layout == CF:
        step, col = npol * 2, chan * ntime * npol * 2 + pol * 2 + comp
    elif layout == TF:
        step, col = R, chan * npol * 2 + pol * 2 + comp
    else:
        step, col = R, (pol * nchan + chan) * ncomp + comp
    col = col.reshape(-1)
    T = strided_prefix(buf, step)
    so = np.asarray(offsets, np.int64)
    frames = np.flatnonzero(valid_sources(so, buf.size, pay))
    flat = sums.reshape(nbins, R, 2)
    per_frame = (nt - 1) // bin_rows + 2                     # (frame, bin) pairs of a frame, at most
    nf = max(1, chunk // (per_frame * R))
    for k in range(0, frames.size, nf):
        f = frames[k:k + nf]
        g0 = first_row + f * nt
        b_lo, b_hi = g0 // bin_rows, (g0 + nt - 1) // bin_rows
        cnt = b_hi - b_lo + 1
        which = np.repeat(np.arange(f.size), cnt)
        bins = b_lo[which] + (np.arange(which.size) - np.repeat(np.cumsum(cnt) - cnt, cnt))
        lo = np.maximum(bins * bin_rows, g0[which]) - g0[which] + t_lo       # times of the frame in the bin
        hi = np.minimum((bins + 1) * bin_rows, g0[which] + nt) - g0[which] + t_lo
        at = so[f][which][:, None] + col[None, :]
        D = T[at + hi[:, None] * step] - T[at + lo[:, None] * step]
        starts = np.r_[0, np.flatnonzero(np.diff(bins)) + 1]                 # (the bins only grow: frames in order)
        flat[bins[starts]] += np.add.reduceat(D, starts, axis=0)
    return sums


class Split(object):
    """The work split of one launch.  mode: 'run', 'rows4' or 'rows16'; nwork items of which a wave walks `per`
    in a row, `ranges` waves with one, `grid` workgroups."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def item(self, w):
        """Item number -> (unit, frame, segment)."""
        unit, r = divmod(w, self.nframes * self.nseg)
        return (unit,) + divmod(r, self.nseg)

    def range_of(self, k):
        return k * self.per, min(self.nwork, (k + 1) * self.per)


def split(layout, npol, nchan, ncomp, ntime, nframes, t_lo, t_hi, wide, waves=GRID_WAVES):
    """moments_params_check and the split of bb_i8_moments.  `wide`: no index, and the buffer, the first
    offset and the stride are multiples of 16 (rows of a multiple of 16 bytes then take 16 bytes a lane)."""
    R = row_bytes(layout, npol, nchan, ncomp)
    nt = t_hi - t_lo
    assert nt > 0 and nframes > 0
    s = Split(layout=layout, npol=npol, nchan=nchan, ncomp=ncomp, ntime=ntime, nframes=nframes, t_lo=t_lo, nt=nt, R=R,
              P=0, Rb=0, nrun=1, pitch=0, c_stride=0, tf=False, V=0, NV=0, rpl=0, chunk_rows=0)
    if layout == ROWS:
        if R in (1, 2, 4):
            s.P = R
        else:
            assert R % 4 == 0, R
            s.Rb = R
        s.ph_off = [j % s.P if s.P else 0 for j in range(4)]
    else:
        assert ncomp == 2 and npol <= 2 and (layout == CF or npol == 2)
        P = npol * 2
        if layout == TF and nchan > 1:
            s.Rb, s.tf = R, True
        else:
            s.P = P
            if layout == CF:
                s.nrun, s.pitch, s.c_stride = nchan, ntime * P, 2
        s.ph_off = [((j % P) // 2) * nchan * 2 + (j & 1) for j in range(4)]
    if s.P:
        s.mode = 'run'
        nst = (nt * s.P + 15 + STEP - 1) // STEP
        s.nseg = -(-nst // RUN_STEPS)
        s.units = s.nrun
    else:
        v4 = bool(wide) and s.Rb % 16 == 0
        s.mode = 'rows16' if v4 else 'rows4'
        s.V = 4 if v4 else 1
        s.NV = s.Rb // (4 * s.V)
        s.rpl = WAVE // s.NV if s.NV < WAVE else 1
        s.chunk_rows = s.rpl * ROW_STEPS
        s.nseg = -(-nt // s.chunk_rows)
        s.units = -(-s.NV // WAVE)
    s.nwork = s.nseg * nframes * s.units
    w = min(s.nwork, waves)
    s.per = -(-s.nwork // w)
    s.ranges = -(-s.nwork // s.per)
    s.grid = -(-s.ranges // WAVES_PER_BLOCK)
    return s


def _run_item(s, so, unit, seg, buf_align):
    """The bytes [x0, x1) of the buffer that a run-form item counts and where its groups of loads begin, or None."""
    A0 = so + unit * s.pitch + s.t_lo * s.P
    A1 = A0 + s.nt * s.P
    base = A0 - ((buf_align + A0) & 15)
    nst = -(-(A1 - base) // STEP)
    st = seg * RUN_STEPS
    if st >= nst:
        return None
    st_end = min(st + RUN_STEPS, nst)
    return max(A0, base + st * STEP), min(A1, base + st_end * STEP), base + st * STEP, A0


def skipped_items(s, offsets, size, buf_align=0, kinds=False):
    """bool per item number: the kernel leaves it at one of its three `continue`s.  `kinds`: -> (the source is
    missing, outside the buffer or misaligned; the run ended before this item)."""
    pay = s.ntime * s.R
    ok = valid_sources(offsets, size, pay, 4 * max(s.V, 1))
    w = np.arange(s.nwork)
    unit, r = np.divmod(w, s.nframes * s.nseg)
    frame, seg = np.divmod(r, s.nseg)
    missing, ended = ~ok[frame], np.zeros(s.nwork, bool)
    if s.mode == 'run':
        so = np.asarray(offsets, np.int64)[frame]
        A0 = so + unit * s.pitch + s.t_lo * s.P
        base = A0 - ((buf_align + A0) & 15)
        nst = -(-(A0 + s.nt * s.P - base) // STEP)
        ended = ~missing & (seg * RUN_STEPS >= nst)
    return (missing, ended) if kinds else missing | ended


def crossings(s, offsets, size, buf_align=0):
    """What the ranges of a launch cross -> dict of bool: does at least one range begin inside a frame
    ('mid_frame'), hold items of two frames of one unit ('frame'), counted items of two units ('unit'), a
    skipped item followed by a counted one ('skip_then_count'), a frame whose source is missing between two
    counted items ('count_skip_count'), and is one shorter than the others ('short')."""
    k = np.arange(s.ranges)
    w0 = k * s.per
    w1 = np.minimum(w0 + s.per, s.nwork) - 1
    per_unit = s.nframes * s.nseg
    missing, ended = skipped_items(s, offsets, size, buf_align, kinds=True)
    skip = missing | ended
    pair = skip[:-1] & ~skip[1:] & (np.arange(s.nwork - 1) % s.per != s.per - 1)
    counted = np.flatnonzero(~skip)
    a, b = counted[:-1], counted[1:]                         # a counted item and the next one
    together = a // s.per == b // s.per
    nmiss = np.cumsum(missing)
    return dict(mid_frame=bool((w0 % s.nseg != 0).any()),
                frame=bool(((w0 // s.nseg != w1 // s.nseg) & (w0 // per_unit == w1 // per_unit)).any()),
                unit=bool((together & (a // per_unit != b // per_unit)).any()),
                skip_then_count=bool(pair.any()),
                count_skip_count=bool((together & (nmiss[b] > nmiss[a])).any()),
                short=s.nwork % s.per != 0)


def model(buf, offsets, layout, npol, nchan, ncomp, ntime, t_lo, t_hi, bin_rows, nbins, first_row=0, sums=None,
          wide=False, waves=GRID_WAVES, fault=None, buf_align=0):
    """The model kernel: what k_i8_moments adds, computed as it computes it at item granularity.  Every wave
    walks its range with the incremental counter; an item's sums per bin are differences of prefix sums (the
    oracle's arithmetic); they go through int32 accumulators that wrap as the hardware's do and stand for the
    wave's lanes added up (run form: one per byte phase of a dword; row form: one per byte column of the unit),
    are folded into int64 after RUN_FOLD passes or ROW_FOLD rows, and leave when the (unit, bin) changes and at
    the range's end.  `fault` (one of FAULTS): the counter is not advanced past a skipped item; no flush when
    the unit changes and the bin number does not; the bin is taken from the range's first counted item and
    carried on from there; a last range shorter than the others is dropped; no fold; a fold threshold 8 times
    too high."""
    assert fault is None or fault in FAULTS, fault
    if sums is None:
        sums = np.zeros((nbins, npol, nchan, ncomp, 2), np.int64)
    nframes = len(offsets)
    s = split(layout, npol, nchan, ncomp, ntime, nframes, t_lo, t_hi, wide, waves)
    run = s.mode == 'run'
    flat = sums.reshape(nbins, s.R, 2)
    so_all = [int(x) for x in offsets]
    ok = valid_sources(offsets, buf.size, ntime * s.R, 4 * max(s.V, 1))
    T = strided_prefix(buf, 4 if run else s.Rb)
    fold_at = (RUN_FOLD if run else ROW_FOLD) * (8 if fault == 'fold_x8' else 1)
    if fault == 'no_fold':
        fold_at = 1 << 62
    if run:
        elem_of = [np.array([s.ph_off[j] + c * s.c_stride for j in range(4)]) for c in range(s.units)]
        gran = s.P                                            # the series is walked in bytes
    else:
        cols = [np.arange(u * 256 * s.V, min(s.Rb, (u + 1) * 256 * s.V)) for u in range(s.units)]
        elem_of = [(((q >> 1) & 1) * nchan + (q >> 2)) * 2 + (q & 1) if s.tf else q for q in cols]
        gran = 1                                              # ... in rows
    uniq, inv = zip(*[np.unique(e, return_inverse=True) for e in elem_of])
    bin_g = bin_rows * gran
    phases = np.arange(4)

    def flush():
        if 0 <= cur_bin < nbins:
            np.add.at(flat[cur_bin], elem_of[cur_unit], tot + acc.astype(np.int64))

    for k in range(s.ranges):
        w0, w1 = s.range_of(k)
        if fault == 'drop_last' and w1 - w0 < s.per:
            continue
        unit, frame, seg = s.item(w0)
        have, cur_unit, cur_bin, nacc, carried = False, 0, 0, 0, None
        acc = tot = None
        for w in range(w0, w1):
            u_, f_, s_ = unit, frame, seg
            seg += 1
            if seg == s.nseg:
                seg, frame = 0, frame + 1
                if frame == nframes:
                    frame, unit = 0, unit + 1
            so, it = so_all[f_], None
            if ok[f_]:
                if run:
                    it = _run_item(s, so, u_, s_, buf_align)
                else:
                    r0 = t_lo + s_ * s.chunk_rows
                    it = (r0, min(r0 + s.chunk_rows, t_hi), 0, t_lo)
            if it is None:
                if fault == 'stuck_counter':
                    unit, frame, seg = u_, f_, s_
                continue
            x0, x1, origin, A0 = it
            g = (first_row + f_ * s.nt) * gran + (x0 - A0)    # where the item's first byte (row) lies in the series
            if fault == 'first_bin' and carried is not None:
                g = carried
            carried = g + (x1 - x0)
            b_lo, b_hi = g // bin_g, (g + (x1 - x0) - 1) // bin_g
            edges = np.empty(b_hi - b_lo + 2, np.int64)
            edges[0], edges[-1] = x0, x1
            edges[1:-1] = x0 + (np.arange(b_lo + 1, b_hi + 1) * bin_g - g)
            if run:
                at = edges[:, None] + ((phases[None, :] - edges[:, None]) & 3)
                cost = (edges[1:] - 1 - origin) // (U * STEP) - (edges[:-1] - origin) // (U * STEP) + 1   # passes
            else:
                at = so + cols[u_][None, :] + edges[:, None] * s.Rb
                cost = edges[1:] - edges[:-1]                 # rows
            D = T[at]
            D = (D[1:] - D[:-1]).astype(np.int32)             # (as the partials hold it)
            for i in (0, len(D) - 1) if len(D) > 1 else (0,):
                b = b_lo + i
                if i and len(D) > 2:
                    # the bins in between begin and end inside the item: each is flushed as it stands
                    mid = np.arange(b_lo + 1, min(b, nbins))
                    X = np.zeros((mid.size, len(uniq[u_]), 2), np.int64)
                    for j, e in enumerate(inv[u_]):            # (byte phases of one component share an element)
                        X[:, e] += D[1:1 + mid.size, j]
                    flat[np.ix_(mid, uniq[u_])] += X
                unit_changed = u_ != cur_unit and fault != 'no_unit_flush'
                if not have or unit_changed or b != cur_bin:
                    if have:
                        flush()
                    have, cur_unit, cur_bin, nacc = True, u_, b, 0
                    acc, tot = np.zeros((len(elem_of[u_]), 2), np.int32), np.zeros((len(elem_of[u_]), 2), np.int64)
                if not run and nacc + cost[i] > fold_at:      # the row form folds before it adds, by leaving
                    flush()
                    acc[:], tot[:], nacc = 0, 0, 0
                n = min(len(acc), D.shape[1])                 # (they differ only where a fault keeps another unit's partials)
                acc[:n] += D[i, :n]
                nacc += int(cost[i])
                if run and nacc >= fold_at:
                    tot += acc
                    acc[:], nacc = 0, 0
        if have:
            flush()
    return sums


# ---- the inputs of the range tests ------------------------------------------------------------------------

def indexed(geom, nframes, t_lo, t_hi, rng, waves=GRID_WAVES):
    """A small random buffer and an index of `nframes` entries into it -> (buf, offsets).  The entries are a
    handful of overlapping payloads on every dword of 16 bytes, one of them ending exactly at the buffer's
    end; scattered between them are -1, an offset past the buffer, one that leaves it by a dword and one
    with so % 4 == 2, also as the first, a middle and the last item of ranges spread over the launch."""
    layout, npol, nchan, ncomp, ntime = geom
    pay = ntime * row_bytes(layout, npol, nchan, ncomp)
    assert pay % 4 == 0
    size = 64 + 2 * pay + 40
    buf = rng.integers(0, 256, size, dtype=np.uint8)
    good = np.array([64, 68, 76, 64 + (pay // 2 & ~15) + 8, size - pay], np.int64)
    bad = np.array([-1, size + 64, size - pay + 4, 66], np.int64)
    offsets = good[rng.integers(0, good.size, nframes)]
    stray = rng.random(nframes) < 0.02
    offsets[stray] = bad[rng.integers(0, bad.size, int(stray.sum()))]
    s = split(layout, npol, nchan, ncomp, ntime, nframes, t_lo, t_hi, False, waves)
    for i, k in enumerate(np.linspace(1, s.ranges - 2, 36).astype(int)):
        w0, w1 = s.range_of(int(k))
        w = (w0, (w0 + w1 - 1) // 2, w1 - 1)[i % 3]
        offsets[s.item(w)[1]] = bad[(i // 3) % bad.size]
    offsets[[0, 1, -2, -1]] = good[[1, 3, 4, 0]]               # (the frames either side of a unit boundary count)
    return buf, offsets


def strided(geom, nframes, src0, stride, rng):
    """A random buffer that holds `nframes` payloads from `src0` on at `stride` bytes (they overlap), the
    last one ending at the buffer's end -> (buf, offsets)."""
    layout, npol, nchan, ncomp, ntime = geom
    pay = ntime * row_bytes(layout, npol, nchan, ncomp)
    buf = rng.integers(0, 256, src0 + (nframes - 1) * stride + pay, dtype=np.uint8)
    return buf, src0 + stride * np.arange(nframes, dtype=np.int64)
