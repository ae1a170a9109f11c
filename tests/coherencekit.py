"""What the tests of bb_i8_coherence (k_i8_coherence) share, all of it NumPy and plain Python:

  * `oracle`: the plain int64 reference, frame by frame, on `momentkit.samples`;
  * `split`: the host's work split (coherence_params_check and bb_i8_coherence in csrc/bb_packed.inc)
    restated: shape, items, items of a wave's range, ranges, grid;
  * the fold constants of csrc/k_coherence.h and the two extreme quads;
  * `sdot4`, `quad_sums` and `pair_sums`: the kernel's arithmetic on dwords, instruction by instruction.

A unit is a run (run shape) or a block of 64 lane columns (row shapes)."""
import numpy as np

import momentkit as mk
from momentkit import CF, TF, ROWS        # noqa: F401

# csrc/k_coherence.h (tests/test_coherencekit.py reads them there); the rest of the split is momentkit's
RUN_FOLD = 32                       # BB_COH_RUN_FOLD
ROW_FOLD = 1 << 15                  # BB_COH_ROW_FOLD

# (xr, xi, yr, yi): per sample |X|^2 = 32513, |Y|^2 = 32768, Re = 128 and Im = +32640, -32640
EXTREME = ((127, -128, -128, -128), (-128, 127, -128, -128))
EXTREME_SUMS = ((32513, 32768, 128, 32640), (32513, 32768, 128, -32640))


def oracle(buf, offsets, layout, nchan, ntime, t_lo, t_hi, bin_rows, nbins, first_row=0, sums=None):
    """What bb_i8_coherence adds for the frames at `offsets` of the NumPy byte buffer `buf` -> int64
    (nbins, nchan, 4): sum |X|^2, sum |Y|^2, Re and Im of sum X conj(Y)."""
    if sums is None:
        sums = np.zeros((nbins, nchan, 4), np.int64)
    pay, nt = ntime * 4 * nchan, t_hi - t_lo
    for f, so in enumerate(offsets):
        so = int(so)
        if so < 0 or so + pay > buf.size or so % 4 or nt == 0:
            continue
        s = mk.samples(buf[so:so + pay], layout, 2, nchan, 2, ntime)[t_lo:t_hi]      # (time, pol, chan, re/im)
        xr, xi, yr, yi = s[:, 0, :, 0], s[:, 0, :, 1], s[:, 1, :, 0], s[:, 1, :, 1]
        v = np.stack((xr * xr + xi * xi, yr * yr + yi * yi, xr * yr + xi * yi, xi * yr - xr * yi), -1)
        bins = (first_row + f * nt + np.arange(nt)) // bin_rows
        starts = np.r_[0, np.flatnonzero(np.diff(bins)) + 1]
        sums[bins[starts]] += np.add.reduceat(v, starts, axis=0)
    return sums


def supported(layout, nchan):
    """coherence_params_check on top of the moments check, for two complex polarisations."""
    return not (layout == ROWS and nchan > 1 and nchan % 2)


def split(layout, nchan, ntime, nframes, t_lo, t_hi, wide, waves=mk.GRID_WAVES):
    """The split of bb_i8_coherence -> momentkit.Split with mode 'run', 'rows4', 'rows16', 'split4' or
    'split16'.  `wide`: no index, and the buffer, the first offset and the stride are multiples of 16."""
    assert supported(layout, nchan)
    s = mk.split(layout, 2, nchan, 2, ntime, nframes, t_lo, t_hi, wide, waves)
    if layout != ROWS or nchan == 1:
        return s                                             # runs of quads, rows of quads: the moments split
    v4 = bool(wide) and s.Rb % 32 == 0                       # lane columns of the X half of a row
    s.mode = 'split16' if v4 else 'split4'
    s.V = 4 if v4 else 1
    s.NV = s.Rb // (8 * s.V)
    s.rpl = mk.WAVE // s.NV if s.NV < mk.WAVE else 1
    s.chunk_rows = s.rpl * mk.ROW_STEPS
    s.nseg = -(-s.nt // s.chunk_rows)
    s.units = -(-s.NV // mk.WAVE)
    s.nwork = s.nseg * nframes * s.units
    w = min(s.nwork, waves)
    s.per = -(-s.nwork // w)
    s.ranges = -(-s.nwork // s.per)
    s.grid = -(-s.ranges // mk.WAVES_PER_BLOCK)
    return s


def constant_payload(layout, nchan, ntime, quad):
    """One payload in which every sample of every channel is `quad` = (xr, xi, yr, yi)."""
    s = np.empty((ntime, 2, nchan, 2), np.int8)
    s[:, 0, :, 0], s[:, 0, :, 1], s[:, 1, :, 0], s[:, 1, :, 1] = quad
    if layout == CF:
        s = s.transpose(2, 0, 1, 3)
    elif layout == TF:
        s = s.transpose(0, 2, 1, 3)
    return np.ascontiguousarray(s).reshape(-1).view(np.uint8)


def constant_expected(per_sample, nrows, bin_rows, first_row=0):
    """Sums per bin of `nrows` rows of a constant quad, in Python integers -> int64 (nbins, 4)."""
    nbins = (first_row + nrows - 1) // bin_rows + 1
    out = np.zeros((nbins, 4), np.int64)
    for b in range(nbins):
        n = min((b + 1) * bin_rows, first_row + nrows) - max(b * bin_rows, first_row)
        out[b] = [v * max(n, 0) for v in per_sample]
    return out


# ---- the kernel's arithmetic ------------------------------------------------------------------------------

def sdot4(a, b):
    """v_dot4_i32_i8 without an addend: uint32 arrays -> the sum of the four products of their signed bytes."""
    a8 = np.ascontiguousarray(a, np.uint32).view(np.int8).reshape(-1, 4).astype(np.int64)
    b8 = np.ascontiguousarray(b, np.uint32).view(np.int8).reshape(-1, 4).astype(np.int64)
    return (a8 * b8).sum(1)


def quad_sums(w):
    """bb_coh_quad: dwords (xr, xi, yr, yi) -> int64 (n, 4)."""
    w = np.ascontiguousarray(w, np.uint32)
    return np.stack((sdot4(w, w & 0x0000ffff), sdot4(w, w & 0xffff0000), sdot4(w, w >> 16),
                     sdot4(w, (w >> 8) & 0xff00) - sdot4(w, w >> 24)), -1)


def pair_sums(x, y):
    """bb_coh_pair: dwords (xr0, xi0, xr1, xi1) and (yr0, yi0, yr1, yi1) -> int64 (n, 2 channels, 4)."""
    x, y = np.ascontiguousarray(x, np.uint32), np.ascontiguousarray(y, np.uint32)
    lo = np.stack((sdot4(x, x & 0x0000ffff), sdot4(y, y & 0x0000ffff), sdot4(x, y & 0x0000ffff),
                   sdot4(x, (y << 8) & 0x0000ff00) - sdot4(x, (y >> 8) & 0x000000ff)), -1)
    hi = np.stack((sdot4(x, x & 0xffff0000), sdot4(y, y & 0xffff0000), sdot4(x, y & 0xffff0000),
                   sdot4(x, (y << 8) & 0xff000000) - sdot4(x, (y >> 8) & 0x00ff0000)), -1)
    return np.stack((lo, hi), 1)
