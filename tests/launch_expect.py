"""What every decode, Mark 4, tiled and copy case of tests/golden/launch_notes.json must write,
worked out on the CPU in NumPy: `expected(case)` gives the exact output, in the output's
element type (float32; uint16 patterns for float16 / bfloat16).  The inputs are the ones
tests/launch_replay.py uploads (its builders, its generator); the values come from
oracle/bb_oracle_np.py and the layouts from include/bbdecode.h.  torch is used for the
bfloat16 rounding of `half_bits` only; nothing here touches a GPU.

tests/test_launch_expect.py compares the SHA-256 of these arrays with the recorded ones,
tests/test_decode_guard_gpu.py compares them with what the kernels write into a guarded,
poisoned output."""
import numpy as np

import bb_oracle_np as orc
import launch_replay as lr

CODER_NAMES = {0: 'vdif', 1: 'mark5b', 2: 'int'}
OUT_TYPES = {'f32': 0, 'f16': 1, 'bf16': 2}
DECODE_FILL = -2.5, 1.5             # launch_replay._decode: (re, im); re alone for real data
MARK4_FILL = -2.5
TILED_FILL = 3.0, -4.0
OPS = ('decode', 'mark4', 'tiled', 'copy')


def _follows(o, size, unit):
    """Does a decode follow index entry `o`?  Only when the whole unit lies inside the buffer."""
    return 0 <= o <= size - unit


def as_out_type(x, out):
    """float32 values -> the elements a decode with output type `out` writes."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if out == 'f32':
        return x
    from test_half_abi import half_bits
    return half_bits(x.reshape(-1), OUT_TYPES[out]).reshape(x.shape)


def decode_values(raw, src, nframes, nslot, chunk, pn, coder, bps, cplx, fill=DECODE_FILL, within=None):
    """bb_decode_frames / bb_decode_frames_select: float32 (frame, row, slot, chunk or kept position)."""
    nval = pn * 8 // bps
    rows = nval // chunk
    full = np.empty((nframes, rows, nslot, chunk), np.float32)
    fill_row = np.full(chunk, fill[0], np.float32)
    if cplx:
        fill_row[1::2] = fill[1]
    for f in range(nframes):
        for s in range(nslot):
            o = int(src[f * nslot + s])
            if _follows(o, raw.size, pn):
                full[f, :, s, :] = orc.decode_flat(raw[o:o + pn], CODER_NAMES[coder], bps).reshape(rows, chunk)
            else:
                full[f, :, s, :] = fill_row
    return full if within is None else np.ascontiguousarray(full[..., list(within)])


def mark4_values(raw, src, nframes, ntrack, nwords, sign, mag, fill_words, fill=MARK4_FILL):
    """bb_decode_mark4 / _select: float32 (frame, word, output)."""
    levels = np.sort(orc.code_levels('vdif', 2))
    unit = nwords * ntrack // 8
    out = np.empty((nframes, nwords, len(sign)), np.float32)
    sign, mag = np.array(sign, np.uint64), np.array(mag, np.uint64)
    one = np.uint64(1)
    for f in range(nframes):
        o = int(src[f])
        if not _follows(o, raw.size, unit):
            out[f] = fill
            continue
        w = raw[o:o + unit].copy().view(orc.MARK4_DTYPES[ntrack]).astype(np.uint64)[:, None]
        out[f] = levels[(2 * ((w >> sign) & one) + ((w >> mag) & one)).astype(np.intp)]
        out[f, :fill_words] = fill
    return out


def tiled_values(raw, src, nframes, layout, npol, nchan, ntime, t_lo, t_hi, nchan_stored=0, npol_stored=0, pol_first=0,
                 chan_map=None, fill=TILED_FILL):
    """bb_decode_i8_tiled: float32 (frame, time, pol, chan, re / im)."""
    ncs, nps = nchan_stored or nchan, npol_stored or npol
    pn = ntime * nps * ncs * 2
    chans = list(chan_map) if chan_map is not None else list(range(nchan))
    out = np.empty((nframes, t_hi - t_lo, npol, nchan, 2), np.float32)
    for f in range(nframes):
        o = int(src[f])
        if not _follows(o, raw.size, pn):
            out[f] = np.array(fill, np.float32)
            continue
        b = raw[o:o + pn].view(np.int8).astype(np.float32)
        if layout == 0:
            v = b.reshape(ncs, ntime, nps, 2).transpose(1, 2, 0, 3)
        elif layout == 1:
            v = b.reshape(ntime // 256, nps, ncs, 256, 2).transpose(0, 3, 1, 2, 4).reshape(ntime, nps, ncs, 2)
        else:
            v = b.reshape(ntime, ncs, nps, 2).transpose(0, 2, 1, 3)
        out[f] = v[t_lo:t_hi, pol_first:pol_first + npol][:, :, chans]
    return out


def copy_values(raw, nframes, n, src0, stride):
    """bb_copy_frames: the runs, back to back, as float32."""
    return np.concatenate([raw[src0 + f * stride:src0 + f * stride + n] for f in range(nframes)]).view(np.float32)


def fixed_index(n, first, stride):
    return first + np.arange(n, dtype=np.int64) * stride


def expected(case):
    """-> flat ndarray: the output of `case` (float32, or uint16 patterns of float16 / bfloat16)."""
    a, rng = case['args'], lr._rng(case)
    if case['op'] == 'decode':
        raw, head, stride, src = lr.decode_inputs(case, rng)
        nslot = a.get('nslot', 1)
        if src is None:
            src = fixed_index(a['nframes'] * nslot, head, stride)
        v = decode_values(raw, src, a['nframes'], nslot, a.get('chunk', 1), a['payload'], a['coder'], a['bps'],
                          bool(a.get('complex', False)), within=a.get('within'))
        return as_out_type(v, a.get('out', 'f32')).reshape(-1)
    if case['op'] == 'mark4':
        raw, unit, sign, mag, src = lr.mark4_inputs(case, rng)
        return mark4_values(raw, src, a['nframes'], a['ntrack'], a['nwords'], sign, mag, a.get('fill_words', 0)).reshape(-1)
    if case['op'] == 'tiled':
        raw, pn, stride, src = lr.tiled_inputs(case, rng)
        if src is None:
            src = fixed_index(a['nframes'], a['head'], stride)
        return tiled_values(raw, src, a['nframes'], a['layout'], a['npol'], a['nchan'], a['ntime'], a['t_lo'], a['t_hi'],
                            a.get('nchan_stored', 0), a.get('npol_stored', 0), a.get('pol_first', 0),
                            a.get('chan_map')).reshape(-1)
    if case['op'] == 'copy':
        return copy_values(lr.copy_inputs(case, rng), a['nframes'], a['n'], a['src0'], a['stride'])
    raise KeyError(case['op'])
