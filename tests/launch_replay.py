"""Runs one recorded launch case (tests/golden/launch_notes.json) on the GPU and
answers what the table pins: the exact bb_last_kernel() note -- kernel, template
arguments, grid, work-item geometry -- and the SHA-256 of the output bytes.  Used by
tests/test_launch_notes_gpu.py and by oracle/gen_golden_launch_notes.py, which records
the table.  Inputs come from a NumPy generator seeded by the case's id; the builders
(`decode_inputs` & co.) are shared with tests/launch_expect.py, which works out on the CPU
what each case must write, and `launch(case, out=...)` with tests/test_decode_guard_gpu.py,
which decodes into guarded outputs.

Cases that decode through an index carry one -1 entry and one entry whose unit would
end past the buffer, so every kernel's fill path runs."""
import hashlib
import zlib

import numpy as np

# knob -> the value that restores the library's default
KNOB_DEFAULTS = {'BLOCKS': 0, 'VDIF8_LDS_GIB': -1, 'M4_WIDEN': 1, 'TILED_STAGE': 1, 'XPOSE': 1}
OUT_DTYPES = {'f32': 'float32', 'f16': 'float16', 'bf16': 'bfloat16'}


def _rng(case):
    return np.random.default_rng(zlib.crc32(case['id'].encode()))


def _index(nunits, head, stride, raw_size, unit_bytes):
    src = head + np.arange(nunits, dtype=np.int64) * stride
    src[1] = -1                                             # a missing unit
    src[nunits - 2] = raw_size - unit_bytes + 8             # would end past the buffer
    return src


# ---- inputs of the decode, Mark 4, tiled and copy cases: NumPy only, shared with tests/launch_expect.py,
# which builds the expected output of a case from the same arrays (same generator, same order of draws) ----

def out_nelem(case):
    """Elements of a case's output (float32 values, or 16-bit ones with `out` f16 / bf16)."""
    a = case['args']
    if case['op'] == 'decode':
        n = a['nframes'] * a.get('nslot', 1) * (a['payload'] * 8 // a['bps'])
        return n // a.get('chunk', 1) * len(a['within']) if 'within' in a else n
    if case['op'] == 'mark4':
        return a['nframes'] * a['nwords'] * (a.get('nout', 0) or a['ntrack'] // 2)
    if case['op'] == 'tiled':
        return a['nframes'] * (a['t_hi'] - a['t_lo']) * a['npol'] * a['nchan'] * 2
    return a['nframes'] * a['n'] // 4


def decode_inputs(case, rng):
    """-> raw bytes, offset of the first payload, stride, index (one entry per frame-slot; None: fixed stride)."""
    a = case['args']
    nfs, pn = a['nframes'] * a.get('nslot', 1), a['payload']
    head, stride = 32, pn + 32
    raw = rng.integers(0, 256, head + nfs * stride, dtype=np.uint8)
    src = _index(nfs, head, stride, raw.size, pn) if a.get('index', False) else None
    return raw, head, stride, src


def mark4_inputs(case, rng):
    """-> raw bytes, bytes per unit, sign map, magnitude map (cut to `nout`), index."""
    a = case['args']
    ntrack, nwords, nframes = a['ntrack'], a['nwords'], a['nframes']
    unit = nwords * ntrack // 8
    stride = unit + 64
    raw = rng.integers(0, 256, nframes * stride, dtype=np.uint8)
    perm = rng.permutation(ntrack)
    sign, mag = [int(x) for x in perm[:ntrack // 2]], [int(x) for x in perm[ntrack // 2:]]
    nout = a.get('nout', 0)
    if nout:
        sign, mag = sign[:nout], mag[:nout]
    return raw, unit, sign, mag, _index(nframes, 0, stride, raw.size, unit)


def tiled_inputs(case, rng):
    """-> raw bytes, payload bytes, stride, index (None: fixed stride from `head`)."""
    a = case['args']
    T, head, nfr = a['ntime'], a['head'], a['nframes']
    pn = T * (a.get('npol_stored', 0) or a['npol']) * (a.get('nchan_stored', 0) or a['nchan']) * 2
    stride = pn + head + (-(pn + head)) % 16 if a.get('pad16', True) else pn + head
    raw = rng.integers(0, 256, nfr * stride, dtype=np.uint8)
    src = None
    if a.get('index', False):
        src = head + np.arange(nfr, dtype=np.int64) * stride
        src[1] = -1
    return raw, pn, stride, src


def copy_inputs(case, rng):
    a = case['args']
    return rng.integers(0, 256, a['src0'] + a['nframes'] * a['stride'], dtype=np.uint8)


# ---- the launches.  `out`: the tensor to decode into (tests/test_decode_guard_gpu.py passes a view of a
# poisoned allocation); None: the wrapper allocates, as when the table was recorded ----

def _decode(case, rng, out=None):
    import torch
    from baseband_amd import kernels
    a = case['args']
    nslot, chunk, pn, nframes = a.get('nslot', 1), a.get('chunk', 1), a['payload'], a['nframes']
    raw, head, stride, src = decode_inputs(case, rng)
    dbuf = kernels.to_device_bytes(raw)
    cplx = bool(a.get('complex', False))
    kw = dict(chunk=chunk, nslot=nslot, complex_data=cplx, fill_value=(-2.5 + 1.5j) if cplx else -2.5, out=out)
    if src is not None:
        kw['src'] = torch.from_numpy(src).cuda()
    else:
        kw.update(src0=head, src_stride=stride)
    if 'within' in a:
        kw['within'] = torch.tensor(a['within'], dtype=torch.int32, device='cuda')
        if out is None and a.get('out_offset', 0):          # an output off the 16-byte grid: scalar stores
            nelem = out_nelem(case)
            kw['out'] = torch.empty(nelem + 4, dtype=torch.float32, device='cuda')[a['out_offset']:a['out_offset'] + nelem]
    else:
        kw['out_dtype'] = getattr(torch, OUT_DTYPES[a.get('out', 'f32')])
    return kernels.decode_frames(dbuf, nframes, pn, a['coder'], a['bps'], **kw)


def _mark4(case, rng, out=None):
    import torch
    from baseband_amd import kernels
    a = case['args']
    raw, unit, sign, mag, src = mark4_inputs(case, rng)
    dbuf = kernels.to_device_bytes(raw)
    return kernels.decode_mark4(dbuf, a['nframes'], a['ntrack'], a['nwords'], sign, mag, fill_words=a.get('fill_words', 0),
                                src=torch.from_numpy(src).cuda(), fill_value=-2.5, select=bool(a.get('nout', 0)), out=out)


def _tiled(case, rng, out=None):
    import torch
    from baseband_amd import kernels
    a = case['args']
    raw, pn, stride, src = tiled_inputs(case, rng)
    dbuf = kernels.to_device_bytes(raw)
    kw = dict(nchan_stored=a.get('nchan_stored', 0), npol_stored=a.get('npol_stored', 0), pol_first=a.get('pol_first', 0),
              fill_value=3 - 4j, out=out)
    if 'chan_map' in a:
        kw['chan_map'] = torch.tensor(a['chan_map'], dtype=torch.int32, device='cuda')
    if src is not None:
        kw['src'] = torch.from_numpy(src).cuda()
    else:
        kw.update(src0=a['head'], src_stride=stride)
    return kernels.decode_i8_tiled(dbuf, a['nframes'], a['layout'], a['npol'], a['nchan'], a['ntime'], a['t_lo'], a['t_hi'], **kw)


def _copy(case, rng, out=None):
    from baseband_amd import kernels
    a = case['args']
    raw = copy_inputs(case, rng)
    return kernels.copy_frames(kernels.to_device_bytes(raw), a['nframes'], a['n'], src0=a['src0'], src_stride=a['stride'], out=out)


def _encode_flat(case, rng):
    import torch
    from baseband_amd import kernels
    a = case['args']
    x = (rng.standard_normal(a['nelem']) * 2).astype(np.float32)
    return kernels.encode_flat(torch.from_numpy(x).cuda(), a['coder'], a['bps'])


def _encode_mark4(case, rng):
    import torch
    from baseband_amd import kernels
    a = case['args']
    ntrack = a['ntrack']
    x = (rng.standard_normal((a['nwords'], ntrack // 2)) * 2).astype(np.float32)
    perm = rng.permutation(ntrack)
    return kernels.encode_mark4(torch.from_numpy(x).cuda(), ntrack, [int(v) for v in perm[:ntrack // 2]],
                                [int(v) for v in perm[ntrack // 2:]])


OPS = {'decode': _decode, 'mark4': _mark4, 'tiled': _tiled, 'copy': _copy, 'encode_flat': _encode_flat,
       'encode_mark4': _encode_mark4}


def launch(case, out=None):
    """Runs one case with its knobs set -> (bb_last_kernel() note, output tensor).  With `out` (decode, Mark 4,
    tiled and copy cases) the launch is asked to write that tensor."""
    from baseband_amd import kernels, _lib
    knobs = case.get('tune', {})
    try:
        for k, v in knobs.items():
            kernels.tune(getattr(_lib, 'TUNE_' + k), v)
        res = OPS[case['op']](case, _rng(case)) if out is None else OPS[case['op']](case, _rng(case), out)
        note = _lib.last_kernel()
    finally:
        for k in knobs:
            kernels.tune(getattr(_lib, 'TUNE_' + k), KNOB_DEFAULTS[k])
    return note, res


def run(case):
    """-> (bb_last_kernel() note, SHA-256 of the output bytes) of one case."""
    import torch
    note, out = launch(case)
    data = out.contiguous().view(torch.uint8).cpu().numpy()
    return note, hashlib.sha256(data.tobytes()).hexdigest()
