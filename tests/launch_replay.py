"""Runs one recorded launch case (tests/golden/launch_notes.json) on the GPU and
answers what the table pins: the exact bb_last_kernel() note -- kernel, template
arguments, grid, work-item geometry -- and the SHA-256 of the output bytes.  Used by
tests/test_launch_notes_gpu.py and by oracle/gen_golden_launch_notes.py, which records
the table.  Inputs come from a NumPy generator seeded by the case's id.

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


def _decode(case, rng):
    import torch
    from baseband_amd import kernels
    a = case['args']
    nslot, chunk, pn, nframes = a.get('nslot', 1), a.get('chunk', 1), a['payload'], a['nframes']
    head, stride = 32, pn + 32
    nfs = nframes * nslot
    raw = rng.integers(0, 256, head + nfs * stride, dtype=np.uint8)
    dbuf = kernels.to_device_bytes(raw)
    cplx = bool(a.get('complex', False))
    kw = dict(chunk=chunk, nslot=nslot, complex_data=cplx, fill_value=(-2.5 + 1.5j) if cplx else -2.5)
    if a.get('index', False):
        kw['src'] = torch.from_numpy(_index(nfs, head, stride, raw.size, pn)).cuda()
    else:
        kw.update(src0=head, src_stride=stride)
    if 'within' in a:
        kw['within'] = torch.tensor(a['within'], dtype=torch.int32, device='cuda')
        if a.get('out_offset', 0):                          # an output off the 16-byte grid: scalar stores
            nelem = nfs * (pn * 8 // a['bps']) // chunk * len(a['within'])
            kw['out'] = torch.empty(nelem + 4, dtype=torch.float32, device='cuda')[a['out_offset']:a['out_offset'] + nelem]
    else:
        kw['out_dtype'] = getattr(torch, OUT_DTYPES[a.get('out', 'f32')])
    return kernels.decode_frames(dbuf, nframes, pn, a['coder'], a['bps'], **kw)


def _mark4(case, rng):
    import torch
    from baseband_amd import kernels
    a = case['args']
    ntrack, nwords, nframes = a['ntrack'], a['nwords'], a['nframes']
    unit = nwords * ntrack // 8
    stride = unit + 64
    raw = rng.integers(0, 256, nframes * stride, dtype=np.uint8)
    dbuf = kernels.to_device_bytes(raw)
    perm = rng.permutation(ntrack)
    sign, mag = [int(x) for x in perm[:ntrack // 2]], [int(x) for x in perm[ntrack // 2:]]
    nout = a.get('nout', 0)
    if nout:
        sign, mag = sign[:nout], mag[:nout]
    src = torch.from_numpy(_index(nframes, 0, stride, raw.size, unit)).cuda()
    return kernels.decode_mark4(dbuf, nframes, ntrack, nwords, sign, mag, fill_words=a.get('fill_words', 0), src=src,
                                fill_value=-2.5, select=bool(nout))


def _tiled(case, rng):
    import torch
    from baseband_amd import kernels
    a = case['args']
    layout, npol, nchan, T, head, nfr = a['layout'], a['npol'], a['nchan'], a['ntime'], a['head'], a['nframes']
    stored, nps = a.get('nchan_stored', 0), a.get('npol_stored', 0)
    pn = T * (nps or npol) * (stored or nchan) * 2
    stride = pn + head + (-(pn + head)) % 16 if a.get('pad16', True) else pn + head
    raw = rng.integers(0, 256, nfr * stride, dtype=np.uint8)
    dbuf = kernels.to_device_bytes(raw)
    kw = dict(nchan_stored=stored, npol_stored=nps, pol_first=a.get('pol_first', 0), fill_value=3 - 4j)
    if 'chan_map' in a:
        kw['chan_map'] = torch.tensor(a['chan_map'], dtype=torch.int32, device='cuda')
    if a.get('index', False):
        src = head + np.arange(nfr, dtype=np.int64) * stride
        src[1] = -1
        kw['src'] = torch.from_numpy(src).cuda()
    else:
        kw.update(src0=head, src_stride=stride)
    return kernels.decode_i8_tiled(dbuf, nfr, layout, npol, nchan, T, a['t_lo'], a['t_hi'], **kw)


def _copy(case, rng):
    from baseband_amd import kernels
    a = case['args']
    raw = rng.integers(0, 256, a['src0'] + a['nframes'] * a['stride'], dtype=np.uint8)
    return kernels.copy_frames(kernels.to_device_bytes(raw), a['nframes'], a['n'], src0=a['src0'], src_stride=a['stride'])


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


def run(case):
    """-> (bb_last_kernel() note, SHA-256 of the output bytes) of one case."""
    import torch
    from baseband_amd import kernels, _lib
    knobs = case.get('tune', {})
    try:
        for k, v in knobs.items():
            kernels.tune(getattr(_lib, 'TUNE_' + k), v)
        out = OPS[case['op']](case, _rng(case))
        note = _lib.last_kernel()
    finally:
        for k in knobs:
            kernels.tune(getattr(_lib, 'TUNE_' + k), KNOB_DEFAULTS[k])
    data = out.contiguous().view(torch.uint8).cpu().numpy()
    return note, hashlib.sha256(data.tobytes()).hexdigest()
