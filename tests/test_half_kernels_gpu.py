"""Raw C-ABI decode to float16 / bfloat16 (k_half.h) against the CPU oracle, on
the GPU.  Expected value of every element, no tolerance: the 16-bit pattern of
the float32 value the oracle gives, converted by ``ndarray.astype(float16)`` /
``Tensor.to(bfloat16)`` on the CPU; comparisons are on the integer view."""
import numpy as np
import pytest

import bb_oracle_np as orc
from conftest import bits_equal
from test_half_abi import half_bits
from test_kernels_gpu import CODERS, COMBOS

pytestmark = pytest.mark.gpu

TYPES = [1, 2]          # BB_OUT_F16, BB_OUT_BF16


def _torch():
    import torch
    return torch


def _dtype(out_type):
    torch = _torch()
    return {1: torch.float16, 2: torch.bfloat16}[out_type]


def bits16(t):
    """uint16 patterns of a float16 / bfloat16 tensor."""
    return t.view(_torch().int16).cpu().numpy().view(np.uint16)


def ran_half_kernel(flat):
    from baseband_amd import _lib
    name = _lib.last_kernel()
    return name.startswith('k_decode_half_flat<' if flat else 'k_decode_half_rows<')


@pytest.mark.parametrize('out_type', TYPES)
@pytest.mark.parametrize('coder,bps', COMBOS)
@pytest.mark.parametrize('nbytes', [8, 256, 1000, 8000, 8192 + 24, 70000])
def test_flat_decode_single_payload(coder, bps, nbytes, out_type):
    from baseband_amd import kernels
    rng = np.random.default_rng(bps * 1000 + nbytes)
    raw = rng.integers(0, 256, nbytes, dtype=np.uint8)
    dbuf = kernels.to_device_bytes(raw)
    out = kernels.decode_frames(dbuf, 1, nbytes, CODERS[coder], bps, out_dtype=_dtype(out_type))
    assert out.dtype == _dtype(out_type) and ran_half_kernel(True)
    assert np.array_equal(bits16(out), half_bits(orc.decode_flat(raw, coder, bps), out_type))


@pytest.mark.parametrize('out_type', TYPES)
@pytest.mark.parametrize('coder,bps', COMBOS)
def test_all_byte_values(coder, bps, out_type):
    from baseband_amd import kernels
    raw = np.repeat(np.arange(256, dtype=np.uint8), 4)       # dword multiples
    out = kernels.decode_frames(kernels.to_device_bytes(raw), 1, raw.size, CODERS[coder], bps,
                                out_dtype=_dtype(out_type))
    assert ran_half_kernel(True)
    assert np.array_equal(bits16(out), half_bits(orc.decode_flat(raw, coder, bps), out_type))


@pytest.mark.parametrize('out_type', TYPES)
@pytest.mark.parametrize('bps,chunk,nslot', [(2, 1, 8), (2, 2, 4), (2, 32, 8),
                                             (4, 4, 2), (8, 2, 4), (1, 16, 3),
                                             (2, 4, 5), (8, 1, 2), (4, 1, 2),
                                             (2, 8, 8), (2, 16, 2), (8, 4, 8), (8, 16, 4),
                                             (1, 4, 2), (4, 8, 16), (2, 64, 2), (2, 128, 4),
                                             (8, 64, 2), (2, 4, 1 + 2)])
def test_multislot_interleave_and_fill(bps, chunk, nslot, out_type):
    """Frame-set layout (vdif/frame.py:402-434) with missing/invalid frames:
    tests/test_kernels_gpu.py::test_multislot_interleave_and_fill in 16 bits."""
    torch = _torch()
    from baseband_amd import kernels
    nframes, pn = 7, 640
    rng = np.random.default_rng(bps * 100 + chunk * 10 + nslot)
    raw = rng.integers(0, 256, nframes * nslot * pn, dtype=np.uint8)
    perm = rng.permutation(nframes * nslot)
    src = (perm * pn).astype(np.int64)
    missing = rng.choice(nframes * nslot, size=5, replace=False)
    src[missing] = -1
    cplx = chunk % 2 == 0
    fill = -7.5
    out = kernels.decode_frames(
        kernels.to_device_bytes(raw), nframes, pn, 0, bps, chunk=chunk,
        nslot=nslot, src=torch.from_numpy(src).cuda(), complex_data=cplx,
        fill_value=fill, out_dtype=_dtype(out_type))
    assert ran_half_kernel(False)
    E = pn * 8 // bps
    R = E // chunk
    exp = np.empty((nframes, R, nslot, chunk), np.float32)
    fillrow = np.tile(np.array([fill, 0.], np.float32), chunk // 2) if cplx \
        else np.full(chunk, fill, np.float32)
    for f in range(nframes):
        for s in range(nslot):
            o = src[f * nslot + s]
            if o < 0:
                exp[f, :, s, :] = fillrow
            else:
                exp[f, :, s, :] = orc.decode_flat(raw[o:o + pn], 'vdif', bps).reshape(R, chunk)
    assert np.array_equal(bits16(out), half_bits(exp.reshape(-1), out_type))


@pytest.mark.parametrize('out_type', TYPES)
@pytest.mark.parametrize('bps,chunk,nslot,pn', [(2, 4, 8, 4000), (2, 8, 8, 4000), (8, 2, 3, 20), (8, 4, 5, 36),
                                                (2, 4096, 2, 8192), (1, 2, 1024, 64), (4, 8, 2, 20000),
                                                (8, 16384, 3, 32768)])
def test_interleave_geometries(bps, chunk, nslot, pn, out_type):
    """Thread interleave beyond the shapes above: work items of several rows and of
    part of a row (chunk wider than an item), many slots, frames whose output is
    8-byte aligned only (8-bit samples, odd dword count, odd slot count), payloads at
    odd addresses, fixed stride (no index)."""
    torch = _torch()
    from baseband_amd import kernels
    nframes = 5
    rng = np.random.default_rng(bps + chunk + nslot + pn)
    stride = pn + 36
    nfs = nframes * nslot
    raw = rng.integers(0, 256, stride * (nfs + 1) + 8, dtype=np.uint8)
    dbuf = kernels.to_device_bytes(raw)
    src = (rng.permutation(nfs) * stride + 36).astype(np.int64)
    src[1] += 1
    src[nfs - 2] += 3
    src[[2, nfs - 1]] = -1
    cplx = chunk % 2 == 0
    fill = (2 - 1j) if cplx else 9.
    E = pn * 8 // bps
    R = E // chunk
    fillrow = np.tile(np.array([2., -1.], np.float32), chunk // 2) if cplx else np.full(chunk, 9., np.float32)

    def expected(offsets):
        exp = np.empty((nframes, R, nslot, chunk), np.float32)
        for f in range(nframes):
            for s in range(nslot):
                o = offsets[f * nslot + s]
                exp[f, :, s, :] = fillrow if o < 0 else orc.decode_flat(raw[o:o + pn], 'vdif', bps).reshape(R, chunk)
        return half_bits(exp.reshape(-1), out_type)

    out = kernels.decode_frames(dbuf, nframes, pn, 0, bps, chunk=chunk, nslot=nslot,
                                src=torch.from_numpy(src).cuda(), complex_data=cplx, fill_value=fill,
                                out_dtype=_dtype(out_type))
    assert ran_half_kernel(False)
    assert np.array_equal(bits16(out), expected(src))
    out = kernels.decode_frames(dbuf, nframes, pn, 0, bps, chunk=chunk, nslot=nslot, src0=36, src_stride=stride,
                                out_dtype=_dtype(out_type))
    assert ran_half_kernel(False)
    assert np.array_equal(bits16(out), expected(36 + np.arange(nfs) * stride))


def _lut16(coder, bps, out_type):
    """byte -> its 8 / bps elements as 16-bit patterns, from the oracle's decode of
    all byte values."""
    return half_bits(orc.decode_flat(np.arange(256, dtype=np.uint8), coder, bps), out_type).reshape(256, 8 // bps)


@pytest.mark.parametrize('out_type', TYPES)
@pytest.mark.parametrize('coder,bps,frame,hdr', [('vdif', 2, 8032, 32), ('mark5b', 2, 10016, 16),
                                                 ('vdif', 8, 8032, 32), ('int', 8, 8192, 0),
                                                 ('vdif', 1, 8032, 32), ('vdif', 4, 8032, 32)])
def test_fixed_stride_many_frames(coder, bps, frame, hdr, out_type):
    """4,096 frames at a fixed stride: the permuted work dealing and several work
    items per frame; guard elements around the output stay untouched."""
    torch = _torch()
    from baseband_amd import kernels
    n, pn = 4096, frame - hdr
    rng = np.random.default_rng(frame + bps)
    raw = rng.integers(0, 256, frame * n, dtype=np.uint8)
    nelem = n * pn * 8 // bps
    whole = torch.full((nelem + 16,), 0x5a5a, dtype=torch.int16, device='cuda').view(_dtype(out_type))
    out = kernels.decode_frames(kernels.to_device_bytes(raw), n, pn, CODERS[coder], bps, src0=hdr,
                                src_stride=frame, out=whole[8:8 + nelem], out_dtype=_dtype(out_type))
    assert out.data_ptr() == whole.data_ptr() + 16 and ran_half_kernel(True)
    got = bits16(whole)
    assert np.all(got[:8] == 0x5a5a) and np.all(got[-8:] == 0x5a5a)
    exp = _lut16(coder, bps, out_type)[raw.reshape(n, frame)[:, hdr:]]
    assert np.array_equal(got[8:-8], exp.reshape(-1))


@pytest.mark.parametrize('out_type', TYPES)
@pytest.mark.parametrize('coder,bps', COMBOS)
@pytest.mark.parametrize('pn', [260, 1000, 8000, 10000])
def test_index_odd_addresses_bad_entries_and_fill(coder, bps, pn, out_type):
    """Contiguous output through an index: shuffled payloads, payloads at odd byte
    addresses, missing frames, entries that point outside the buffer (fill, nothing
    read), complex fill, a fill value float16 cannot hold (1e5 -> +inf; finite in
    bfloat16), and untouched guard elements around the output."""
    torch = _torch()
    from baseband_amd import kernels
    rng = np.random.default_rng(pn + bps + 10 * CODERS[coder])
    nframes = 37
    stride = pn + 32
    raw = rng.integers(0, 256, stride * (nframes + 3) + 16, dtype=np.uint8)
    dbuf = kernels.to_device_bytes(raw)
    order = rng.permutation(nframes + 3)[:nframes]
    src = (order * stride + 32).astype(np.int64)
    src[3] += 1
    src[9] += 2
    src[11] += 3
    src[[0, 5, 20, nframes - 1]] = -1
    src[6] = raw.size - pn + 4                  # the payload would end outside the buffer
    src[7] = raw.size + (1 << 40)
    src[8] = -(1 << 33)
    dsrc = torch.from_numpy(src).cuda()
    E = pn * 8 // bps
    inside = (src >= 0) & (src + pn <= raw.size)
    dt = _dtype(out_type)

    def expected(fill_pair):
        want = np.empty((nframes, E), np.uint16)
        for f, o in enumerate(src):
            want[f] = half_bits(orc.decode_flat(raw[o:o + pn], coder, bps), out_type) if inside[f] \
                else np.tile(half_bits(np.array(fill_pair, np.float32), out_type), E // 2)
        return want.reshape(-1)

    whole = torch.full((nframes * E + 16,), 0x5a5a, dtype=torch.int16, device='cuda').view(dt)
    kernels.decode_frames(dbuf, nframes, pn, CODERS[coder], bps, src=dsrc, fill_value=-2.5,
                          out=whole[8:-8], out_dtype=dt)
    assert ran_half_kernel(True)
    got = bits16(whole)
    assert np.all(got[:8] == 0x5a5a) and np.all(got[-8:] == 0x5a5a)
    assert np.array_equal(got[8:-8], expected([-2.5, -2.5]))
    c = kernels.decode_frames(dbuf, nframes, pn, CODERS[coder], bps, src=dsrc, complex_data=True,
                              fill_value=1 - 3j, out_dtype=dt)
    assert np.array_equal(bits16(c), expected([1., -3.]))
    big = kernels.decode_frames(dbuf, nframes, pn, CODERS[coder], bps, src=dsrc, fill_value=1e5, out_dtype=dt)
    fill_bits = bits16(big).reshape(nframes, E)[0]
    assert np.all(fill_bits == (0x7c00 if out_type == 1 else half_bits(np.array([1e5], np.float32), 2)[0]))
    assert np.array_equal(bits16(big), expected([1e5, 1e5]))
    if out_type == 2:
        assert np.isfinite(big.float().cpu().numpy()).all()


def test_float32_launches_in_between_are_unchanged():
    """out_type 0 still takes today's kernels and gives today's bits, before and
    after 16-bit launches on the same thread."""
    torch = _torch()
    from baseband_amd import kernels, _lib
    rng = np.random.default_rng(77)
    raw = rng.integers(0, 256, 8032 * 64, dtype=np.uint8)
    dbuf = kernels.to_device_bytes(raw)
    exp = np.concatenate([orc.decode_flat(raw[i * 8032 + 32:(i + 1) * 8032], 'vdif', 2) for i in range(64)])
    src = torch.arange(64 * 8, dtype=torch.int64, device='cuda') * 1004 + 32
    for dt, ot in ((torch.float16, 1), (torch.bfloat16, 2)):
        a = kernels.decode_frames(dbuf, 64, 8000, 0, 2, src0=32, src_stride=8032)
        assert _lib.last_kernel().startswith('k_decode_flat_lds<2,') and a.dtype == torch.float32
        h = kernels.decode_frames(dbuf, 64, 8000, 0, 2, src0=32, src_stride=8032, out_dtype=dt)
        assert _lib.last_kernel().startswith('k_decode_half_flat<2,') and ('bf16' in _lib.last_kernel()) == (ot == 2)
        b = kernels.decode_frames(dbuf, 64, 8000, 0, 2, src0=32, src_stride=8032)
        assert _lib.last_kernel().startswith('k_decode_flat_lds<2,')
        assert bits_equal(a.cpu().numpy(), exp) and bits_equal(b.cpu().numpy(), exp)
        assert np.array_equal(bits16(h), half_bits(exp, ot))
        r32 = kernels.decode_frames(dbuf, 64, 1000, 0, 2, chunk=8, nslot=8, src=src, complex_data=True)
        k32 = _lib.last_kernel()
        r16 = kernels.decode_frames(dbuf, 64, 1000, 0, 2, chunk=8, nslot=8, src=src, complex_data=True, out_dtype=dt)
        assert _lib.last_kernel().startswith('k_decode_half_rows<2>')
        again = kernels.decode_frames(dbuf, 64, 1000, 0, 2, chunk=8, nslot=8, src=src, complex_data=True)
        assert _lib.last_kernel() == k32 and not k32.startswith('k_decode_half')
        assert bits_equal(r32.cpu().numpy(), again.cpu().numpy())
        assert np.array_equal(bits16(r16), half_bits(r32.cpu().numpy(), ot))


def test_argument_errors_and_unknown_type():
    torch = _torch()
    import ctypes as C
    from baseband_amd import kernels, _lib
    dbuf = torch.zeros(1024, dtype=torch.uint8, device='cuda')
    out = torch.full((4096,), 0x5a5a, dtype=torch.int16, device='cuda')
    p = _lib.DecodeParams()
    p.coder, p.bps, p.chunk, p.nslot, p.payload_nbytes = 0, 2, 1, 1, 64

    def launch(nelem=4096, optr=None):
        return _lib.lib.bb_decode_frames(dbuf.data_ptr(), 1024, None, 1, C.byref(p),
                                         out.data_ptr() if optr is None else optr, nelem, None)
    for bad in (3, -1, 1 << 16):
        p.out_type = bad
        assert launch() == _lib.BB_EINVAL
    p.out_type = _lib.OUT_F16
    assert launch(255) == _lib.BB_ERANGE                    # 256 elements wanted (counted in elements)
    assert launch(optr=out.data_ptr() + 8) == _lib.BB_EINVAL    # 16-byte alignment as for float32
    p.src0 = 1024 - 60
    assert launch() == _lib.BB_ERANGE                       # the payload ends outside the buffer
    torch.cuda.synchronize()
    assert bool((out == 0x5a5a).all())
    p.src0 = 0
    assert launch(256) == _lib.BB_OK
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint16)
    assert np.all(got[:256] == _lib.levels_as(0, 2, _lib.OUT_F16)[0]) and np.all(got[256:] == 0x5a5a)
    with pytest.raises(TypeError):
        kernels.decode_frames(dbuf, 1, 64, 0, 2, out_dtype=torch.float64)
    with pytest.raises(TypeError):                          # the output tensor's type is the decode's
        kernels.decode_frames(dbuf, 1, 64, 0, 2, out=torch.empty(256, device='cuda'), out_dtype=torch.float16)


@pytest.mark.parametrize('out_type', TYPES)
def test_paths_without_16_bit_kernels_answer_enotsup(out_type):
    """Channel subsets folded into the decode, Mark 4 and the int8 transposes write
    float32 only: asked for a 16-bit type they answer BB_ENOTSUP (KeyError in the
    wrappers) and write nothing."""
    torch = _torch()
    from baseband_amd import kernels, _lib
    dt = _dtype(out_type)
    dbuf = torch.zeros(1 << 16, dtype=torch.uint8, device='cuda')
    out = torch.full((1 << 16,), 0x5a5a, dtype=torch.int16, device='cuda')
    within = torch.tensor([0, 2], dtype=torch.int32, device='cuda')
    src = torch.zeros(2, dtype=torch.int64, device='cuda')
    with pytest.raises(KeyError):
        kernels.decode_frames(dbuf, 1, 4000, 0, 2, chunk=4, nslot=2, src=src, within=within,
                              out=out.view(dt), out_dtype=dt)
    assert kernels.decode_frames(dbuf, 1, 4000, 0, 2, chunk=4, nslot=2, src=src, within=within).dtype == torch.float32
    sign, mag = list(range(0, 32, 2)), list(range(1, 32, 2))
    with pytest.raises(KeyError):
        kernels.decode_mark4(dbuf, 1, 32, 2500, sign, mag, out=out.view(dt)[:2500 * 16], out_dtype=dt)
    assert kernels.decode_mark4(dbuf, 1, 32, 2500, sign, mag).dtype == torch.float32
    with pytest.raises(KeyError):
        kernels.decode_mark4(dbuf, 1, 32, 2500, sign[:4], mag[:4], select=True, out=out.view(dt), out_dtype=dt)
    with pytest.raises(KeyError):
        kernels.decode_i8_tiled(dbuf, 1, _lib.LAYOUT_GUPPI_TF, 2, 8, 64, 0, 64, out=out.view(dt)[:64 * 32],
                                out_dtype=dt)
    assert kernels.decode_i8_tiled(dbuf, 1, _lib.LAYOUT_GUPPI_TF, 2, 8, 64, 0, 64).dtype == torch.float32
    torch.cuda.synchronize()
    assert bool((out == 0x5a5a).all())
