"""bb_recode_frames on the device against NumPy on the bytes alone: every input slot stream
unpacked at bps_in, rows formed across the slots, sent through the table where the payload
is valid and set to fill_code elsewhere, split into the output slots and packed at bps_out
-- exact byte equality.  All 16 pairs of widths at every thread shape, frames that do not
line up and frames that do, payloads through an index (shuffled, odd addresses, missing,
negative, out of bounds) and at a fixed stride, row ranges with a first row, one request
split over two calls, more work items than the launch has waves, equal thread structures
against bb_requant_frames, equal widths against bb_repack_frames, and the argument errors.
Outputs are poisoned and guarded: bytes outside the rows written must still hold the poison."""
import ctypes

import numpy as np
import pytest

import guardkit
from packedkit import _torch, device, whole_rows, indexed_case, judge
from recodekit import (WIDTHS, PAIRS, THREAD_SHAPES, PAYLOADS, fits, byte_unit, lined_up, payloads_out, random_table,
                       Request, nbytes_out, run)

pytestmark = pytest.mark.gpu

CASES = [(bi, bo, si, so) for bi, bo in PAIRS for si, so in THREAD_SHAPES if fits(bi, bo, si[0] * si[1])]


def test_the_cases_are_all_width_pairs_at_all_thread_shapes():
    assert {(bi, bo) for bi, bo, _, _ in CASES} == set(PAIRS)
    assert {(si, so) for _, _, si, so in CASES} == set(THREAD_SHAPES)
    assert len(CASES) == sum(1 for bi, bo in PAIRS for si, _ in THREAD_SHAPES if si[0] * si[1] * max(bi, bo) <= 256)


@pytest.mark.parametrize('bps_in,bps_out,shape_in,shape_out', CASES)
def test_recode_through_an_index(bps_in, bps_out, shape_in, shape_out):
    rng = np.random.default_rng([1, bps_in, bps_out, *shape_in, *shape_out])
    (nslot_in, chunk_in), (nslot_out, chunk_out) = shape_in, shape_out
    u = byte_unit(bps_in, chunk_in, bps_out, chunk_out)
    for nbytes, nframes in PAYLOADS:
        payload_in, lined = lined_up(nbytes, bps_in, chunk_in, bps_out, chunk_out)
        buf, src = indexed_case(rng, payload_in, nframes, nslot_in)
        dbuf, dsrc = device(buf), device(src)
        req = Request(buf, src, nframes, payload_in, bps_in, nslot_in, chunk_in)
        assert req.valid.any() and not req.valid.all()
        hi = req.total // u * u
        outs = payloads_out(lined, bps_out, chunk_out)
        assert lined in outs and len(outs) >= 3
        for payload_out in outs:
            table = random_table(rng, bps_in, bps_out)
            fill = int(rng.integers(0, 1 << bps_out))
            n = nbytes_out(hi, 0, bps_out, shape_out, payload_out)
            whole, view, before = run(dbuf, nframes, payload_in, bps_in, shape_in, bps_out, shape_out, payload_out,
                                      table, fill, n, src=dsrc, row_hi=hi)
            want = req.expect(before, table, bps_out, shape_out, payload_out, fill, 0, hi)
            judge(whole, view, want, (payload_in, nframes, payload_out))


@pytest.mark.parametrize('bps_in,bps_out,shape_in,shape_out', CASES)
def test_recode_at_a_fixed_stride(bps_in, bps_out, shape_in, shape_out):
    rng = np.random.default_rng([2, bps_in, bps_out, *shape_in, *shape_out])
    (nslot_in, chunk_in), (nslot_out, chunk_out) = shape_in, shape_out
    u = byte_unit(bps_in, chunk_in, bps_out, chunk_out)
    for nbytes, nframes in PAYLOADS[1:]:
        payload_in, lined = lined_up(nbytes, bps_in, chunk_in, bps_out, chunk_out)
        src0, stride = 8, payload_in + 4                        # (every other payload off the 16-byte grid)
        n = nframes * nslot_in
        buf = rng.integers(0, 256, src0 + (n - 1) * stride + payload_in, dtype=np.uint8)
        dbuf = device(buf)
        req = Request(buf, src0 + np.arange(n) * stride, nframes, payload_in, bps_in, nslot_in, chunk_in)
        assert req.valid.all()
        hi = req.total // u * u
        table = random_table(rng, bps_in, bps_out)
        for payload_out in payloads_out(lined, bps_out, chunk_out)[1:]:
            nb = nbytes_out(hi, 0, bps_out, shape_out, payload_out)
            whole, view, before = run(dbuf, nframes, payload_in, bps_in, shape_in, bps_out, shape_out, payload_out,
                                      table, 0, nb, src0=src0, src_stride=stride, row_hi=hi)
            judge(whole, view, req.expect(before, table, bps_out, shape_out, payload_out, 0, 0, hi),
                  (payload_in, payload_out))


@pytest.mark.parametrize('bps_in,bps_out', PAIRS)
def test_row_ranges_with_a_first_row(bps_in, bps_out):
    """Ranges that begin and end inside frames, in one frame, without the first and last
    frames and empty, placed anywhere in the output; on byte boundaries of both sides."""
    from baseband_amd import kernels
    torch = _torch()
    rng = np.random.default_rng(300 * bps_in + bps_out)
    nframes = 7
    for shape_in, shape_out in (((8, 1), (1, 8)), ((1, 8), (8, 1)), ((4, 2), (2, 4))):
        (nslot_in, chunk_in), (nslot_out, chunk_out) = shape_in, shape_out
        payload_in, lined = lined_up(260, bps_in, chunk_in, bps_out, chunk_out)
        buf, src = indexed_case(rng, payload_in, nframes, nslot_in)
        dbuf, dsrc = device(buf), device(src)
        req = Request(buf, src, nframes, payload_in, bps_in, nslot_in, chunk_in)
        u = byte_unit(bps_in, chunk_in, bps_out, chunk_out)
        R, total = req.R_in, req.total // u * u
        ranges = [(3 * u, total - 5 * u), (u, 2 * u), (R // u * u + u, R // u * u + 2 * u),
                  (2 * R // u * u, 3 * R // u * u - u), (R // u * u, total - R // u * u), (total - u, total)]
        table = random_table(rng, bps_in, bps_out)
        for k, (lo, hi) in enumerate(ranges):
            assert 0 <= lo < hi <= total
            for payload_out in payloads_out(lined, bps_out, chunk_out)[1:3]:
                R_out = payload_out * 8 // bps_out // chunk_out
                for first_row in (0, 5 * u, R_out // u * u - u, 3 * (R_out // u * u) + u):
                    n = nbytes_out(hi - lo, first_row, bps_out, shape_out, payload_out) + (k & 1) * nslot_out * payload_out
                    whole, view, before = run(dbuf, nframes, payload_in, bps_in, shape_in, bps_out, shape_out, payload_out,
                                              table, 1, n, src=dsrc, row_lo=lo, row_hi=hi, first_row=first_row)
                    want = req.expect(before, table, bps_out, shape_out, payload_out, 1, lo, hi, first_row)
                    judge(whole, view, want, (shape_in, lo, hi, payload_out, first_row))
        # an empty range and a request of no frames write nothing
        payload_out = payloads_out(lined, bps_out, chunk_out)[0]
        for lo, nf in ((0, nframes), (9 * u, nframes), (total, nframes), (0, 0)):
            whole, view, before = run(dbuf, nf, payload_in, bps_in, shape_in, bps_out, shape_out, payload_out, table, 0,
                                      nslot_out * payload_out, src=dsrc, row_lo=lo, row_hi=lo)
            judge(whole, view, before, ('empty', lo, nf))
        # without `out`: whole output frames, as many as the rows need
        got = kernels.recode_frames(dbuf, nframes, payload_in, bps_in, chunk_in, nslot_in, bps_out, chunk_out, nslot_out,
                                    payload_out, table, src=dsrc, row_lo=u, row_hi=total, first_row=u)
        assert got.dtype == torch.uint8 and got.numel() == nbytes_out(total - u, u, bps_out, shape_out, payload_out)


SPLITS = [(8, 2, (8, 1), (1, 8), 1000, 1032), (2, 8, (1, 8), (8, 1), 1000, 520), (4, 2, (4, 2), (2, 4), 4096, 5000),
          (1, 8, (2, 4), (8, 1), 104, 64), (8, 1, (32, 1), (1, 32), 1000, 104), (2, 2, (1, 32), (32, 1), 1024, 520),
          (8, 4, (16, 1), (1, 16), 4096, 5000)]


@pytest.mark.parametrize('bps_in,bps_out,shape_in,shape_out,payload_in,payload_out', SPLITS)
def test_a_request_split_over_two_calls(bps_in, bps_out, shape_in, shape_out, payload_in, payload_out):
    """Frames [0, k) and [k, n) into one output buffer with the matching first_row: the
    output frame that straddles the cut is completed by the second call, which must not
    disturb a byte of the first call's."""
    from baseband_amd import kernels
    torch = _torch()
    rng = np.random.default_rng(400 * bps_in + bps_out)
    (nslot_in, chunk_in), (nslot_out, chunk_out) = shape_in, shape_out
    payload_in, payload_out = whole_rows(payload_in, bps_in, chunk_in), whole_rows(payload_out, bps_out, chunk_out)
    nframes = 11
    buf, src = indexed_case(rng, payload_in, nframes, nslot_in)
    dbuf, dsrc = device(buf), device(src)
    req = Request(buf, src, nframes, payload_in, bps_in, nslot_in, chunk_in)
    u = byte_unit(bps_in, chunk_in, bps_out, chunk_out)
    R = req.R_in
    assert R % u == 0
    table = random_table(rng, bps_in, bps_out)
    lo, hi = 3 * u, req.total - 2 * u
    for first_row in (0, 2 * u):
        n = nbytes_out(hi - lo, first_row, bps_out, shape_out, payload_out)
        for k in (1, 4, 10):
            whole, view, before = run(dbuf, k, payload_in, bps_in, shape_in, bps_out, shape_out, payload_out, table, 1, n,
                                      src=dsrc[:k * nslot_in], row_lo=lo, row_hi=k * R, first_row=first_row)
            half = req.expect(before, table, bps_out, shape_out, payload_out, 1, lo, k * R, first_row)
            judge(whole, view, half, ('first call', k, first_row))
            kernels.recode_frames(dbuf, nframes - k, payload_in, bps_in, chunk_in, nslot_in, bps_out, chunk_out, nslot_out,
                                  payload_out, table, fill_code=1, src=dsrc[k * nslot_in:].contiguous(), row_lo=0,
                                  row_hi=hi - k * R, first_row=first_row + k * R - lo, out=view.view(torch.uint8))
            want = req.expect(before, table, bps_out, shape_out, payload_out, 1, lo, hi, first_row)
            judge(whole, view, want, ('both calls', k, first_row))


@pytest.mark.parametrize('bps_in,bps_out,shape_in,shape_out,payload_in,payload_out',
                         [(8, 2, (8, 1), (1, 8), 64, 40), (2, 8, (1, 8), (8, 1), 40, 12), (4, 1, (4, 2), (2, 4), 104, 32),
                          (8, 8, (2, 4), (8, 1), 40, 12)])
def test_more_work_items_than_the_launch_has_waves(bps_in, bps_out, shape_in, shape_out, payload_in, payload_out):
    """Small payloads and many frames: an output frame is a work item, so there are hundreds
    of them -- on the default grid one per wave with a last workgroup that is not full, and
    on a grid of 3 workgroups (BB_TUNE_BLOCKS) twelve waves that walk many items each."""
    from baseband_amd import _lib, kernels
    rng = np.random.default_rng(500 * bps_in + bps_out)
    (nslot_in, chunk_in), (nslot_out, chunk_out) = shape_in, shape_out
    payload_in, payload_out = whole_rows(payload_in, bps_in, chunk_in), whole_rows(payload_out, bps_out, chunk_out)
    nframes = 403
    n = nframes * nslot_in
    buf = rng.integers(0, 256, n * payload_in, dtype=np.uint8)
    dbuf = device(buf)
    req = Request(buf, np.arange(n) * payload_in, nframes, payload_in, bps_in, nslot_in, chunk_in)
    table = random_table(rng, bps_in, bps_out)
    u = byte_unit(bps_in, chunk_in, bps_out, chunk_out)
    lo, hi = u, req.total // u * u - 3 * u
    nb = nbytes_out(hi - lo, 0, bps_out, shape_out, payload_out)
    assert nb // (nslot_out * payload_out) > 200                # output frames, a work item each: far more than 12 waves
    want = None
    try:
        for blocks in (0, 3):
            kernels.tune(_lib.TUNE_BLOCKS, blocks)
            whole, view, before = run(dbuf, nframes, payload_in, bps_in, shape_in, bps_out, shape_out, payload_out, table,
                                      0, nb, src0=0, src_stride=payload_in, row_lo=lo, row_hi=hi)
            if want is None:
                want = req.expect(before, table, bps_out, shape_out, payload_out, 0, lo, hi)
            judge(whole, view, want, ('blocks', blocks))
    finally:
        kernels.tune(_lib.TUNE_BLOCKS, 0)


@pytest.mark.parametrize('bps_in,bps_out', PAIRS)
def test_equal_thread_structures_give_the_bytes_of_requant_frames(bps_in, bps_out):
    from baseband_amd import kernels
    torch = _torch()
    rng = np.random.default_rng(600 * bps_in + bps_out)
    nframes = 9
    for nslot, chunk in ((1, 1), (8, 1), (2, 2), (1, 8)):
        payload_in, lined = lined_up(1000, bps_in, chunk, bps_out, chunk)
        buf, src = indexed_case(rng, payload_in, nframes, nslot)
        dbuf, dsrc = device(buf), device(src)
        u = byte_unit(bps_in, chunk, bps_out, chunk)
        total = nframes * (payload_in * 8 // bps_in // chunk)
        table = random_table(rng, bps_in, bps_out)
        for payload_out in (whole_rows(520, bps_out, chunk), lined):
            kw = dict(fill_code=1, src=dsrc, row_lo=2 * u, row_hi=total - u, first_row=3 * u)
            zeros = torch.zeros(nbytes_out(total, 0, bps_out, (nslot, chunk), payload_out), dtype=torch.uint8, device='cuda')
            want = kernels.requant_frames(dbuf, nframes, payload_in, bps_in, chunk, nslot, bps_out, payload_out, table,
                                          out=zeros, **kw)
            got = kernels.recode_frames(dbuf, nframes, payload_in, bps_in, chunk, nslot, bps_out, chunk, nslot,
                                        payload_out, table, out=torch.zeros_like(want), **kw)
            assert torch.equal(got, want), (nslot, chunk, payload_out)


@pytest.mark.parametrize('bps', (1, 2))
@pytest.mark.parametrize('coders', ((0, 1), (1, 0), (0, 0)))
def test_equal_widths_give_the_bytes_of_repack_frames(bps, coders):
    """The table of a VDIF <-> Mark 5B pair at scale 1 is repack's code map."""
    from baseband_amd import kernels
    torch = _torch()
    rng = np.random.default_rng(700 + bps)
    coder_in, coder_out = coders
    table = kernels.requant_table(coder_in, bps, coder_out, bps)
    nframes = 9
    for shape_in, shape_out in THREAD_SHAPES[:4] + THREAD_SHAPES[6:]:
        (nslot_in, chunk_in), (nslot_out, chunk_out) = shape_in, shape_out
        payload_in, lined = lined_up(1000, bps, chunk_in, bps, chunk_out)
        buf, src = indexed_case(rng, payload_in, nframes, nslot_in)
        dbuf, dsrc = device(buf), device(src)
        u = byte_unit(bps, chunk_in, bps, chunk_out)
        total = nframes * (payload_in * 8 // bps // chunk_in)
        for payload_out in (whole_rows(520, bps, chunk_out), lined):
            kw = dict(fill_code=1, src=dsrc, row_lo=2 * u, row_hi=total - u, first_row=3 * u)
            zeros = torch.zeros(nbytes_out(total, 0, bps, shape_out, payload_out), dtype=torch.uint8, device='cuda')
            want = kernels.repack_frames(dbuf, nframes, payload_in, bps, coder_in, chunk_in, nslot_in, coder_out, chunk_out,
                                         nslot_out, payload_out, out=zeros, **kw)
            got = kernels.recode_frames(dbuf, nframes, payload_in, bps, chunk_in, nslot_in, bps, chunk_out, nslot_out,
                                        payload_out, table, out=torch.zeros_like(want), **kw)
            assert torch.equal(got, want), (shape_in, shape_out, payload_out)


def test_argument_errors_leave_the_output_untouched():
    from baseband_amd import _lib
    torch = _torch()
    C = ctypes
    rng = np.random.default_rng(7)
    nframes, payload_in, payload_out, bps_in, bps_out = 5, 1000, 520, 8, 2
    shape_in, shape_out = (8, 1), (4, 2)                        # rows of 8 bits in, of 4 bits out: two rows to a byte
    n = nframes * shape_in[0]
    buf = rng.integers(0, 256, n * payload_in, dtype=np.uint8)
    dbuf = device(buf)
    dsrc = device(np.arange(n, dtype=np.int64) * payload_in)
    total = nframes * payload_in                                # rows: one byte of every input slot each
    nb = nbytes_out(total, 0, bps_out, shape_out, payload_out)
    whole, view = guardkit.poisoned(nb // 4, torch.int32)
    table = random_table(rng, bps_in, bps_out)
    ok = dict(bps_in=bps_in, bps_out=bps_out, chunk_in=1, nslot_in=8, chunk_out=2, nslot_out=4, payload_in=payload_in,
              payload_out=payload_out, table=table, fill_code=1, src0=0, src_stride=payload_in, row_lo=0, row_hi=total,
              first_row=0)

    def call(buf_ptr=dbuf.data_ptr(), buf_n=dbuf.numel(), src_ptr=dsrc.data_ptr(), nfr=nframes,
             out_ptr=view.data_ptr(), out_n=nb, **kw):
        p = _lib.recode_params(**dict(ok, **kw))
        return _lib.lib.bb_recode_frames(buf_ptr, buf_n, src_ptr, nfr, C.byref(p), out_ptr, out_n, None)

    bad_table = table.copy()
    bad_table[200] = 4
    E, R, N = _lib.BB_EINVAL, _lib.BB_ERANGE, _lib.BB_ENOTSUP
    R_out = payload_out * 8 // bps_out // 2
    last = total - 1                                            # the last output row, and the byte behind it
    end = (last // R_out * 4 + 3) * payload_out + ((last % R_out + 1) * 4 + 7) // 8
    assert end < nb
    refusals = [
        (E, dict(buf_ptr=None)), (E, dict(out_ptr=None)), (E, dict(buf_ptr=dbuf.data_ptr() + 2)),
        (E, dict(out_ptr=view.data_ptr() + 4)),                                            # a misaligned out
        (E, dict(reserved=1)), (E, dict(payload_in=1002)), (E, dict(payload_out=522)), (E, dict(payload_out=0)),
        (E, dict(row_lo=12, row_hi=8)), (E, dict(fill_code=4)), (E, dict(fill_code=-1)), (E, dict(table=bad_table)),
        (E, dict(nslot_out=8)),                                                            # 8 components against 16
        (E, dict(src_ptr=None, src0=2)), (E, dict(src_ptr=None, src_stride=-1000)),
        (R, dict(row_hi=total + 4)), (R, dict(out_n=end - 1)), (R, dict(out_n=16)),                # an output too small
        (R, dict(first_row=R_out)),
        (R, dict(src_ptr=None, src_stride=payload_in + 4)), (R, dict(src_ptr=None, src0=4)),
        (N, dict(row_lo=1)), (N, dict(row_hi=total - 1)), (N, dict(first_row=1, row_hi=total - 2)),   # whole bytes only
        (N, dict(row_lo=3, row_hi=total - 1)),
        (N, dict(bps_in=3)), (N, dict(bps_out=3)), (N, dict(nslot_in=3)), (N, dict(chunk_out=3)),
        (N, dict(nslot_in=64, chunk_out=16)),
    ]
    for rc, kw in refusals:
        assert call(**kw) == rc, kw
    torch.cuda.synchronize()
    v = guardkit.verdict(whole, view, guardkit.poison_words(nb // 4))
    assert not v.touched and v.wrong == 0 and v.poison_left == nb // 4, guardkit.describe(v, nb // 4)
    # the same block goes through, with an index and at the fixed stride
    req = Request(buf, np.arange(n) * payload_in, nframes, payload_in, bps_in, *shape_in)
    before = view.cpu().numpy().view(np.uint8).copy()
    want = req.expect(before, table, bps_out, shape_out, payload_out, 1)
    assert call(out_n=end) == _lib.BB_OK                        # (the last row's byte is the last one needed)
    judge(whole, view, want, 'index')
    guardkit.refill(whole)
    assert call(src_ptr=None) == _lib.BB_OK
    judge(whole, view, want, 'fixed stride')
