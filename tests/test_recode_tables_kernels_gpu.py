"""bb_recode_frames_tables on the device against NumPy on the bytes alone: recodekit's rows of
a request, component k of a row sent through ITS table -- ``tables[k][code]`` -- where the
payload is valid and set to fill_code elsewhere, split into the output slots and packed:
exact byte equality.  All 16 pairs of widths at every thread shape (equal structures among
them) with random tables that differ per component, through a shuffled index with missing
entries and at a fixed stride off the 16-byte grid, frames that do not line up, row ranges, a
request split over two launches, more work items than waves, tables that are the constant
``k % (1 << bps_out)`` (a wrong component index shows at once), equal rows against
bb_recode_frames, and table bytes beyond bps_out bits in a device tensor, which the kernel
masks.  Outputs are poisoned and guarded."""
import numpy as np
import pytest

import guardkit
from packedkit import _torch, device, whole_rows, indexed_case, judge, unpack_codes, pack_codes
from recodekit import (PAIRS, THREAD_SHAPES, PAYLOADS, fits, byte_unit, lined_up, payloads_out, random_table, Request,
                       nbytes_out)

pytestmark = pytest.mark.gpu

CASES = [(bi, bo, si, so) for bi, bo in PAIRS for si, so in THREAD_SHAPES if fits(bi, bo, si[0] * si[1])]


def random_tables(rng, bps_in, bps_out, ncomp):
    """A table per component, no two alike where the widths leave room for that."""
    t = rng.integers(0, 1 << bps_out, (ncomp, 1 << bps_in), dtype=np.uint8)
    if (1 << bps_out) ** (1 << bps_in) >= 4 * ncomp:
        while len({r.tobytes() for r in t}) < ncomp:
            t = rng.integers(0, 1 << bps_out, (ncomp, 1 << bps_in), dtype=np.uint8)
    return t


def expect(req, before, tables, bps_out, shape_out, payload_out, fill_code, row_lo=0, row_hi=None, first_row=0):
    """`Request.expect` with ``tables[k][code]`` for component k in place of ``table[code]``."""
    nslot, chunk = shape_out
    assert nslot * chunk == req.ncomp and tables.shape == (req.ncomp, 1 << req.bps_in)
    row_hi = req.total if row_hi is None else row_hi
    nout = len(before) // (nslot * payload_out)
    assert nout * nslot * payload_out == len(before)
    R_out = payload_out * 8 // bps_out // chunk
    out = unpack_codes(before, bps_out).reshape(nout, nslot, R_out, chunk).transpose(0, 2, 1, 3)
    out = out.reshape(nout * R_out, req.ncomp).copy()
    k = slice(row_lo, row_hi)
    assert first_row + row_hi - row_lo <= len(out)
    out[first_row:first_row + row_hi - row_lo] = np.where(
        req.valid[k], tables[np.arange(req.ncomp), req.rows[k]], np.uint8(fill_code))
    return pack_codes(out.reshape(nout, R_out, nslot, chunk).transpose(0, 2, 1, 3), bps_out)


def run(dbuf, nframes, payload_in, bps_in, shape_in, bps_out, shape_out, payload_out, tables, fill_code, nout_bytes, **kw):
    """One launch into a poisoned, guarded output -> (whole, view, bytes before the launch)."""
    from baseband_amd import kernels
    torch = _torch()
    whole, view = guardkit.poisoned(nout_bytes // 4, torch.int32)
    before = view.cpu().numpy().view(np.uint8).copy()
    out = view.view(torch.uint8)
    got = kernels.recode_frames_tables(dbuf, nframes, payload_in, bps_in, shape_in[1], shape_in[0], bps_out, shape_out[1],
                                       shape_out[0], payload_out, tables, fill_code=fill_code, out=out, **kw)
    assert got is out
    return whole, view, before


def test_the_cases_are_all_width_pairs_at_all_thread_shapes():
    assert {(bi, bo) for bi, bo, _, _ in CASES} == set(PAIRS)
    assert {(si, so) for _, _, si, so in CASES} == set(THREAD_SHAPES)
    assert any(si == so for _, _, si, so in CASES)              # equal structures are a geometry of this kernel


@pytest.mark.parametrize('bps_in,bps_out,shape_in,shape_out', CASES)
def test_tables_through_an_index(bps_in, bps_out, shape_in, shape_out):
    rng = np.random.default_rng([11, bps_in, bps_out, *shape_in, *shape_out])
    (nslot_in, chunk_in), (nslot_out, chunk_out) = shape_in, shape_out
    ncomp = nslot_in * chunk_in
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
            tables = random_tables(rng, bps_in, bps_out, ncomp)
            fill = int(rng.integers(0, 1 << bps_out))
            n = nbytes_out(hi, 0, bps_out, shape_out, payload_out)
            whole, view, before = run(dbuf, nframes, payload_in, bps_in, shape_in, bps_out, shape_out, payload_out,
                                      tables, fill, n, src=dsrc, row_hi=hi)
            want = expect(req, before, tables, bps_out, shape_out, payload_out, fill, 0, hi)
            judge(whole, view, want, (payload_in, nframes, payload_out))


@pytest.mark.parametrize('bps_in,bps_out,shape_in,shape_out', CASES)
def test_tables_at_a_fixed_stride(bps_in, bps_out, shape_in, shape_out):
    rng = np.random.default_rng([12, bps_in, bps_out, *shape_in, *shape_out])
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
        tables = device(random_tables(rng, bps_in, bps_out, nslot_in * chunk_in))     # (a device tensor, used for every launch)
        for payload_out in payloads_out(lined, bps_out, chunk_out)[1:]:
            nb = nbytes_out(hi, 0, bps_out, shape_out, payload_out)
            whole, view, before = run(dbuf, nframes, payload_in, bps_in, shape_in, bps_out, shape_out, payload_out,
                                      tables, 0, nb, src0=src0, src_stride=stride, row_hi=hi)
            judge(whole, view, expect(req, before, tables.cpu().numpy(), bps_out, shape_out, payload_out, 0, 0, hi),
                  (payload_in, payload_out))


@pytest.mark.parametrize('bps_in,bps_out', PAIRS)
def test_row_ranges_with_a_first_row(bps_in, bps_out):
    """Ranges that begin and end inside frames, in one frame, without the first and last
    frames and empty, placed anywhere in the output; on byte boundaries of both sides."""
    rng = np.random.default_rng(1300 * bps_in + bps_out)
    nframes = 7
    for shape_in, shape_out in (((8, 1), (1, 8)), ((1, 8), (8, 1)), ((4, 2), (2, 4)), ((2, 2), (2, 2))):
        (nslot_in, chunk_in), (nslot_out, chunk_out) = shape_in, shape_out
        payload_in, lined = lined_up(260, bps_in, chunk_in, bps_out, chunk_out)
        buf, src = indexed_case(rng, payload_in, nframes, nslot_in)
        dbuf, dsrc = device(buf), device(src)
        req = Request(buf, src, nframes, payload_in, bps_in, nslot_in, chunk_in)
        u = byte_unit(bps_in, chunk_in, bps_out, chunk_out)
        R, total = req.R_in, req.total // u * u
        ranges = [(3 * u, total - 5 * u), (u, 2 * u), (R // u * u + u, R // u * u + 2 * u),
                  (2 * R // u * u, 3 * R // u * u - u), (total - u, total)]
        tables = random_tables(rng, bps_in, bps_out, nslot_in * chunk_in)
        for k, (lo, hi) in enumerate(ranges):
            assert 0 <= lo < hi <= total
            outs = payloads_out(lined, bps_out, chunk_out)[1:3]
            payload_out = outs[k % len(outs)]
            R_out = payload_out * 8 // bps_out // chunk_out
            for first_row in (0, R_out // u * u - u, 3 * (R_out // u * u) + u):
                n = nbytes_out(hi - lo, first_row, bps_out, shape_out, payload_out) + (k & 1) * nslot_out * payload_out
                whole, view, before = run(dbuf, nframes, payload_in, bps_in, shape_in, bps_out, shape_out, payload_out,
                                          tables, 1, n, src=dsrc, row_lo=lo, row_hi=hi, first_row=first_row)
                want = expect(req, before, tables, bps_out, shape_out, payload_out, 1, lo, hi, first_row)
                judge(whole, view, want, (shape_in, lo, hi, payload_out, first_row))
        # an empty range and a request of no frames write nothing
        payload_out = payloads_out(lined, bps_out, chunk_out)[0]
        for lo, nf in ((0, nframes), (9 * u, nframes), (total, nframes), (0, 0)):
            whole, view, before = run(dbuf, nf, payload_in, bps_in, shape_in, bps_out, shape_out, payload_out, tables, 0,
                                      nslot_out * payload_out, src=dsrc, row_lo=lo, row_hi=lo)
            judge(whole, view, before, ('empty', lo, nf))


SPLITS = [(8, 2, (8, 1), (1, 8), 1000, 1032), (2, 8, (1, 8), (8, 1), 1000, 520), (4, 2, (4, 2), (2, 4), 4096, 5000),
          (8, 1, (32, 1), (1, 32), 1000, 104), (8, 4, (8, 1), (8, 1), 4096, 5000)]


@pytest.mark.parametrize('bps_in,bps_out,shape_in,shape_out,payload_in,payload_out', SPLITS)
def test_a_request_split_over_two_calls(bps_in, bps_out, shape_in, shape_out, payload_in, payload_out):
    """Frames [0, k) and [k, n) into one output buffer with the matching first_row: the
    output frame that straddles the cut is completed by the second call, which must not
    disturb a byte of the first call's."""
    from baseband_amd import kernels
    torch = _torch()
    rng = np.random.default_rng(1400 * bps_in + bps_out)
    (nslot_in, chunk_in), (nslot_out, chunk_out) = shape_in, shape_out
    payload_in, payload_out = whole_rows(payload_in, bps_in, chunk_in), whole_rows(payload_out, bps_out, chunk_out)
    nframes = 11
    buf, src = indexed_case(rng, payload_in, nframes, nslot_in)
    dbuf, dsrc = device(buf), device(src)
    req = Request(buf, src, nframes, payload_in, bps_in, nslot_in, chunk_in)
    u = byte_unit(bps_in, chunk_in, bps_out, chunk_out)
    R = req.R_in
    assert R % u == 0
    tables = random_tables(rng, bps_in, bps_out, nslot_in * chunk_in)
    lo, hi = 3 * u, req.total - 2 * u
    for first_row in (0, 2 * u):
        n = nbytes_out(hi - lo, first_row, bps_out, shape_out, payload_out)
        for k in (1, 4, 10):
            whole, view, before = run(dbuf, k, payload_in, bps_in, shape_in, bps_out, shape_out, payload_out, tables, 1, n,
                                      src=dsrc[:k * nslot_in], row_lo=lo, row_hi=k * R, first_row=first_row)
            half = expect(req, before, tables, bps_out, shape_out, payload_out, 1, lo, k * R, first_row)
            judge(whole, view, half, ('first call', k, first_row))
            kernels.recode_frames_tables(dbuf, nframes - k, payload_in, bps_in, chunk_in, nslot_in, bps_out, chunk_out,
                                         nslot_out, payload_out, tables, fill_code=1, src=dsrc[k * nslot_in:].contiguous(),
                                         row_lo=0, row_hi=hi - k * R, first_row=first_row + k * R - lo,
                                         out=view.view(torch.uint8))
            want = expect(req, before, tables, bps_out, shape_out, payload_out, 1, lo, hi, first_row)
            judge(whole, view, want, ('both calls', k, first_row))


@pytest.mark.parametrize('bps_in,bps_out,shape_in,shape_out,payload_in,payload_out',
                         [(8, 2, (8, 1), (1, 8), 64, 40), (2, 8, (1, 8), (8, 1), 40, 12), (4, 1, (4, 2), (2, 4), 104, 32),
                          (8, 8, (2, 4), (8, 1), 40, 12), (8, 2, (8, 1), (8, 1), 64, 16)])
def test_more_work_items_than_the_launch_has_waves(bps_in, bps_out, shape_in, shape_out, payload_in, payload_out):
    """Small payloads and many frames: an output frame is a work item, so there are hundreds
    of them -- on the default grid one per wave with a last workgroup that is not full, and
    on a grid of 3 workgroups (BB_TUNE_BLOCKS) twelve waves that walk many items each, every
    workgroup with its own copy of the tables."""
    from baseband_amd import _lib, kernels
    rng = np.random.default_rng(1500 * bps_in + bps_out)
    (nslot_in, chunk_in), (nslot_out, chunk_out) = shape_in, shape_out
    payload_in, payload_out = whole_rows(payload_in, bps_in, chunk_in), whole_rows(payload_out, bps_out, chunk_out)
    nframes = 403
    n = nframes * nslot_in
    buf = rng.integers(0, 256, n * payload_in, dtype=np.uint8)
    dbuf = device(buf)
    req = Request(buf, np.arange(n) * payload_in, nframes, payload_in, bps_in, nslot_in, chunk_in)
    tables = random_tables(rng, bps_in, bps_out, nslot_in * chunk_in)
    u = byte_unit(bps_in, chunk_in, bps_out, chunk_out)
    lo, hi = u, req.total // u * u - 3 * u
    nb = nbytes_out(hi - lo, 0, bps_out, shape_out, payload_out)
    assert nb // (nslot_out * payload_out) > 200                # output frames, a work item each: far more than 12 waves
    want = None
    try:
        for blocks in (0, 3):
            kernels.tune(_lib.TUNE_BLOCKS, blocks)
            whole, view, before = run(dbuf, nframes, payload_in, bps_in, shape_in, bps_out, shape_out, payload_out, tables,
                                      0, nb, src0=0, src_stride=payload_in, row_lo=lo, row_hi=hi)
            if want is None:
                want = expect(req, before, tables, bps_out, shape_out, payload_out, 0, lo, hi)
            judge(whole, view, want, ('blocks', blocks))
    finally:
        kernels.tune(_lib.TUNE_BLOCKS, 0)


@pytest.mark.parametrize('bps_in,bps_out,shape_in,shape_out', CASES)
def test_constant_tables_name_the_component(bps_in, bps_out, shape_in, shape_out):
    """Table k is the constant ``k % (1 << bps_out)``: every valid field of the output holds its
    own component's number, whatever the input's codes."""
    rng = np.random.default_rng([16, bps_in, bps_out, *shape_in, *shape_out])
    (nslot_in, chunk_in), (nslot_out, chunk_out) = shape_in, shape_out
    ncomp = nslot_in * chunk_in
    payload_in, payload_out = lined_up(104, bps_in, chunk_in, bps_out, chunk_out)
    nframes = 9
    buf, src = indexed_case(rng, payload_in, nframes, nslot_in)
    req = Request(buf, src, nframes, payload_in, bps_in, nslot_in, chunk_in)
    u = byte_unit(bps_in, chunk_in, bps_out, chunk_out)
    hi = req.total // u * u
    tables = np.repeat((np.arange(ncomp) % (1 << bps_out)).astype(np.uint8)[:, None], 1 << bps_in, 1)
    fill = (1 << bps_out) - 1
    n = nbytes_out(hi, 0, bps_out, shape_out, payload_out)
    whole, view, before = run(device(buf), nframes, payload_in, bps_in, shape_in, bps_out, shape_out, payload_out,
                              tables, fill, n, src=device(src), row_hi=hi)
    judge(whole, view, expect(req, before, tables, bps_out, shape_out, payload_out, fill, 0, hi), (shape_in, shape_out))
    # ... read back by output slot and field: component t * chunk_out + q, or the fill code
    got = unpack_codes(view.cpu().numpy().view(np.uint8), bps_out).reshape(-1, nslot_out, payload_out * 8 // bps_out // chunk_out,
                                                                         chunk_out)
    rows = got.transpose(0, 2, 1, 3).reshape(-1, ncomp)[:hi]
    names = np.arange(ncomp) % (1 << bps_out)
    assert ((rows == names) | ((rows == fill) & ~req.valid[:hi])).all()


@pytest.mark.parametrize('bps_in,bps_out', PAIRS)
def test_equal_rows_give_the_bytes_of_recode_frames(bps_in, bps_out):
    from baseband_amd import kernels
    torch = _torch()
    rng = np.random.default_rng(1700 * bps_in + bps_out)
    nframes = 9
    for shape_in, shape_out in THREAD_SHAPES[:4] + THREAD_SHAPES[6:]:
        (nslot_in, chunk_in), (nslot_out, chunk_out) = shape_in, shape_out
        payload_in, lined = lined_up(1000, bps_in, chunk_in, bps_out, chunk_out)
        buf, src = indexed_case(rng, payload_in, nframes, nslot_in)
        dbuf, dsrc = device(buf), device(src)
        u = byte_unit(bps_in, chunk_in, bps_out, chunk_out)
        total = nframes * (payload_in * 8 // bps_in // chunk_in)
        table = random_table(rng, bps_in, bps_out)
        tables = np.repeat(table[None, :], nslot_in * chunk_in, 0)
        for payload_out in (whole_rows(520, bps_out, chunk_out), lined):
            kw = dict(fill_code=1, src=dsrc, row_lo=2 * u, row_hi=total - u, first_row=3 * u)
            zeros = torch.zeros(nbytes_out(total, 0, bps_out, shape_out, payload_out), dtype=torch.uint8, device='cuda')
            want = kernels.recode_frames(dbuf, nframes, payload_in, bps_in, chunk_in, nslot_in, bps_out, chunk_out, nslot_out,
                                         payload_out, table, out=zeros, **kw)
            got = kernels.recode_frames_tables(dbuf, nframes, payload_in, bps_in, chunk_in, nslot_in, bps_out, chunk_out,
                                               nslot_out, payload_out, tables, out=torch.zeros_like(want), **kw)
            assert torch.equal(got, want), (shape_in, shape_out, payload_out)


@pytest.mark.parametrize('bps_in,bps_out', [(bi, bo) for bi, bo in PAIRS if bo < 8])
def test_table_bytes_beyond_bps_out_are_masked(bps_in, bps_out):
    """A device tensor's values are not the host's to check: the kernel keeps the low bps_out
    bits of every table byte, so the neighbouring fields are those of the masked tables."""
    from baseband_amd import kernels
    rng = np.random.default_rng(1800 * bps_in + bps_out)
    for shape_in, shape_out in (((8, 1), (1, 8)), ((1, 8), (8, 1)), ((2, 2), (2, 2)), ((1, 1), (1, 1))):
        (nslot_in, chunk_in), (nslot_out, chunk_out) = shape_in, shape_out
        ncomp = nslot_in * chunk_in
        payload_in, payload_out = lined_up(104, bps_in, chunk_in, bps_out, chunk_out)
        nframes = 6
        buf, src = indexed_case(rng, payload_in, nframes, nslot_in)
        req = Request(buf, src, nframes, payload_in, bps_in, nslot_in, chunk_in)
        u = byte_unit(bps_in, chunk_in, bps_out, chunk_out)
        hi = req.total // u * u
        wild = rng.integers(0, 256, (ncomp, 1 << bps_in), dtype=np.uint8)
        wild[:, 0] |= 0xf0 | (1 << bps_out)
        assert (wild >= 1 << bps_out).any()
        n = nbytes_out(hi, 0, bps_out, shape_out, payload_out)
        whole, view, before = run(device(buf), nframes, payload_in, bps_in, shape_in, bps_out, shape_out, payload_out,
                                  device(wild), 0, n, src=device(src), row_hi=hi)
        want = expect(req, before, wild & np.uint8((1 << bps_out) - 1), bps_out, shape_out, payload_out, 0, 0, hi)
        judge(whole, view, want, (shape_in, shape_out))
        # the same values in a NumPy array are the host's to refuse
        with pytest.raises(ValueError, match='not a code of {} bits'.format(bps_out)):
            kernels.recode_frames_tables(device(buf), nframes, payload_in, bps_in, chunk_in, nslot_in, bps_out, chunk_out,
                                         nslot_out, payload_out, wild, src=device(src), row_hi=hi)


def test_tables_of_another_shape_or_type_are_refused():
    from baseband_amd import kernels
    torch = _torch()
    dbuf = torch.zeros(8 * 40, dtype=torch.uint8, device='cuda')
    args = (dbuf, 1, 40, 8, 1, 8, 2, 8, 1, 80)
    for bad in (np.zeros((4, 256), np.uint8), np.zeros((8, 4), np.uint8), np.zeros((8, 256), np.int32),
                torch.zeros((8, 256), dtype=torch.uint8), torch.zeros((8, 256), dtype=torch.int32, device='cuda'),
                torch.zeros((256, 8), dtype=torch.uint8, device='cuda').t(), [[0] * 256] * 8):
        with pytest.raises(ValueError, match='tables must be'):
            kernels.recode_frames_tables(*args, bad, src0=0, src_stride=40)
