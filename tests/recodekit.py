"""What the bb_recode_frames test modules share: the thread shapes, the payloads that line
up and those that do not, and the NumPy oracle on the bytes alone.  A plain helper module,
imported by name, beside packedkit and guardkit."""
import numpy as np

import guardkit
from packedkit import _torch, unpack_codes, pack_codes, whole_rows

WIDTHS = (1, 2, 4, 8)
PAIRS = [(bi, bo) for bi in WIDTHS for bo in WIDTHS]
# ((nslot_in, chunk_in), (nslot_out, chunk_out))
THREAD_SHAPES = [((8, 1), (1, 8)), ((1, 8), (8, 1)), ((4, 2), (2, 4)), ((2, 4), (8, 1)),
                 ((32, 1), (1, 32)), ((1, 32), (32, 1)), ((2, 2), (2, 2)), ((1, 1), (1, 1))]
PAYLOADS = ((40, 37), (104, 19), (8000, 5))                     # (bytes, frames); rounded up to whole rows


def fits(bps_in, bps_out, ncomp):
    return ncomp * max(bps_in, bps_out) <= 256


def byte_unit(bps_in, chunk_in, bps_out, chunk_out):
    """Rows between byte boundaries common to every input and every output slot stream."""
    return max(1, 8 // min(chunk_in * bps_in, chunk_out * bps_out))


def lined_up(nbytes, bps_in, chunk_in, bps_out, chunk_out):
    """-> (payload_in, payload_out) of the same number of rows, both whole dwords, payload_in >= nbytes."""
    unit = max(1, 32 // min(chunk_in * bps_in, chunk_out * bps_out))
    rows = -(-(nbytes * 8) // (chunk_in * bps_in * unit)) * unit
    return rows * chunk_in * bps_in // 8, rows * chunk_out * bps_out // 8


def payloads_out(payload_lined, bps_out, chunk_out):
    """Output payloads whose frames do not line up with the input's (three), and the one that does."""
    unit = max(4, chunk_out * bps_out // 8)
    return sorted({whole_rows(32, bps_out, chunk_out), whole_rows(payload_lined + unit, bps_out, chunk_out),
                   whole_rows(2 * payload_lined // 3, bps_out, chunk_out), payload_lined})


def random_table(rng, bps_in, bps_out):
    return rng.integers(0, 1 << bps_out, 1 << bps_in, dtype=np.uint8)


class Request:
    """The rows of `ncomp` codes of a request and which of them have a payload (NumPy, from
    the bytes alone): every input slot stream unpacked, rows formed across the slots."""

    def __init__(self, buf, src, nframes, payload_in, bps_in, nslot_in, chunk_in):
        self.bps_in, self.ncomp = bps_in, nslot_in * chunk_in
        self.R_in = R = payload_in * 8 // bps_in // chunk_in
        self.total = nframes * R
        codes = np.zeros((nframes, R, nslot_in, chunk_in), np.uint8)
        valid = np.zeros((nframes, R, nslot_in, chunk_in), bool)
        for f in range(nframes):
            for s in range(nslot_in):
                so = int(src[f * nslot_in + s])
                if so < 0 or so + payload_in > len(buf):
                    continue
                codes[f, :, s] = unpack_codes(buf[so:so + payload_in], bps_in).reshape(R, chunk_in)
                valid[f, :, s] = True
        self.rows = codes.reshape(self.total, self.ncomp)
        self.valid = valid.reshape(self.total, self.ncomp)

    def expect(self, before, table, bps_out, shape_out, payload_out, fill_code, row_lo=0, row_hi=None, first_row=0):
        """`before` (the output buffer's bytes, whole output frames) with the rows of the
        request written into it: the table where the payload is valid, `fill_code`
        elsewhere, split into output slots and packed."""
        nslot, chunk = shape_out
        assert nslot * chunk == self.ncomp
        row_hi = self.total if row_hi is None else row_hi
        nout = len(before) // (nslot * payload_out)
        assert nout * nslot * payload_out == len(before)
        R_out = payload_out * 8 // bps_out // chunk
        out = unpack_codes(before, bps_out).reshape(nout, nslot, R_out, chunk).transpose(0, 2, 1, 3)
        out = out.reshape(nout * R_out, self.ncomp).copy()
        k = slice(row_lo, row_hi)
        assert first_row + row_hi - row_lo <= len(out)
        out[first_row:first_row + row_hi - row_lo] = np.where(
            self.valid[k], np.asarray(table, np.uint8)[self.rows[k]], np.uint8(fill_code))
        return pack_codes(out.reshape(nout, R_out, nslot, chunk).transpose(0, 2, 1, 3), bps_out)


def nbytes_out(nrows, first_row, bps_out, shape_out, payload_out):
    nslot, chunk = shape_out
    R_out = payload_out * 8 // bps_out // chunk
    return -(-(first_row + nrows) // R_out) * nslot * payload_out


def run(dbuf, nframes, payload_in, bps_in, shape_in, bps_out, shape_out, payload_out, table, fill_code, nout_bytes, **kw):
    """One launch into a poisoned, guarded output -> (whole, view, bytes before the launch)."""
    from baseband_amd import kernels
    torch = _torch()
    whole, view = guardkit.poisoned(nout_bytes // 4, torch.int32)
    before = view.cpu().numpy().view(np.uint8).copy()
    out = view.view(torch.uint8)
    got = kernels.recode_frames(dbuf, nframes, payload_in, bps_in, shape_in[1], shape_in[0], bps_out, shape_out[1],
                                shape_out[0], payload_out, table, fill_code=fill_code, out=out, **kw)
    assert got is out
    return whole, view, before
