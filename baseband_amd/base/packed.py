"""Work on a file's packed bytes without decoding them: sampler statistics, frame validity
and packed reads (`convert`), given to `base.GPUStreamReaderBase` by `PackedBytesMixin`.
Readers whose frames are fixed-stride payloads of LSB-first codes (VDIF, Mark 5B) define
`_packed_geometry` and `_packed_index`.
"""
import operator
from collections import namedtuple

import numpy as np
import torch

from .. import _lib, kernels
from ..staging import WindowPipeline

PackedGeometry = namedtuple('PackedGeometry', 'coder bps chunk nslot payload_nbytes')


def samples_per_byte(chunk, bps):
    """Samples in a byte of a thread's stream of `chunk` codes of `bps` bits per sample."""
    return max(1, 8 // (chunk * bps))


def piece_rows(start, stop, spf, s, e):
    """-> (row_lo, row_hi, first_row): the rows of the frame sets [s, e), counted from s, that
    the samples [start, stop) take, and which of those samples the first of them is."""
    lo = max(start, s * spf)
    return lo - s * spf, min(stop, e * spf) - s * spf, lo - start


class _ValidityMarks:
    """Which of `nout` output frames of `samples_per_frame_out` samples, cut from the samples [start, stop) of
    frame sets of `spf` samples and `nslot` slots, draw on a set with an index entry below 0 (a difference array)."""

    def __init__(self, nout, samples_per_frame_out, start, stop, spf, nslot):
        self.geom = (nout, samples_per_frame_out, start, stop, spf, nslot)
        self.marks = None

    def add(self, src, s, e):
        nout, spf_out, start, stop, spf, nslot = self.geom
        if self.marks is None:
            self.marks = torch.zeros(nout + 1, dtype=torch.int32, device=src.device)
        bad = torch.nonzero((src.reshape(e - s, nslot) < 0).any(1)).reshape(-1) + s
        lo = torch.clamp(bad * spf, min=start) - start
        hi = torch.clamp((bad + 1) * spf, max=stop) - 1 - start
        one = torch.ones_like(bad, dtype=torch.int32)
        self.marks.index_add_(0, torch.div(lo, spf_out, rounding_mode='floor'), one)
        self.marks.index_add_(0, torch.div(hi, spf_out, rounding_mode='floor') + 1, -one)

    def valid(self):
        return (torch.cumsum(self.marks, 0)[:self.geom[0]] == 0).cpu().numpy()


class _WalkVerdict:
    """What a walk over packed bytes at the fixed stride learns about its frames
    (`PackedBytesMixin._walk_packed`): a device counter that bb_verify_records adds to,
    and the frames the file's bytes did not reach (known on the host)."""
    __slots__ = ('counter', 'missing')

    def __init__(self):
        self.counter = torch.zeros(1, dtype=torch.int32, device='cuda')
        self.missing = 0

    def nbad(self):
        return self.missing + int(self.counter.item())


class PackedBytesMixin:
    """The methods of a stream reader that work on packed bytes, and their hooks."""

    def _packed_geometry(self):
        """`PackedGeometry` of the packed samples (`chunk`: codes per complete sample of a thread), or None."""
        return None

    def _packed_index(self, dbuf, first, nsets, verdict=None):
        """Payload offsets into `dbuf`, which starts at frame set `first`, for `nsets`
        frame sets (-1: missing or invalid): header scan and index, nothing else."""
        raise NotImplementedError

    def _packed_shape(self, counts):
        return counts

    def _packed_entry(self, what):
        """What a method on the packed bytes begins with -> the geometry."""
        if self.closed:
            raise ValueError("I/O operation on closed stream.")
        geom = self._packed_geometry()
        if geom is None:
            raise NotImplementedError("{} has no {}".format(type(self).__name__, what))
        return geom

    def _packed_count(self, count, rest=False):
        """`count` against what is left from the offset; `rest`: None or below 0 stand for all of it."""
        left = self.shape[0] - self.offset
        if rest and (count is None or count < 0):
            count = max(0, left)
        if count < 0 or count > left:
            raise EOFError("cannot read from beyond end of input.")
        return count

    # -- sampler statistics (kernels.count_states, count_states_bins)
    @property
    def state_levels(self):
        """float32 NumPy array of the ``2**bps`` levels of this stream's coder, by raw
        code: with ``c = fh.state_counts()``, ``(c * levels**2).sum(-1) / c.sum(-1)`` is
        the mean power."""
        geom = self._packed_geometry()
        if geom is None:
            raise NotImplementedError("{} has no sampler statistics".format(type(self).__name__))
        return _lib.get_levels(geom.coder, geom.bps)

    def state_counts(self, count=None):
        """How often each raw sample code occurs among the samples ``read(count)``
        would return from the current offset -> int64 device tensor whose last axis
        counts codes ``0 .. 2**bps - 1`` (levels: `state_levels`).  Counted from the
        packed bytes (bb_count_states): one pass over the file's bytes, nothing is
        decoded and the offset does not move.  Samples of frames that ``read()`` would
        fill (missing or invalid ones) are left out; bad frames do not raise.  Threads
        follow the reader's selection; a channel `subset` is NOT applied: counting
        every channel costs nothing more.

        A file that lost bytes or frames is counted as ``read()`` under ``verify='fix'``
        reads it, whatever has been read before: when the pass meets headers that are
        missing or off the fixed stride, the frames are located byte by byte
        (`_relocate`, as a read would) and the whole request is counted again through
        that index.  A ``verify=True`` reader gives the same counts and stays strict:
        the index is used for the statistics only.  ``verify=False`` counts what stands
        at the fixed stride."""
        g = self._packed_entry('sampler statistics')
        if not kernels.count_states_supported(g.bps, g.chunk, g.nslot, g.payload_nbytes):
            raise NotImplementedError(
                "state_counts: a complete sample of {} codes x {} bits is not one the counting kernel "
                "takes (a power of two of codes, chunk * bps <= {})".format(g.chunk, g.bps, kernels.STATES_MAX_ROW_BITS))

        def answer():
            n = self._packed_count(count, rest=True)
            kernels.require_gpu()
            counts = torch.zeros((g.nslot, g.chunk, 1 << g.bps), dtype=torch.int64, device='cuda')

            def add(dbuf, src, s, e, row_lo, row_hi, first_row):
                kernels.count_states(dbuf, e - s, g.payload_nbytes, g.bps, g.chunk, g.nslot, src=src,
                                     row_lo=row_lo, row_hi=row_hi, counts=counts)

            nbad = self._walk_packed(g.nslot, self.offset, self.offset + n, add) if n else 0
            return self._packed_shape(counts), nbad

        return self._answer_packed(answer)

    def state_series(self, bin_samples, count=None):
        """`state_counts` as a time series: int32 device tensor of shape ``(nbins,) +
        state_counts().shape`` with ``nbins = ceil(count / bin_samples)``; bin ``b`` counts
        the samples ``[offset + b * bin_samples, offset + (b + 1) * bin_samples)`` of what
        ``read(count)`` would return (the last bin may be short).  Counted from the packed
        bytes (bb_count_states_bins): one pass, nothing is decoded, the offset does not
        move.  Samples of missing or invalid frames are left out, so a bin's sum over the
        code axis is its number of valid samples, and ``state_series(n, count).sum(0)``
        equals ``state_counts(count)``.  Bins are whole bytes of a thread's stream:
        `bin_samples`, the offset and `count` must be multiples of ``8 / (codes per sample
        * bps)`` samples where that is more than one.  Damaged files and ``verify=True``
        readers: as `state_counts` -- the frames are located, bad frames do not raise."""
        g = self._packed_entry('sampler statistics')
        bin_samples = operator.index(bin_samples)
        if bin_samples < 1:
            raise ValueError("state_series: bin_samples must be at least 1")
        if bin_samples > 0x7fffffff:
            raise ValueError("state_series: bin_samples must be below 2**31")
        if not kernels.count_states_supported(g.bps, g.chunk, g.nslot, g.payload_nbytes) or \
                g.chunk << g.bps > kernels.STATES_BINS_MAX_COUNTERS:
            raise NotImplementedError(
                "state_series: a complete sample of {} codes x {} bits is not one the binned counting kernel "
                "takes (a power of two of codes, chunk * bps <= {}, chunk << bps <= {})".format(
                    g.chunk, g.bps, kernels.STATES_MAX_ROW_BITS, kernels.STATES_BINS_MAX_COUNTERS))
        whole = samples_per_byte(g.chunk, g.bps)

        def answer():
            n = self._packed_count(count, rest=True)
            if bin_samples % whole:
                raise ValueError("state_series: bins are whole bytes: bin_samples must be a multiple of {} "
                                 "samples".format(whole))
            if self.offset % whole:
                raise ValueError("state_series: bins are whole bytes: seek to a multiple of {} samples".format(whole))
            if n % whole:
                raise ValueError("state_series: bins are whole bytes: count must be a multiple of {} "
                                 "samples".format(whole))
            if not kernels.count_states_bins_supported(g.bps, g.chunk, bin_samples, g.nslot, g.payload_nbytes):
                raise NotImplementedError("state_series: the binned counting kernel does not take bins of {} samples "
                                          "of {} codes x {} bits".format(bin_samples, g.chunk, g.bps))
            kernels.require_gpu()
            nbins = -(-n // bin_samples)
            counts = torch.zeros((g.nslot, nbins, g.chunk, 1 << g.bps), dtype=torch.int32, device='cuda')
            shape = tuple(self._packed_shape(torch.empty((g.nslot, g.chunk, 1 << g.bps), device='meta')).shape)

            def add(dbuf, src, s, e, row_lo, row_hi, first_row):
                kernels.count_states_bins(dbuf, e - s, g.payload_nbytes, g.bps, g.chunk, g.nslot, bin_samples, nbins,
                                          src=src, row_lo=row_lo, row_hi=row_hi, first_row=first_row, counts=counts)

            nbad = self._walk_packed(g.nslot, self.offset, self.offset + n, add) if n else 0
            # (the permuted view of `counts`, or the copy a reshape of it had to make: taken after the walk)
            return counts.permute(1, 0, 2, 3).reshape((nbins,) + shape), nbad

        return self._answer_packed(answer)

    def power_series(self, bin_samples, count=None):
        """Mean ``|x|**2`` per valid sample and time bin, from `state_series`: float64
        device tensor of shape ``(nbins, nthread, nchan)`` (Mark 5B: ``(nbins, nchan)``),
        NaN where a bin holds no valid sample.  Exact up to float64 rounding: the power of
        a bin is ``sum(counts * levels**2)``; nothing is decoded.  Damaged files and
        ``verify=True`` readers: as `state_series`."""
        counts = self.state_series(bin_samples, count)
        levels = torch.from_numpy(self.state_levels).to(counts.device).double()
        power = (counts.double() * levels ** 2).sum(-1)
        valid = counts.sum(-1, dtype=torch.int64)
        if self.complex_data:                           # (re, im) axis: a sample has both
            power, valid = power.sum(-1), valid[..., 0]
        return power / valid.double()

    # -- the walk over the packed bytes that the statistics and the packed reads share
    #    (kernels.count_states, count_states_bins, repack_frames; baseband_amd.convert)
    def _walk_packed(self, nslot, start, stop, visit, strict=False):
        """``visit(dbuf, src, s, e, *piece_rows)`` for the frame sets, of `nslot` slots, that hold
        the samples [start, stop), in pieces [s, e): the packed bytes of a piece on the device
        and its index of payload offsets into them (-1: missing or invalid).  Three ways to the
        bytes: a re-located index, resident bytes, or a `WindowPipeline` over the file image,
        the latter two with the un-fused scan and index at the fixed stride.

        Returns the number of frames that a verifying reader found missing or out of place
        at the fixed stride -- the verdict ``read()`` gets from `_resolve_checks`, from the
        same records (with the header behind the request where the format's read looks at
        it) -- always 0 through a re-located index and under ``verify=False``.  What was
        visited is then not the answer: `_answer_packed`.  `strict`: the walk stands in
        for a read, so that a ``verify=True`` reader on a re-located index answers for the
        sets it covers (`_strict_check`)."""
        spf = self.samples_per_frame
        first, last = start // spf, -(-stop // spf)
        set_nbytes = self._set_nbytes
        located = getattr(self, '_resident', None)
        if located is not None:
            if strict and self.verify is True:
                self._strict_check(first, last)
            dev, src = located
            visit(dev, src[first * nslot:last * nslot].contiguous(), first, last,
                  *piece_rows(start, stop, spf, first, last))
            return 0
        verdict = _WalkVerdict() if self.verify else None
        look = 1 if verdict is not None else 0
        resident = self._resident_bytes()
        if resident is not None:
            lo = min(self._file_offset0 + first * set_nbytes, resident.numel())
            hi = max(lo, min(self._file_offset0 + (last + look) * set_nbytes, resident.numel()))
            win = self._device_window(resident, lo, hi)
            visit(win, self._packed_index(win, first, last - first, verdict), first, last,
                  *piece_rows(start, stop, spf, first, last))
        else:
            image = self._image()
            per_win = min(last - first, max(1, self.window_bytes // set_nbytes))
            pipe = WindowPipeline(image, (per_win + look) * set_nbytes)
            ranges, spans = [], []
            for s in range(first, last, per_win):
                e = min(last, s + per_win)
                lo = min(self._file_offset0 + s * set_nbytes, len(image))
                ahead = look if e == last else 0        # (the header behind the request travels with its last window)
                ranges.append((lo, max(lo, min(self._file_offset0 + (e + ahead) * set_nbytes, len(image)))))
                spans.append((s, e))

            def process(dbuf, i):
                s, e = spans[i]
                win = self._device_window(dbuf, 0, dbuf.numel())
                visit(win, self._packed_index(win, s, e - s, verdict), s, e, *piece_rows(start, stop, spf, s, e))

            try:
                pipe.run(ranges, process)
            finally:
                pipe.release()
        return 0 if verdict is None else verdict.nbad()

    def _strict_check(self, first, last):
        """Raise what a ``verify=True`` read of the frame sets [first, last) through the
        index of located frames raises (formats whose strict reads answer per set)."""

    _lenient = None         # what `_relocate` left on a verify=True reader, for its statistics alone

    def _relocated_meanwhile(self, answer):
        """``answer()`` of a ``verify=True`` reader as its ``verify='fix'`` twin gives it:
        through the index of located frames, which is made once and kept aside.  The
        reader itself is left as it was -- its reads go on raising at what they meet."""
        names = self._relocation_state
        before = {k: self.__dict__[k] for k in names if k in self.__dict__}
        try:
            if self._lenient is None:
                self._relocate()
                self._lenient = {k: self.__dict__[k] for k in names if k in self.__dict__}
            else:
                self.__dict__.update(self._lenient)
            return answer()
        finally:
            for k in names:
                self.__dict__.pop(k, None)
            self.__dict__.update(before)

    def _answer_packed(self, answer, strict=False):
        """What a method that works on the packed bytes returns.  ``answer()`` does all of
        it for the reader as it stands -- takes `count`, checks it against the length,
        makes the outputs, walks -- and returns ``(result, nbad)`` with `_walk_packed`'s
        verdict.  When frames were missing or off the fixed stride the reader does what
        ``read()`` does at that point: a ``verify='fix'`` reader locates its frames
        (`_relocate`) and the WHOLE request is answered again through that index, with
        the length the index gives; a ``verify=True`` reader raises the error of its read
        when the method stands in for one (`strict`: `read_packed`, `frames_valid`), and
        answers the statistics as its lenient twin would (`_relocated_meanwhile`)."""
        result, nbad = answer()
        if not nbad:
            return result
        if strict and self.verify is True:
            msg = ("problem loading frame: {} frame header(s) failed verification "
                   "(bad sync/invariants or unexpected time index)".format(nbad))
            err = self._verification_error(msg)
            if err is not None or not self._can_relocate:
                raise err if err is not None else ValueError("wrong frame number. " + msg)
        if not self._can_relocate or self._relocated:
            return result
        if self.verify is True and not strict:
            return self._relocated_meanwhile(lambda: answer()[0])
        self._relocate()
        self.decode_ahead = False           # (as in read(): warnings belong to the read that meets a hole)
        return answer()[0]

    # -- reads that stand in for ``read()``
    def frames_valid(self, count, samples_per_frame):
        """Host bool array, one entry per frame of `samples_per_frame` samples that the
        next `count` samples from the current offset make up (the last one may be short):
        true when every frame-slot of this stream the frame draws from is there and valid,
        that is, when ``read(count)`` would fill none of its samples.  From the headers
        alone (scan and index); nothing is decoded, the offset stays.

        The call stands in for the read: where ``read(count)`` under ``verify='fix'``
        would locate the frames of a damaged file, so does this (and the answer is that
        of the read which follows); where it would raise under ``verify=True``, this
        raises the same."""
        if self.closed:
            raise ValueError("I/O operation on closed stream.")
        self._packed_count(count)
        g = self._packed_geometry()
        nout = -(-count // samples_per_frame)
        if g is None or count == 0:                         # (no index of payloads: nothing known to be missing)
            return np.ones(nout, bool)

        def answer():
            self._asked = (self.offset, self._packed_count(count))
            kernels.require_gpu()
            start, stop = self.offset, self.offset + count
            marks = _ValidityMarks(nout, samples_per_frame, start, stop, self.samples_per_frame, g.nslot)
            nbad = self._walk_packed(g.nslot, start, stop, lambda dbuf, src, s, e, *rows: marks.add(src, s, e),
                                     strict=True)
            return marks.valid(), nbad

        return self._answer_packed(answer, strict=True)

    def _component_gains(self, scale, g):
        """An array `scale` of `read_packed` -> float32 gains, one per component of a row: broadcast to the
        reader's ``(nthread, nchan)`` (Mark 5B: ``(nchan,)``), a complex channel's gain on (re, im) alike."""
        shape = tuple(self._packed_shape(torch.empty((g.nslot, g.chunk, 1), device='meta')).shape[:-1])
        shape = shape[:-1] if self.complex_data else shape
        gains = np.asarray(scale.detach().cpu() if torch.is_tensor(scale) else scale, dtype=np.float32)
        try:
            gains = np.broadcast_to(gains, shape)
        except ValueError:
            raise ValueError("read_packed: a scale of shape {} does not broadcast to the reader's {}"
                             .format(tuple(gains.shape), shape)) from None
        if not np.isfinite(gains).all():
            raise ValueError("read_packed: scale must be finite")
        return np.repeat(gains.reshape(-1), 2 if self.complex_data else 1)

    def read_packed(self, count, coder, nthread, nchan, samples_per_frame, fill_code, bps=None, scale=None,
                    regroup=False):
        """The next `count` samples as packed payloads of another frame geometry, without
        decoding them (bb_repack_frames) -> ``(payloads, valid)``: a uint8 device tensor of
        shape ``(count // samples_per_frame, nthread, payload_nbytes)`` holding what a
        stream writer of `coder` (``_lib.CODER_*``) with `nthread` threads of `nchan`
        channels and `samples_per_frame` samples per frame would encode ``read(count)``
        to, and a host bool array, true where every frame-slot of this stream that an
        output frame draws from is there and valid.  Samples of the others hold
        `fill_code`.  `count` is a whole number of output frames; the offset must lie on a
        byte boundary of a thread's stream on both sides.  Threads follow the reader's
        selection; a channel `subset` is not applied.  Advances the offset.

        With `bps` other than the reader's, or a `scale`, the samples are requantized on
        the packed bytes (bb_requant_frames): every code goes through the table
        ``kernels.requant_table(own coder, own bps, coder, bps, scale)``, which is decode,
        times ``float32(scale)``, encode.  The thread structure must then be the same on
        both sides (`nthread` threads of as many codes per sample as the reader's), else
        NotImplementedError; `fill_code` is a code of `bps` bits and is not mapped.

        With ``regroup=True`` such a request may change the thread structure as well
        (`nthread` threads of `nchan` channels against the reader's, as from 8-bit VDIF with
        one channel per thread to 2-bit VDIF with one thread, or to Mark 5B): permutation
        and table are then one pass (bb_recode_frames).  Both sides must have the same
        number of components (threads times codes per sample), else NotImplementedError.
        Requests that keep the thread structure, or that do not requantize, go the same
        way with and without it.

        `scale` may also be an array or tensor that broadcasts to the reader's ``(nthread,
        nchan)`` after thread selection (Mark 5B: ``(nchan,)``): one float32 gain per channel,
        a complex channel's on its real and imaginary component alike, as in
        ``fw.write(fr.read(n) * scale)``.  Every component of a row then has a table of its
        own (``kernels.requant_tables``, bb_recode_frames_tables), whether or not the thread
        structure changes; a change still needs ``regroup=True``.  A shape that does not
        broadcast and gains that are not finite are ValueError.  `fill_code` stays ONE code,
        not mapped: on an invalid frame the loop would encode ``fill_value * scale[k]`` per
        channel, so the bytes are the loop's on filled samples when that is one code for
        every channel -- a `fill_value` of 0, the usual case.

        A read in every respect but the decoding: a damaged file is repaired under
        ``verify='fix'`` as ``read(count)`` repairs it (the frames are located and the
        whole request is answered through that index), and ``verify=True`` raises what
        ``read(count)`` raises; the offset then stays."""
        count = operator.index(count)
        g = self._packed_entry('packed reads')
        self._asked = (self.offset, self._packed_count(count))
        chunk_out = nchan * (2 if self.complex_data else 1)
        if count % samples_per_frame:
            raise ValueError("read_packed: count must be a whole number of frames of {} samples"
                             .format(samples_per_frame))
        requant = scale is not None or (bps is not None and bps != g.bps)
        bps_out = g.bps if bps is None else operator.index(bps)
        if samples_per_frame * chunk_out * bps_out % 32:
            raise ValueError("read_packed: payloads are whole 32-bit words")
        payload_out = samples_per_frame * chunk_out * bps_out // 8
        recode = requant and (nthread != g.nslot or chunk_out != g.chunk)
        gains = None if scale is None or np.ndim(scale) == 0 else self._component_gains(scale, g)
        if recode:
            if not regroup:
                raise NotImplementedError(
                    "read_packed: a change of sample width or scale keeps the thread structure ({} x {} codes "
                    "-> {} x {}) unless regroup=True".format(g.nslot, g.chunk, nthread, chunk_out))
            if nthread * chunk_out != g.nslot * g.chunk:
                raise NotImplementedError(
                    "read_packed: a change of sample width or scale keeps the number of components ({} x {} codes "
                    "-> {} x {})".format(g.nslot, g.chunk, nthread, chunk_out))
        if gains is not None:
            if not kernels.recode_tables_supported(g.bps, bps_out, g.chunk, g.nslot, chunk_out, nthread,
                                                   g.payload_nbytes, payload_out):
                raise NotImplementedError(
                    "read_packed: {} x {} codes of {} bits -> {} x {} codes of {} bits is not a conversion the "
                    "recode kernel with a table per component takes".format(g.nslot, g.chunk, g.bps, nthread,
                                                                            chunk_out, bps_out))
        elif recode:
            if not kernels.recode_supported(g.bps, bps_out, g.chunk, g.nslot, chunk_out, nthread,
                                            g.payload_nbytes, payload_out):
                raise NotImplementedError(
                    "read_packed: {} x {} codes of {} bits -> {} x {} codes of {} bits is not a conversion the "
                    "recode kernel takes".format(g.nslot, g.chunk, g.bps, nthread, chunk_out, bps_out))
        elif requant:
            if not kernels.requant_supported(g.bps, bps_out, g.chunk, g.nslot, g.payload_nbytes, payload_out):
                raise NotImplementedError(
                    "read_packed: {} x {} codes of {} bits -> {} bits is not a conversion the requantize "
                    "kernel takes".format(g.nslot, g.chunk, g.bps, bps_out))
        elif not kernels.repack_supported(g.bps, g.coder, coder, g.chunk, g.nslot, chunk_out, nthread,
                                          g.payload_nbytes, payload_out):
            raise NotImplementedError(
                "read_packed: {} x {} codes of {} bits (coder {}) -> {} x {} (coder {}) is not a conversion the "
                "repack kernel takes".format(g.nslot, g.chunk, g.bps, g.coder, nthread, chunk_out, coder))
        whole = samples_per_byte(min(g.chunk, chunk_out), min(g.bps, bps_out))
        if self.offset % whole:
            raise ValueError("read_packed: whole bytes only: seek to a multiple of {} samples".format(whole))
        kernels.require_gpu()
        nout = count // samples_per_frame
        if gains is not None:                               # (uploaded once, for every window of the walk)
            table = torch.from_numpy(kernels.requant_tables(g.coder, g.bps, coder, bps_out, gains)).cuda()
        else:
            table = kernels.requant_table(g.coder, g.bps, coder, bps_out, scale) if requant else None
        if count == 0:
            return torch.empty((0, nthread, payload_out), dtype=torch.uint8, device='cuda'), np.ones(0, bool)

        def answer():
            self._asked = (self.offset, self._packed_count(count))
            out = torch.empty((nout, nthread, payload_out), dtype=torch.uint8, device='cuda')
            start, stop = self.offset, self.offset + count
            marks = _ValidityMarks(nout, samples_per_frame, start, stop, self.samples_per_frame, g.nslot)

            def visit(dbuf, src, s, e, row_lo, row_hi, first_row):
                if gains is not None:
                    kernels.recode_frames_tables(dbuf, e - s, g.payload_nbytes, g.bps, g.chunk, g.nslot, bps_out,
                                                 chunk_out, nthread, payload_out, table, fill_code=fill_code, src=src,
                                                 row_lo=row_lo, row_hi=row_hi, first_row=first_row, out=out.reshape(-1))
                elif recode:
                    kernels.recode_frames(dbuf, e - s, g.payload_nbytes, g.bps, g.chunk, g.nslot, bps_out, chunk_out,
                                          nthread, payload_out, table, fill_code=fill_code, src=src, row_lo=row_lo,
                                          row_hi=row_hi, first_row=first_row, out=out.reshape(-1))
                elif requant:
                    kernels.requant_frames(dbuf, e - s, g.payload_nbytes, g.bps, g.chunk, g.nslot, bps_out, payload_out,
                                           table, fill_code=fill_code, src=src, row_lo=row_lo, row_hi=row_hi,
                                           first_row=first_row, out=out.reshape(-1))
                else:
                    kernels.repack_frames(dbuf, e - s, g.payload_nbytes, g.bps, g.coder, g.chunk, g.nslot, coder,
                                          chunk_out, nthread, payload_out, fill_code=fill_code, src=src,
                                          row_lo=row_lo, row_hi=row_hi, first_row=first_row, out=out.reshape(-1))
                marks.add(src, s, e)

            nbad = self._walk_packed(g.nslot, start, stop, visit, strict=True)
            return (out, marks.valid()), nbad

        out, valid = self._answer_packed(answer, strict=True)
        self.offset += count
        return out, valid
