"""Stream reader for byte-aligned block formats (GUPPI, DADA).

These formats have few, large frames (tens of MiB) with ASCII headers, so
there is no device-side header scan: the host walks the headers and the read
is cut into pieces ``(frame, first row, last row)`` exactly as the reference's
loop would take them (base/base.py:957-967 with the per-format ``_get_frame``
rules).  Runs of frames with the same row range are staged frame-by-frame
through the pinned pipeline and decoded by one kernel launch per window.
"""
import operator

import numpy as np
import torch

from .. import kernels
from ..placement import empty_output
from ..staging import WindowPipeline
from .base import GPUStreamReaderBase, _apply_squeeze, _to_host_array


def bin_counts(nbins, bin_samples, count, device=None):
    """Samples in each of the `nbins` bins of `bin_samples` that a request of `count` samples fills
    (``nbins = ceil(count / bin_samples)``: the last may be short) -> int64 tensor on `device`."""
    n = torch.full((nbins,), bin_samples, dtype=torch.int64, device=device)
    if nbins:
        n[-1] = count - (nbins - 1) * bin_samples
    return n


class BlockStreamReader(GPUStreamReaderBase):
    # subclasses set: _frame_nbytes, _header_nbytes, _file_offset0, _nframes
    def _pieces(self, offset, count):
        """[(frame, row_lo, row_hi), ...] covering `count` samples from
        sample `offset`."""
        raise NotImplementedError

    def _decode_window(self, dbuf, nframes, row_lo, row_hi, out_flat,
                       payload_offset, frame_stride, first_frame):
        raise NotImplementedError

    def _row_range_source(self, frame, a, b):
        """For rows [a, b) of `frame`: ``(pieces, decode)`` where `pieces` is a
        list of (byte offset in the file image, nbytes) that together hold
        those rows and ``decode(dbuf, out_flat)`` decodes them from a device
        buffer in which the pieces lie back to back -- or None when the format
        has no such shortcut (the whole frame is staged then)."""
        return None

    _touched = None         # sample offset at which the previous small request ended
    _prefetch = None        # (frame, future) of a frame on its way to HBM in the background
    prefetch_next = True    # set False to stage every frame when it is first needed

    def _start_prefetch(self, frame):
        """A sequential loop of small reads is inside frame - 1: bring `frame`
        to HBM on the worker thread meanwhile (`staging.upload_in_background`)."""
        if (not self.prefetch_next or frame >= self._nframes or self._resident_bytes() is not None
                or (self._prefetch is not None and self._prefetch[0] == frame)):
            return
        from ..staging import upload_in_background
        image = self._image()
        lo, nbytes = self._frame_span(frame)
        self._prefetch = (frame, upload_in_background(image, lo, min(lo + nbytes, len(image))))

    def _take_prefetch(self, frame):
        """The device bytes of `frame` if they were prefetched, else None."""
        pending, self._prefetch = self._prefetch, None
        if pending is None:
            return None
        dev, done = pending[1].result()             # (also waits out a prefetch nobody wants)
        if pending[0] != frame:
            return None
        torch.cuda.current_stream().wait_event(done)
        return dev

    def close(self):
        if self._prefetch is not None:
            try:
                self._prefetch[1].result()
            except Exception:
                pass
            self._prefetch = None
        super().close()
    _chan_lo = 0            # first channel decoded (`_plan_channel_range`)
    _sel = None             # (first pol, pols kept, int32 channel list): a selection that is not a plain range
    _cmap_dev = None

    def _plan_channel_range(self):
        """For (pol, chan) samples decoded by bb_decode_i8_tiled: fold a
        `subset` into the decode instead of decoding whole blocks and indexing
        afterwards, as the reference does (base/base.py:706-717 after
        guppi/payload.py:90-102, dada/payload.py:76-79).

        * all polarisations and a contiguous RANGE of channels: the same decode
          with the payload entered at the first kept channel and fewer channels
          (`nchan_stored` tells the kernel the strides); the other channels are
          not written and -- where the format stores channels apart (GUPPI
          channels-first) -- not read either.  Every kernel takes this.
        * any channel LIST (gaps, any order) and / or one of two polarisations:
          `chan_map` / `pol_first` of bb_tiled_params (`_sel`); taken by the
          fast transposing kernel only -- `_tiled_decode` falls back to decoding
          whole blocks and indexing when the library answers ENOTSUP.

        Checked by value, like `_plan_channel_select`: the subset is applied to
        arrays of polarisation and channel numbers."""
        if not self.subset or len(self._unsliced_shape) != 2:
            return
        npol, nchan = self._unsliced_shape
        chan = np.broadcast_to(np.arange(nchan), (npol, nchan))
        pol = np.broadcast_to(np.arange(npol)[:, np.newaxis], (npol, nchan))

        def view(a):
            a = np.ascontiguousarray(a)[np.newaxis]
            if self.squeeze:
                a = a.reshape(a.shape[:1] + tuple(s for s in a.shape[1:] if s > 1))
            return a[(slice(None),) + tuple(self.subset)]
        try:
            c, p = view(chan).reshape(-1), view(pol).reshape(-1)
        except Exception:
            return
        if c.size == 0:
            return
        # the polarisations kept: a run pf, pf + 1, ... each with the same channel list
        npk = int(np.unique(p).size)
        if c.size % npk:
            return
        m, pf, lo = c.size // npk, int(p[0]), int(c[0])
        cl = c[:m]
        if not (np.array_equal(p, np.repeat(np.arange(pf, pf + npk), m))
                and np.array_equal(c, np.tile(cl, npk))):
            return
        whole_pols = npk == npol
        if whole_pols and np.array_equal(cl, np.arange(lo, lo + m)):
            if m == nchan:
                return                              # everything, in order: nothing to fold
            self._chan_lo = lo
            self._decode_shape = (npol, m)
            self._within_np = np.arange(lo, lo + m, dtype=np.int32)     # (the decode applies the subset)
            return
        if not (whole_pols or (npol == 2 and npk == 1)) or m % 2 or m > 65536:
            return                                  # (the kernel writes channel pairs; odd counts index afterwards)
        self._sel = (pf, npk, cl.astype(np.int32))
        self._decode_shape = (npk, m)
        self._within_np = cl.astype(np.int32)

    def _tiled_decode(self, dbuf, nframes, layout, ntime, a, b, src0, src_stride, out_flat):
        """Times [a, b) of `nframes` blocks of `ntime` stored times each (payloads
        at ``src0 + i * src_stride``) -> `out_flat`, honouring the planned channel
        range or selection."""
        npol_s, nchan_s = self._unsliced_shape
        if self._sel is None:
            skip = kernels.tiled_channel_skip(layout, npol_s, ntime, self._chan_lo)
            kernels.decode_i8_tiled(dbuf, nframes, layout, npol_s, self._decode_shape[-1], ntime, a, b,
                                    src0=src0 + skip, src_stride=src_stride, out=out_flat,
                                    nchan_stored=nchan_s)
            return
        pf, npk, cl = self._sel
        if self._cmap_dev is None or self._cmap_dev.device != dbuf.device:
            self._cmap_dev = torch.from_numpy(cl).to(dbuf.device)
        try:
            kernels.decode_i8_tiled(dbuf, nframes, layout, npk, cl.size, ntime, a, b, src0=src0,
                                    src_stride=src_stride, out=out_flat, nchan_stored=nchan_s,
                                    npol_stored=npol_s, pol_first=pf, chan_map=self._cmap_dev)
            return
        except KeyError:
            pass
        # a geometry the selecting kernel does not take (unaligned payloads):
        # whole blocks, then the index -- the reference's order -- in pieces of
        # at most 1 GiB of decoded samples
        rows = b - a
        per = max(1, (1 << 28) // max(1, rows * npol_s * nchan_s * 2))
        idx = self._cmap_dev.long()
        n_out = rows * npk * cl.size * 2
        for f0 in range(0, nframes, per):
            n = min(per, nframes - f0)
            tmp = kernels.decode_i8_tiled(dbuf, n, layout, npol_s, nchan_s, ntime, a, b,
                                          src0=src0 + f0 * src_stride, src_stride=src_stride)
            part = tmp.view(n * rows, npol_s, nchan_s, 2)[:, pf:pf + npk][:, :, idx]
            out_flat[f0 * n_out:(f0 + n) * n_out] = part.reshape(-1)

    def _frame_span(self, frame):
        """(byte offset of the frame in the file, number of bytes to stage)."""
        return (self._file_offset0 + frame * self._frame_nbytes,
                self._frame_nbytes)

    def _cut_windows(self, f0, f1, image_nbytes):
        """The run of frames [f0, f1) in windows of whole frames, as many as `window_bytes` holds and one at
        the least -> ``(cap, ranges, spans)``: the bytes a window may take, every window's bytes ``(lo, hi)``
        of the image (the last frame cut at the image's end) and its frames ``(s, e)``."""
        per_win = max(1, self.window_bytes // self._frame_nbytes)
        cap = max(per_win * self._frame_nbytes, self._frame_span(f0)[1])
        ranges, spans = [], []
        for s in range(f0, f1, per_win):
            e = min(f1, s + per_win)
            last_lo, last_n = self._frame_span(e - 1)
            ranges.append((self._frame_span(s)[0], min(last_lo + last_n, image_nbytes)))
            spans.append((s, e))
        return cap, ranges, spans

    def _windows(self, image, f0, f1):
        """``(ranges, spans)`` of `_cut_windows` for `image`, with `self._pipeline` large enough for them."""
        cap, ranges, spans = self._cut_windows(f0, f1, len(image))
        if self._pipeline is None or self._pipeline.cap < cap:
            self._pipeline = WindowPipeline(image, cap)
        return ranges, spans

    read_through = True     # queue a read-only pass over a request's frames in front of their decode (kernels.touch)

    def read(self, count=None, out=None):
        if self.closed:
            raise ValueError("I/O operation on closed stream.")
        samples_left = self.shape[0] - self.offset
        if out is None:
            if count is None or count < 0:
                count = max(0, samples_left)
        else:
            assert tuple(out.shape[1:]) == self.sample_shape, (
                "'out' must have trailing shape {}".format(self.sample_shape))
            count = out.shape[0]
        if count > samples_left:
            raise EOFError("cannot read from beyond end of input.")
        kernels.require_gpu()
        if isinstance(out, torch.Tensor):
            self._refuse_complex_bfloat16(out.dtype)
        # element type of the result (`sample_dtype`, or what a tensor `out` is made of); a 16-bit
        # type this format's kernels do not write is decoded to float32 and converted at the end
        elem = self._elem_dtype() if out is None else self._out_elem(out)
        convert = elem != torch.float32 and not self._half_direct(elem)
        ncomp = 2 if self.complex_data else 1
        row = int(np.prod(self._decode_shape)) * ncomp
        # pieces land exactly where they belong, so a suitable `out` tensor is
        # decoded into directly
        direct = (isinstance(out, torch.Tensor) and out.is_cuda and out.is_contiguous()
                  and count > 0 and (not self.subset or self._within_np is not None)
                  and out.dtype in ((torch.complex64, torch.complex32) if self.complex_data
                                    else (torch.float32, torch.float16, torch.bfloat16)))
        pieces = self._pieces(self.offset, count)
        image = self._image()
        resident = self._resident_bytes()
        if resident is not None and pieces and self.read_through:
            # The frames of this request are in HBM: a pass that only reads them is queued NOW,
            # before the output is drawn and the launches are prepared; the decode behind it finds
            # its input -- a fifth of an int8 decode's traffic -- in the memory-side cache and runs
            # 20-25 % faster (profiles/r06dm_exp_cached_input_int8.log)
            lo = self._frame_span(pieces[0][0])[0]
            last_lo, last_n = self._frame_span(pieces[-1][0])
            hi = min(last_lo + last_n, resident.numel())
            if 2 * count * self._frame_nbytes >= (hi - lo) * self.samples_per_frame:    # (most of it is wanted)
                kernels.touch(resident, lo, hi - lo)
        if direct and not convert:
            flat = (torch.view_as_real(out) if self.complex_data else out).reshape(-1)
        else:
            flat = kernels.empty_decoded(count * row, dtype=torch.float32 if convert else elem)
        # merge consecutive frames that use the same row range into runs
        runs = []
        for f, a, b in pieces:
            if runs and runs[-1][1] == f and tuple(runs[-1][2:]) == (a, b):
                runs[-1][1] = f + 1
            else:
                runs.append([f, f + 1, a, b])
        done = 0
        # requests of less than one frame (loops of small reads): the frame is
        # staged once and kept in HBM; following requests inside it only launch
        # kernels instead of staging the whole block again for every call
        if count < self.samples_per_frame and len(runs) <= 2 and all(r[1] == r[0] + 1 for r in runs):
            from ..staging import upload
            for f0, f1, a, b in runs:
                o = flat[done * row:(done + (b - a)) * row]
                done += b - a
                cached = self._ahead is not None and self._ahead[0] == f0
                # random access: stage just the rows asked for; a request that
                # continues where the previous small one ended (a sequential
                # loop) brings the whole frame in
                source = None if cached or self._touched == self.offset else self._row_range_source(f0, a, b)
                if resident is not None:
                    # the frame is in HBM already: decode from where it lies
                    lo, nbytes = self._frame_span(f0)
                    self._decode_window(self._device_window(resident, lo, min(lo + nbytes, resident.numel())),
                                        1, a, b, o, self._header_nbytes, self._frame_nbytes, f0)
                    continue
                if source is not None:
                    pieces, decode = source
                    host = np.concatenate([image[lo:lo + n] for lo, n in pieces]) if len(pieces) > 1 \
                        else image[pieces[0][0]:pieces[0][0] + pieces[0][1]]
                    decode(upload(host), o)
                    continue
                if not cached:
                    dev = self._take_prefetch(f0)
                    if dev is None:
                        lo, nbytes = self._frame_span(f0)
                        dev = upload(image[lo:min(lo + nbytes, len(image))])
                    self._ahead = (f0, dev)
                    # a sequential loop: the next frame travels while this one is consumed
                    self._start_prefetch(f0 + 1)
                self._decode_window(self._ahead[1], 1, a, b, o, self._header_nbytes,
                                    self._frame_nbytes, f0)
            runs = []
            self._touched = self.offset + count
        for f0, f1, a, b in runs:
            if resident is not None:
                # ONE launch for the whole run of frames, straight from HBM
                lo = self._frame_span(f0)[0]
                last_lo, last_n = self._frame_span(f1 - 1)
                hi = min(last_lo + last_n, resident.numel())
                o = flat[done * row:(done + (f1 - f0) * (b - a)) * row]
                self._decode_window(self._device_window(resident, lo, hi), f1 - f0, a, b, o,
                                    self._header_nbytes, self._frame_nbytes, f0)
                done += (f1 - f0) * (b - a)
                continue
            ranges, spans = self._windows(image, f0, f1)
            base = done

            def process(dbuf, i, base=base, a=a, b=b, f0=f0):
                s, e = spans[i]
                o = flat[(base + (s - f0) * (b - a)) * row:
                         (base + (e - f0) * (b - a)) * row]
                self._decode_window(dbuf, e - s, a, b, o, self._header_nbytes,
                                    self._frame_nbytes, s)

            self._pipeline.run(ranges, process)
            done += (f1 - f0) * (b - a)
        assert done == count
        if direct:
            if convert:
                (torch.view_as_real(out) if self.complex_data else out).reshape(-1).copy_(flat)
            self.offset += count
            return out
        if convert:
            flat = flat.to(elem)
        if self.complex_data:
            flat = torch.view_as_complex(flat.view(-1, 2))
        data = flat.reshape((count,) + tuple(self._decode_shape))
        data = self._squeeze_and_subset(data)
        self.offset += count
        if out is None:
            if self.host_results:           # (what the plugin modules switch on: NumPy arrays, base/base.py)
                from ..staging import download_new
                return download_new(data)
            return data
        if isinstance(out, torch.Tensor):
            out.copy_(data)
        else:
            _to_host_array(data, out)
        return out

    # -- power and moments per channel and time bin from the stored int8 bytes (kernels.i8_moments)
    moments_fallback_bytes = 256 << 20      # decoded bytes per piece of the fallback (read, then reduce)

    def _moments_geometry(self):
        """``(layout, ncomp)`` of the stored int8 samples for `kernels.i8_moments`
        (``_lib.MOMENTS_*``), or a str: why the kernel does not take this stream."""
        return "{} has no kernel for its stored samples".format(type(self).__name__)

    def _moments_ntime(self, frame):
        """Times stored in the payload of `frame`."""
        return self.samples_per_frame

    def _moments_plan(self, bin_samples):
        """``(layout, npol, nchan, ncomp)`` where the kernel takes this stream with bins of
        `bin_samples`, else the reason as a str."""
        geom = self._moments_geometry()
        if isinstance(geom, str):
            return geom
        layout, ncomp = geom
        npol, nchan = self._unsliced_shape
        ntimes = {self._moments_ntime(0), self._moments_ntime(self._nframes - 1)}
        for ntime in ntimes:
            if not kernels.i8_moments_supported(layout, npol, nchan, ncomp, ntime, bin_rows=bin_samples,
                                                src0=self._header_nbytes, src_stride=self._frame_nbytes):
                return ("the moments kernel does not take {} pol x {} chan x {} components, {} times a frame, "
                        "payloads at {} + k * {} bytes".format(npol, nchan, ncomp, ntime, self._header_nbytes,
                                                               self._frame_nbytes))
        return layout, npol, nchan, ncomp

    def _launch_per_run(self, count, add):
        """The walk of `moment_series` and `coherence_series` over the samples ``read(count)`` would
        return from the offset: ``add(dbuf, nframes, a, b, nt, first_row)`` once per run of frames that
        share a row range [a, b) and a payload of `nt` times -- from the resident bytes, from the
        frame that small reads keep staged, or window by window -- with `first_row` the place of
        the run's (the window's) first sample in the request."""
        # runs of frames that share a row range and a payload size: one launch each (per window)
        runs = []
        for f, a, b in self._pieces(self.offset, count):
            nt = self._moments_ntime(f)
            if runs and runs[-1][1] == f and tuple(runs[-1][2:]) == (a, b, nt):
                runs[-1][1] = f + 1
            else:
                runs.append([f, f + 1, a, b, nt])
        image = self._image()
        resident = self._resident_bytes()
        done = 0
        for f0, f1, a, b, nt in runs:
            if resident is not None:
                lo = self._frame_span(f0)[0]
                last_lo, last_n = self._frame_span(f1 - 1)
                add(self._device_window(resident, lo, min(last_lo + last_n, resident.numel())), f1 - f0, a, b, nt, done)
            elif f1 == f0 + 1 and self._ahead is not None and self._ahead[0] == f0:
                add(self._ahead[1], 1, a, b, nt, done)      # the frame that small reads keep staged
            else:
                ranges, spans = self._windows(image, f0, f1)

                def process(dbuf, i, base=done, a=a, b=b, nt=nt, f0=f0):
                    s, e = spans[i]
                    add(dbuf, e - s, a, b, nt, base + (s - f0) * (b - a))

                self._pipeline.run(ranges, process)
            done += (f1 - f0) * (b - a)
        assert done == count

    def _series_request(self, name, bin_samples, count, check=None):
        """What `moment_series` and `coherence_series` (`name`) check before anything else, in this order:
        the stream is open, `bin_samples`, int8 samples, `check()` (what else the method asks of the
        stream), `count`, a GPU -> ``(bin_samples, count, nbins)`` as plain numbers, and what `check`
        returned.  `power_series` and `stokes_series` ask it too, for the samples of their bins."""
        if self.closed:
            raise ValueError("I/O operation on closed stream.")
        bin_samples = operator.index(bin_samples)
        if bin_samples < 1:
            raise ValueError(name + ": bin_samples must be at least 1")
        if self.bps != 8:
            raise NotImplementedError("{}: samples of {} bits are not int8".format(name, self.bps))
        checked = check() if check is not None else None
        left = self.shape[0] - self.offset
        if count is None or count < 0:
            count = max(0, left)
        if count > left:
            raise EOFError("cannot read from beyond end of input.")
        kernels.require_gpu()
        return bin_samples, count, -(-count // bin_samples), checked

    def _series_plan(self, name, plan_of, bin_samples, packed):
        """``plan_of(bin_samples)`` where the kernel serves the request, None where the fallback does:
        with ``packed=False``, and where the plan is a str, the reason why the kernel does not take the
        stream -- which ``packed=True`` raises as `NotImplementedError`."""
        plan = None if packed is False else plan_of(bin_samples)
        if isinstance(plan, str):
            if packed:
                raise NotImplementedError(name + ": " + plan)
            plan = None
        return plan

    def moment_series(self, bin_samples, count=None, packed=None):
        """Sum of x and sum of x * x of every real component per time bin, over the samples
        ``read(count)`` would return from the current offset -> int64 device tensor of shape
        ``(nbins,) + sample_shape + ((2,) if complex) + (2,)`` with ``nbins = ceil(count /
        bin_samples)``; the last axis is (sum x, sum x * x), the one before it (real,
        imaginary).  Bin ``b`` covers the samples ``[offset + b * bin_samples, offset + (b + 1)
        * bin_samples)`` (the last bin may be short).  The offset does not move.

        With ``packed=None`` the sums come from the stored int8 bytes where the kernel takes the
        stream (bb_i8_moments: one pass over the file's bytes, nothing is decoded, every stored
        channel summed; `squeeze` and `subset` are applied to the small result as ``read()``
        applies them to a sample) and from ``read()`` in pieces followed by a reduction
        elsewhere (MKBF heaps, real GUPPI samples, samples of 6 bytes, payloads off a dword);
        both are exact.  ``packed=False`` always reads and reduces, ``packed=True`` raises
        `NotImplementedError` where the kernel does not take the stream."""
        bin_samples, count, nbins, _ = self._series_request('moment_series', bin_samples, count)
        plan = self._series_plan('moment_series', self._moments_plan, bin_samples, packed)
        if plan is None:
            return self._moments_by_read(bin_samples, count, nbins)
        layout, npol, nchan, ncomp = plan
        sums = torch.zeros((nbins, npol, nchan, ncomp, 2), dtype=torch.int64, device='cuda')

        def add(dbuf, nframes, a, b, nt, first_row):
            kernels.i8_moments(dbuf, nframes, layout, npol, nchan, ncomp, nt, a, b, bin_samples, nbins,
                               first_row=first_row, src0=self._header_nbytes, src_stride=self._frame_nbytes, sums=sums)

        self._launch_per_run(count, add)
        if ncomp == 1:
            sums = sums.reshape(nbins, npol, nchan, 2)
        # squeeze and subset, as read() applies them to a sample
        if self.squeeze:
            sums = sums.reshape((nbins,) + _apply_squeeze((npol, nchan)) + tuple(sums.shape[3:]))
        if self.subset:
            sums = sums[(slice(None),) + self._torch_subset()]
        return sums

    def _moments_by_read(self, bin_samples, count, nbins):
        """`moment_series` from ``read()`` in pieces of at most `moments_fallback_bytes` of
        decoded samples, summed in int64 (exact: the decoded values are the stored integers)."""
        comp = (2,) if self.complex_data else ()
        sums = torch.zeros((nbins,) + tuple(self.sample_shape) + comp + (2,), dtype=torch.int64, device='cuda')

        def values(data):
            x = (torch.view_as_real(data) if self.complex_data else data).to(torch.int64)
            return torch.stack((x, x * x), -1)

        return self._binned_by_read(bin_samples, count, sums, values)

    def _binned_by_read(self, bin_samples, count, sums, values):
        """``values(data)`` (int64, a row per sample) of ``read()`` in pieces of at most
        `moments_fallback_bytes` of decoded samples, added up per bin into `sums`; the offset
        does not move."""
        per_sample = 4 * max(1, int(np.prod(self.sample_shape))) * (2 if self.complex_data else 1)
        step = max(1, self.moments_fallback_bytes // per_sample)
        offset, host = self.offset, self.host_results
        self.host_results = False
        try:
            for lo in range(0, count, step):
                n = min(step, count - lo)
                x = values(self.read(n))
                # the rows up to the next bin edge, whole bins, the rest
                head = min(n, -lo % bin_samples)
                whole = (n - head) // bin_samples
                b = (lo + head) // bin_samples
                if head:
                    sums[lo // bin_samples] += x[:head].sum(0)
                if whole:
                    sums[b:b + whole] += x[head:head + whole * bin_samples].reshape(
                        (whole, bin_samples) + tuple(x.shape[1:])).sum(1)
                if head + whole * bin_samples < n:
                    sums[b + whole] += x[head + whole * bin_samples:].sum(0)
        finally:
            self.offset, self.host_results = offset, host
        return sums

    def power_series(self, bin_samples, count=None, packed=None):
        """Mean ``|x|**2`` per sample and time bin, from `moment_series`: float64 device tensor
        of shape ``(nbins,) + sample_shape``: the sum of x * x over the components of a bin,
        divided by the number of samples in it.  Name and meaning are those of the VDIF and
        Mark 5B method; `packed` as in `moment_series`."""
        bin_samples, count, nbins, _ = self._series_request('moment_series', bin_samples, count)
        sq = self.moment_series(bin_samples, count, packed)[..., 1]
        if self.complex_data:
            sq = sq.sum(-1)
        n = bin_counts(nbins, bin_samples, count, sq.device)
        return sq.double() / n.double().reshape((nbins,) + (1,) * (sq.dim() - 1))

    # -- cross-polarisation products per channel and time bin from the stored int8 bytes (kernels.i8_coherence)
    def _coherence_channels(self):
        """The channels of the answer: squeeze and subset applied to the index grid of (npol, nchan)
        must leave polarisation 0, then polarisation 1, over the same channels -> int64 array of
        those channels, shaped as the channel part of a sample."""
        npol, nchan = self._unsliced_shape
        if npol != 2:
            raise ValueError("coherence_series needs a stream of exactly two polarisations, not {}".format(npol))
        grid = np.arange(npol * nchan).reshape(npol, nchan)
        if self.squeeze:
            grid = grid.reshape(_apply_squeeze(grid.shape))
        if self.subset:
            grid = grid[tuple(np.asarray(s) if isinstance(s, list) else s for s in self.subset)]
        grid = np.asarray(grid)
        if grid.ndim < 1 or grid.shape[0] != 2 or (grid[0] >= nchan).any() or not np.array_equal(grid[1], grid[0] + nchan):
            raise ValueError("coherence_series: the subset must keep both polarisations, 0 then 1, over the same "
                             "channels; this one selects (pol, chan) = {}".format(
                                 [divmod(int(i), nchan) for i in grid.reshape(-1)[:8]]))
        return grid[0]

    def _coherence_plan(self, bin_samples):
        """``(layout, nchan)`` where the kernel takes this stream with bins of `bin_samples`, else
        the reason as a str."""
        geom = self._moments_geometry()
        if isinstance(geom, str):
            return geom
        layout, ncomp = geom
        if ncomp != 2:
            return "real samples have no coherence kernel"
        nchan = self._unsliced_shape[1]
        for ntime in {self._moments_ntime(0), self._moments_ntime(self._nframes - 1)}:
            if not kernels.i8_coherence_supported(layout, nchan, ntime, bin_rows=bin_samples,
                                                  src0=self._header_nbytes, src_stride=self._frame_nbytes):
                return ("the coherence kernel does not take 2 pol x {} chan, {} times a frame, payloads at "
                        "{} + k * {} bytes".format(nchan, ntime, self._header_nbytes, self._frame_nbytes))
        return layout, nchan

    def coherence_series(self, bin_samples, count=None, packed=None):
        """Cross-polarisation products per channel and time bin of a stream of two polarisations
        X, Y, over the samples ``read(count)`` would return from the current offset -> int64
        device tensor of shape ``(nbins, nchan, 4)`` (``(nbins, 4)`` with `squeeze` and one
        channel), ``nbins = ceil(count / bin_samples)``; the last axis is (sum ``|X|**2``, sum
        ``|Y|**2``, Re sum ``X * conj(Y)``, Im sum ``X * conj(Y)``).  Bins as in `moment_series`;
        the offset does not move.  A `subset` must keep both polarisations over the same
        channels (`ValueError` otherwise); those channels select from the answer.

        With ``packed=None`` the sums come from the stored int8 bytes where the kernel takes the
        stream (bb_i8_coherence: one pass over the file's bytes, nothing is decoded) and from
        ``read()`` in pieces followed by a reduction elsewhere (MKBF heaps, an odd number of
        channels above one in plain DADA, payloads off a dword, real samples: X * Y, then 0);
        both are exact.  ``packed=False`` always reads and reduces, ``packed=True`` raises
        `NotImplementedError` where the kernel does not take the stream."""
        bin_samples, count, nbins, chans = self._series_request('coherence_series', bin_samples, count,
                                                                check=self._coherence_channels)
        plan = self._series_plan('coherence_series', self._coherence_plan, bin_samples, packed)
        if plan is None:
            return self._coherence_by_read(bin_samples, count, nbins, chans.shape)
        layout, nchan = plan
        sums = torch.zeros((nbins, nchan, 4), dtype=torch.int64, device='cuda')

        def add(dbuf, nframes, a, b, nt, first_row):
            kernels.i8_coherence(dbuf, nframes, layout, nchan, nt, a, b, bin_samples, nbins,
                                 first_row=first_row, src0=self._header_nbytes, src_stride=self._frame_nbytes, sums=sums)

        self._launch_per_run(count, add)
        if not (chans.shape == (nchan,) and np.array_equal(chans, np.arange(nchan))):
            sums = sums[:, torch.from_numpy(chans.reshape(-1).astype(np.int64)).cuda()]
        return sums.reshape((nbins,) + chans.shape + (4,))

    def _coherence_by_read(self, bin_samples, count, nbins, chan_shape):
        """`coherence_series` from ``read()`` in pieces, summed in int64 (exact: the decoded values
        are the stored integers); a sample is (2,) + `chan_shape` (`_coherence_channels`)."""
        sums = torch.zeros((nbins,) + tuple(chan_shape) + (4,), dtype=torch.int64, device='cuda')

        def values(data):
            if not self.complex_data:
                x, y = data[:, 0].to(torch.int64), data[:, 1].to(torch.int64)
                return torch.stack((x * x, y * y, x * y, torch.zeros_like(x)), -1)
            z = torch.view_as_real(data).to(torch.int64)
            xr, xi, yr, yi = z[:, 0, ..., 0], z[:, 0, ..., 1], z[:, 1, ..., 0], z[:, 1, ..., 1]
            return torch.stack((xr * xr + xi * xi, yr * yr + yi * yi, xr * yr + xi * yi, xi * yr - xr * yi), -1)

        return self._binned_by_read(bin_samples, count, sums, values)

    def stokes_series(self, bin_samples, count=None, packed=None):
        """``(XX + YY, XX - YY, 2 Re, 2 Im)`` of `coherence_series` (XX, YY, Re, Im its last axis),
        divided by the number of samples in the bin (the last bin may be short) -> float64
        device tensor of the same shape."""
        bin_samples, count, nbins, _ = self._series_request('coherence_series', bin_samples, count,
                                                            check=self._coherence_channels)
        xx, yy, re, im = self.coherence_series(bin_samples, count, packed).unbind(-1)
        s = torch.stack((xx + yy, xx - yy, 2 * re, 2 * im), -1)
        n = bin_counts(nbins, bin_samples, count, s.device)
        return s.double() / n.double().reshape((nbins,) + (1,) * (s.dim() - 1))
