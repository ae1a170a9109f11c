"""File and stream reader bases.

Host-side mirror of the reference's ``FileBase``/``VLBIFileReaderBase``
(base/base.py:54-406) and ``StreamReaderBase``/``VLBIStreamReaderBase``
(base/base.py:602-1227).  The public surface is the same -- ``read(count,
out)``, ``seek``, ``tell``, ``shape/size/ndim/dtype/sample_shape``,
``start_time/stop_time/time``, ``squeeze/subset/fill_value/verify``, context
manager, ``close`` -- but ``read`` does not loop over frames in Python
(base/base.py:957-967).  It maps the requested sample range to a range of
frame sets, streams the corresponding bytes to HBM in large windows
(`staging.WindowPipeline`), and per window launches header scan ->
index build -> decode.  The result is a device tensor.
"""
import operator
import io
import os
import threading
import warnings

import numpy as np
import torch

from .. import _lib
from .. import kernels
from ..placement import empty_output
from .. import placement as _placement
from ..staging import host_image, WindowPipeline
from .packed import PackedBytesMixin
from .quantities import as_time, as_timedelta, is_time_like, is_duration_like

# BB_SIDE_SCAN=0: the scan of a request on resident bytes stays on the caller's stream
_SIDE_SCAN = os.environ.get('BB_SIDE_SCAN', '1') not in ('0', 'no', 'off')
_scan_streams = {}              # device index -> the side stream of every reader's scans there
_scan_streams_lock = threading.Lock()

__all__ = ['FileBase', 'VLBIFileReaderBase', 'GPUStreamReaderBase',
           'HeaderNotFoundError']


class HeaderNotFoundError(LookupError):
    pass


class FileBase:
    """Thin wrapper around a binary filehandle (base/base.py:54-151)."""

    def __init__(self, fh_raw):
        self.fh_raw = fh_raw

    def __getattr__(self, attr):
        if attr == 'fh_raw':
            raise AttributeError(attr)
        return getattr(self.fh_raw, attr)

    # A stream writer queues the frames it has packed for this handle
    # (staging.write_device_bytes; the queue writes to `fh_raw` itself).  Whoever asks
    # where the file stands, or writes or seeks on the side, finds the file as if
    # every frame had been written when ``write`` returned -- as in the reference.
    _queues_writes = True

    # Pickling a file reader: what it was given, where it stands, and the NAME of the
    # file underneath -- the handle is opened again on arrival (base/base.py:123-151 in
    # the reference); images of the file, windows in HBM and the info are made again.
    _unpickled_state = ('_image', '_frame_dev', '_frame_end', '_frame_run', '_frame_dev_bytes', 'info', '_info')

    def __getstate__(self):
        if self.writable():
            raise TypeError('cannot pickle file opened for writing')
        state = {k: v for k, v in self.__dict__.items() if k not in self._unpickled_state}
        fh = state['fh_raw']
        if isinstance(fh, io.IOBase):
            del state['fh_raw']
            state['_reopen'] = (fh.name, fh.mode, None if fh.closed else fh.tell())
        return state

    def __setstate__(self, state):
        reopen = state.pop('_reopen', None)
        if reopen is not None:
            name, mode, offset = reopen
            fh = io.open(name, mode)
            if offset is None:
                fh.close()
            else:
                fh.seek(offset)
            state['fh_raw'] = fh
        self.__dict__.update(state)

    def _settle(self):
        from .. import staging
        if staging._sinks:
            staging.finish_writes(self, close_sink=False)

    def tell(self):
        self._settle()
        return self.fh_raw.tell()

    def seek(self, *args):
        self._settle()
        return self.fh_raw.seek(*args)

    def write(self, data):
        self._settle()
        return self.fh_raw.write(data)

    class _TemporaryOffset:
        def __init__(self, fh, offset, whence):
            self.fh, self.offset, self.whence = fh, offset, whence

        def __enter__(self):
            self.old = self.fh.tell()
            if self.offset is not None:
                self.fh.seek(self.offset, self.whence)
            return self.fh

        def __exit__(self, *exc):
            self.fh.seek(self.old)

    def temporary_offset(self, offset=None, whence=0):
        return self._TemporaryOffset(self, offset, whence)

    # -- frame-at-a-time loops over a binary file ('rb': read_frame().data ...)
    _frame_end = None       # file offset at which the previous frame read here ended
    _frame_run = 0          # frames read back to back
    _frame_dev = None       # (lo, hi, device bytes) window of the file kept in HBM
    _frame_dev_bytes = 1 << 20

    def _lend_device_words(self, frame):
        """The frame just read ends at the current file position.  In a loop
        that reads frame after frame, ``frame.payload`` gets its bytes as a
        view of a window of the file kept in HBM (1 MiB, quadrupling up to 64
        MiB while the loop goes on), so that ``.data`` only launches the decode
        -- without a host-to-device copy for every single payload.  The host
        words stay what they are; writing to them drops the device view
        (`PayloadBase._device_words`)."""
        payload = getattr(frame, 'payload', frame)         # (a frame, or a payload read on its own)
        try:
            end = self.fh_raw.tell()
            nbytes = payload.nbytes
        except Exception:
            return frame
        start = end - nbytes
        prev, self._frame_end = self._frame_end, end
        # (a frame that begins where the previous one ended, give or take its header)
        if prev is None or not 0 <= start - prev <= 65536:
            self._frame_run, self._frame_dev, self._frame_dev_bytes = 0, None, 1 << 20
            return frame
        self._frame_run += 1
        if (self._frame_run < 2 or start % 8 or nbytes > (16 << 20)
                or getattr(payload, '_dwords', None) is not None):
            # (large block payloads stage just the rows they are asked for)
            return frame
        if self._frame_dev is None and not torch.cuda.is_available():
            self._frame_end = None              # (no GPU: `.data` will say so itself)
            return frame
        win = self._frame_dev
        if win is None or not (win[0] <= start and end <= win[1]):
            try:
                image = host_image(self.fh_raw)
            except Exception:
                return frame
            from ..staging import upload
            resident = getattr(image, 'device_tensor', None)
            if resident is not None:            # the file IS in HBM (open(<device tensor>, 'rb'))
                if resident.data_ptr() % 8:
                    return frame
                win = self._frame_dev = (0, len(image), resident)
            else:
                hi = min(len(image), start + max(nbytes, self._frame_dev_bytes))
                if hi < end:
                    return frame
                win = self._frame_dev = (start, hi, upload(image[start:hi]))
                self._frame_dev_bytes = min(64 << 20, 4 * self._frame_dev_bytes)
        words = getattr(payload, 'words', None)
        if words is not None and getattr(words, 'flags', None) is not None and not words.flags.writeable:
            payload._dwords = win[2][start - win[0]:end - win[0]]
        return frame

    def close(self):
        self._frame_dev = None
        img, self._image = getattr(self, '_image', None), None
        if img is not None:
            from ..staging import retire_image
            retire_image(img)
        self.fh_raw.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __repr__(self):
        return "{}(fh_raw={})".format(type(self).__name__, self.fh_raw)


class VLBIFileReaderBase(FileBase):
    """Adds header walking helpers shared by fixed-frame formats."""

    def image(self):
        """uint8 view of the whole file (memory mapped when possible)."""
        if getattr(self, '_image', None) is None:
            self._image = host_image(self.fh_raw)
        return self._image

    # -- masked byte-pattern search (base/base.py:181-368)
    @staticmethod
    def _as_bytes(value):
        """Pattern or mask given as header words, bytes, an int or ints
        (unsigned 32-bit, little endian), or a uint8 array -> uint8 array."""
        if isinstance(value, (bytes, bytearray)):
            return np.frombuffer(bytes(value), np.uint8)
        arr = np.asanyarray(value)
        if arr.dtype == np.uint8:
            return np.ascontiguousarray(arr).reshape(-1)
        return np.atleast_1d(arr).astype('<u4').view(np.uint8)

    def locate_frames(self, pattern, *, mask=None, frame_nbytes=None, offset=0,
                      forward=True, maximum=None, check=1, _here_first=False):
        """Frame starts near the current position, nearest first, at which the
        (masked) byte `pattern` sits `offset` bytes into the frame, whose frame
        fits in the file, and for which the pattern is also found `check` frames
        away wherever that position can be looked at.

        Same arguments and results as the reference's
        ``VLBIFileReaderBase.locate_frames`` (base/base.py:181-335): `pattern`
        may be a header (its invariant pattern and frame size are used), bytes,
        a uint8 / masked array, an int or ints (32-bit little-endian words);
        `maximum` defaults to two frames (minus one byte), or 10^6 bytes when no
        frame size is known.  The search is a vectorised compare over the
        memory-mapped file, leading byte first.
        """
        if hasattr(pattern, 'invariant_pattern'):
            if frame_nbytes is None:
                frame_nbytes = pattern.frame_nbytes
            pattern, mask = pattern.invariant_pattern()
        if isinstance(pattern, np.ma.MaskedArray):
            if mask is None:
                mask = np.where(np.ma.getmaskarray(pattern), 0, 0xff).astype(np.uint8)
            pattern = pattern.filled(0)
        pat = self._as_bytes(pattern)
        msk = None
        if mask is not None:
            msk = self._as_bytes(mask)
            used = np.nonzero(msk)[0]
            span = slice(used[0], used[-1] + 1)
            pat, msk = pat[span], msk[span]
            offset += span.start
        if maximum is None:
            maximum = (2 * frame_nbytes if frame_nbytes else 1000000) - 1
        if check is None or frame_nbytes is None:
            checks = np.zeros(0, dtype=np.int64)
        else:
            checks = np.atleast_1d(check).astype(np.int64) * frame_nbytes
        check_min = min(int(checks.min()) if checks.size else 0, 0)
        check_max = max(int(checks.max()) if checks.size else 0, 0)
        need = frame_nbytes if frame_nbytes is not None else offset + pat.size

        image = self.image()
        here = self.fh_raw.tell()
        seek_start = here if forward else here - maximum
        # bytes that may be looked at: from the earliest check position to the
        # end of the last candidate frame and its latest check pattern
        start = max(seek_start + offset + check_min, 0)
        stop = min(max(seek_start + maximum + 1 + check_max + need, start), len(image))
        size = min(maximum + 1 + check_max - check_min, stop - start - pat.size)
        if size <= 0:
            return []
        if _here_first:
            # (`find_header`: the current position is the nearest candidate in
            # either direction; when it qualifies -- a file of whole frames read
            # from its start, or backwards from its end -- two or three compares
            # of the pattern replace the search over two frames: Mark 4 open()
            # 1.65 -> 1.0 ms.  Same conditions as the filter below.)
            if not (max(seek_start, 0) <= here < min(seek_start + maximum + 1, stop - need + 1)):
                return []
            lo_ok, hi_ok = start, stop - offset - pat.size
            for c in [0] + [c for c in checks.tolist() if lo_ok <= here + c < hi_ok]:
                at = here + c + offset
                if at < 0 or at + pat.size > len(image):
                    return []
                piece = np.asarray(image[at:at + pat.size])
                if np.any(piece != pat) if msk is None else np.any((piece ^ pat) & msk):
                    return []
            return [here]
        data = np.asarray(image[start:start + size + pat.size])

        def matches_at(lo, hi):
            """Pattern positions (in `data`) within [lo, hi): first byte, then the rest."""
            first = data[lo:hi]
            hit = (first == pat[0]) if msk is None else (((first ^ pat[0]) & msk[0]) == 0)
            idx = np.nonzero(hit)[0] + lo
            for k in range(1, pat.size):
                if idx.size == 0:
                    break
                col = data[idx + k]
                ok = (col == pat[k]) if msk is None else (((col ^ pat[k]) & msk[k]) == 0)
                idx = idx[ok]
            return idx

        found = matches_at(0, size) + (start - offset)        # frame starts
        found_set = set(found.tolist())
        loc_lo = max(seek_start, 0)
        loc_hi = min(seek_start + maximum + 1, stop - need + 1)
        check_lo, check_hi = start, stop - offset - pat.size
        out = [int(loc) for loc in found.tolist()
               if loc_lo <= loc < loc_hi
               and all((int(loc + c) in found_set) for c in checks.tolist()
                       if check_lo <= loc + c < check_hi)]
        return out if forward else out[::-1]

    def find_header(self, *args, **kwargs):
        """Nearest header from the current position (arguments as for
        `locate_frames`); the file pointer is left at its start
        (base/base.py:337-368)."""
        for here_first in (True, False):
            for location in self.locate_frames(*args, _here_first=here_first, **kwargs):
                with self.temporary_offset(location):
                    try:
                        header = self.read_header()
                    except Exception:
                        continue
                if self._accept_header(header):
                    self.fh_raw.seek(location)
                    return header
        raise HeaderNotFoundError('could not locate a a nearby frame.')

    def _accept_header(self, header):
        return True

    # name used in `info.format`; constructor arguments a reader may lack
    _format = None

    def _info_needs(self):
        return {}

    def _info_extras(self, header0, offset0):
        return {}

    info = None         # (the descriptor below, set once the class exists)


class _FileReaderInfoProperty:
    """``reader.info``: a `FileReaderInfo` snapshot kept in the reader's ``__dict__``
    and made again when the reader is closed or one of the arguments it was
    constructed with is changed (``fh.nchan = 8``); it can be deleted (to have it made
    again) but not set (base/file_info.py:282-415, and the `info_item` machinery there)."""

    @staticmethod
    def _key(reader):
        cls = type(reader)
        names = cls.__dict__.get('_info_key_names')
        if names is None:
            import inspect
            names = tuple(n for n in inspect.signature(cls.__init__).parameters if n not in ('self', 'fh_raw'))
            cls._info_key_names = names
        try:
            closed = bool(reader.fh_raw.closed)
        except Exception:
            closed = False
        return (closed,) + tuple(str(getattr(reader, n, None)) for n in names)

    def __get__(self, reader, cls=None):
        if reader is None:
            return self
        from .info import FileReaderInfo
        cached = reader.__dict__.get('info')
        if cached is None or cached._made_for != self._key(reader):
            cached = FileReaderInfo(
                reader, reader._format or type(reader).__name__.replace('FileReader', '').lower(),
                reader._info_needs())
            cached._made_for = self._key(reader)        # (after: making it may settle e.g. Mark 4 `ntrack`)
            reader.__dict__['info'] = cached
        return cached

    def __set__(self, reader, value):
        raise AttributeError("can't set attribute 'info'")

    def __delete__(self, reader):
        reader.__dict__.pop('info', None)


VLBIFileReaderBase.info = _FileReaderInfoProperty()


def _to_host_array(data, out):
    """Device tensor -> the caller's NumPy `out`: pinned double-buffered copy
    for large contiguous destinations, plain copy otherwise."""
    from ..staging import download
    want = np.complex64 if data.is_complex() else np.float32
    if (isinstance(out, np.ndarray) and out.flags.c_contiguous and out.dtype == want
            and out.nbytes >= (32 << 20)):
        download(data, out)
    else:
        out[...] = data.cpu().numpy()


def _apply_squeeze(shape):
    return tuple(s for s in shape if s > 1)


class GPUStreamReaderBase(PackedBytesMixin):
    """Sample-stream view of a file whose frames decode on the GPU.

    Subclasses set up the geometry (`_setup`) and implement
    ``_scan_window(dbuf, nframes, first_set)`` -> scan records and
    ``_decode_window(dbuf, src, nsets, out_flat)``.
    """
    # window of file bytes staged per pipeline step
    window_bytes = 64 << 20
    # ... of a large read streamed from the host (128 and 256 MiB: 1-5 % slower, the
    # two short windows at the start grow with it; profiles/r04zs_pipeline_buffers.log)
    pipeline_window_bytes = 64 << 20

    def __init__(self, fh_raw, header0, *, sample_rate, samples_per_frame,
                 unsliced_shape, bps, complex_data, squeeze=True, subset=(),
                 fill_value=0., verify=True):
        self.fh_raw = fh_raw
        self._header0 = header0
        self._sample_rate = sample_rate
        self.samples_per_frame = samples_per_frame
        self._unsliced_shape = tuple(unsliced_shape)
        self._decode_shape = tuple(unsliced_shape)
        self.bps = bps
        self.complex_data = complex_data
        self._squeeze = bool(squeeze)
        self._subset = (() if subset is None
                        else subset if isinstance(subset, tuple) else (subset,))
        if self._subset:
            self.sample_shape               # (a subset that cannot index a sample is refused here, at open)
        self._fill_value = float(fill_value)
        self.verify = verify
        self.offset = 0
        self._pipeline = None
        self._closed = False
        # (open readers keep the output arena's memory; the last one to close
        # lets it go back to the device: placement.reader_closed)
        self._registered = True
        _placement.reader_opened()

    def _unregister(self):
        if self.__dict__.pop('_registered', False):
            _placement.reader_closed()

    def __del__(self):
        try:
            self._unregister()
        except Exception:
            pass

    # -- simple attributes
    @property
    def header0(self):
        return self._header0

    @property
    def squeeze(self):
        return self._squeeze

    @property
    def subset(self):
        return self._subset

    @property
    def fill_value(self):
        return self._fill_value

    @property
    def verify(self):
        return self._verify

    @verify.setter
    def verify(self, verify):
        self._verify = bool(verify) if verify != 'fix' else verify

    @property
    def sample_rate(self):
        """Complete samples per second (Hz, float)."""
        return self._sample_rate

    @property
    def closed(self):
        return self._closed

    def readable(self):
        """Whether the stream can be read and decoded (base/base.py:1012-1018)."""
        return bool(self.info.readable)

    def writable(self):
        """A stream reader cannot be written to (base/base.py:559-567 there)."""
        return False

    def __repr__(self):
        """The reference's layout (base/base.py:592-599)."""
        def attr(name):
            try:
                return getattr(self, name)
            except Exception:
                return None
        sub = 'subset={0}, '.format(self.subset) if getattr(self, 'subset', None) else ''
        return ("<{cls} name={name} offset={offset}\n"
                "    sample_rate={rate}, samples_per_frame={spf},\n"
                "    sample_shape={shape}, bps={bps},\n"
                "    {sub}start_time={start}>"
                .format(cls=type(self).__name__, name=getattr(self.fh_raw, 'name', None), offset=attr('offset'),
                        rate=attr('sample_rate'), spf=attr('samples_per_frame'), shape=attr('sample_shape'),
                        bps=attr('bps'), sub=sub, start=attr('start_time')))

    def seekable(self):
        return True

    @property
    def info(self):
        """`StreamReaderInfo` snapshot, renewed when `verify` changes or the
        stream is closed (base/file_info.py:417-571)."""
        from .info import StreamReaderInfo
        cached = self.__dict__.get('_info')
        if cached is None or cached.verify != self.verify or cached.closed != self.closed:
            cached = self.__dict__['_info'] = StreamReaderInfo(self)
        return cached

    def close(self):
        self._closed = True
        self._drop_windows()
        self._staged = self._sink = None
        self._have = []
        if self._pipeline is not None:
            self._pipeline.release()
            self._pipeline = None
        self.fh_raw.close()
        self._unregister()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- channel selection folded into the decode kernel
    _within_np = None       # int32 positions of a thread sample that are decoded (None: all)
    _within_dev = None

    @property
    def _within(self):
        """The selection as a device tensor (uploaded on first use, so that a
        reader can be opened -- for `info`, say -- without a GPU)."""
        if self._within_np is None:
            return None
        if self._within_dev is None:
            kernels.require_gpu()
            self._within_dev = torch.from_numpy(self._within_np).to('cuda')
        return self._within_dev

    def _plan_channel_select(self, subset, lead_in_sample=False, payload_nbytes=None):
        """If `subset` (what `_squeeze_and_subset` would apply to decoded
        frames) only picks CHANNELS -- the last axis of `_decode_shape` -- the
        same for every thread, have the decode kernel write just those
        (bb_decode_frames_select): the reference decodes whole frames and
        indexes afterwards (base/base.py:706-717, 957-969), which on the GPU
        would be one or two extra passes over the 16x expanded output.  The
        test is done by value: the subset is applied to arrays of channel and
        thread numbers, and folded only if the result is `(threads) x (channel
        list)` in that order.  Anything else keeps the general path.

        `lead_in_sample`: the leading axis is not a set of thread frames but
        lies inside every stored sample (DADA: polarisations); the positions
        then run over the whole (lead, channel) sample.

        `payload_nbytes`: bytes per frame and thread slot, when fixed.  The
        selecting kernel has limits (at most 4096 kept positions; a thread
        sample must fit whole rows into a work item of at most 16 tiles; the
        slots' staging must fit in LDS): the plan is checked against the
        library's own predicate (`kernels.select_supported`) and dropped --
        general path -- when the kernel would refuse it."""
        shape = tuple(self._decode_shape)
        if not subset or not shape or len(shape) > 2 or (len(shape) == 2 and shape[0] > 96):
            return
        nchan = shape[-1]
        lead = int(np.prod(shape[:-1])) if len(shape) > 1 else 1
        if (nchan * lead if lead_in_sample else nchan) & ((nchan * lead if lead_in_sample else nchan) - 1):
            return
        chan = np.broadcast_to(np.arange(nchan), shape)
        thread = np.broadcast_to(np.arange(lead).reshape(shape[:-1] + (1,)), shape)

        def view(a):
            a = np.ascontiguousarray(a)[np.newaxis]
            if self.squeeze:
                a = a.reshape(a.shape[:1] + _apply_squeeze(a.shape[1:]))
            return a[(slice(None),) + tuple(subset)]
        try:
            c, t = view(chan), view(thread)
        except Exception:
            return
        if c.shape[:1] != (1,) or c.size == 0 or c.size % lead:
            return
        c, t = c.reshape(-1), t.reshape(-1)
        m = c.size // lead
        picked = c[:m]
        if not (np.array_equal(t, np.repeat(np.arange(lead), m))
                and np.array_equal(c, np.tile(picked, lead))):
            return
        if m == nchan and np.array_equal(picked, np.arange(nchan)):
            return                                  # every channel, in order: nothing to fold
        ncomp = 2 if self.complex_data else 1
        if lead_in_sample:
            picked = (np.arange(lead)[:, None] * nchan + picked).reshape(-1)
        within = (picked[:, None] * ncomp + np.arange(ncomp)).reshape(-1).astype(np.int32)
        chunk = (nchan * lead if lead_in_sample else nchan) * ncomp
        if not kernels.select_supported(self.bps, chunk, 1 if lead_in_sample else lead, within.size,
                                        payload_nbytes):
            return
        self._within_np = within
        self._decode_shape = shape[:-1] + (m,)

    # -- shapes
    def _squeeze_and_subset(self, data):
        """Remove unit dimensions, then apply `subset`
        (base/base.py:706-717)."""
        if self._within_np is not None:
            # the kernel wrote exactly the selected samples, in the final order
            return data.reshape(data.shape[:1] + self.sample_shape)
        if self.squeeze:
            data = data.reshape(data.shape[:1] + _apply_squeeze(data.shape[1:]))
        if self.subset:
            data = data[(slice(None),) + self._torch_subset()]
        return data

    def _torch_subset(self):
        out = []
        for s in self.subset:
            if isinstance(s, (list, np.ndarray)):
                s = torch.as_tensor(np.asarray(s), device='cuda')
            out.append(s)
        return tuple(out)

    @property
    def sample_shape(self):
        """Shape of a complete sample, squeezed and subset as the stream is: a named
        tuple (``fh.sample_shape.nthread``) where the dimensions have names
        (`_sample_shape_fields`), as the reference's (base/base.py:460-485,719-775)."""
        # (made once per squeeze / subset setting: a named tuple CLASS is made for it,
        # which costs a hundred microseconds -- and read() asks for the shape)
        key = (self.squeeze, id(self.subset), tuple(self._unsliced_shape))
        cached = self.__dict__.get('_sample_shape_cached')
        if cached is None or cached[0] != key:
            from .utils import named_sample_shape
            fields = self._sample_shape_fields
            if callable(fields):
                fields = fields(len(self._unsliced_shape))
            cached = self._sample_shape_cached = (
                key, named_sample_shape(self._unsliced_shape, fields, self.squeeze, self.subset), self.subset)
        return cached[1]

    _sample_shape_fields = None     # names of the dimensions of a complete sample

    @property
    def shape(self):
        return (self._nsample,) + self.sample_shape

    @property
    def size(self):
        prod = 1
        for dim in self.shape:
            prod *= dim
        return prod

    @property
    def ndim(self):
        return len(self.shape)

    @property
    def dtype(self):
        return np.dtype(np.complex64 if self.complex_data else np.float32)

    # -- times (numpy datetime64[ns]; see DESIGN.md on astropy)
    @property
    def start_time(self):
        return self._start_time

    @property
    def stop_time(self):
        return self._time_at(self._nsample)

    @property
    def time(self):
        return self._time_at(self.offset)

    def _time_at(self, offset):
        ns = int(round(offset * 1e9 / self.sample_rate))
        return self._start_time + np.timedelta64(ns, 'ns')

    def tell(self, unit=None):
        """Current sample offset; ``unit='time'`` gives the time
        (base/base.py:552-576)."""
        if unit is None:
            return self.offset
        if unit == 'time':
            return self.time
        if unit == 's':
            return self.offset / self.sample_rate
        if hasattr(unit, 'to'):
            # a unit object of the caller's (astropy: ``fh.tell(u.ms)``): the
            # offset in that unit, as whatever number * unit makes (a Quantity)
            return (self.offset / self.sample_rate / float(unit.to('s'))) * unit
        raise ValueError("unit should be None, 'time', 's' or a unit of time")

    def seek(self, offset, whence=0):
        """Move the sample pointer (base/base.py:876-917).  `offset` may be an
        integer sample count, a ``numpy.timedelta64`` or a ``numpy.datetime64``,
        a float number of seconds -- or what the reference's callers pass: a
        `Time` (absolute; `whence` is ignored), a `TimeDelta` or a `Quantity`
        of time (base/quantities.py)."""
        try:
            offset = operator.index(offset)
        except Exception:
            if isinstance(offset, np.datetime64) or is_time_like(offset):
                offset = as_time(offset) - self.start_time
                whence = 0
            elif is_duration_like(offset):
                offset = as_timedelta(offset)
            if isinstance(offset, np.timedelta64):
                ns = offset / np.timedelta64(1, 'ns')
                offset = int(round(ns * self.sample_rate / 1e9))
            else:
                offset = int(round(float(offset) * self.sample_rate))
        origin = {0: 0, 'start': 0,
                  1: self.offset, 'current': self.offset,
                  2: self.shape[0], 'end': self.shape[0]}
        if whence not in origin:
            raise ValueError("whence must be 0 / 'start', 1 / 'current' or 2 / 'end', "
                             "not {!r}".format(whence))
        self.offset = origin[whence] + offset
        return self.offset

    # -- file image resident in HBM (resident.py)
    _staged = None

    def stage(self):
        """Upload the whole file once and keep it in HBM: every later
        ``read()`` decodes straight from there with one scan / index / decode
        launch per request (no staging windows, no PCIe).  A reader opened on
        a device tensor is resident from the start.  Returns self."""
        from ..staging import upload
        image = self._image()
        if getattr(image, 'device_tensor', None) is None and self._staged is None:
            kernels.require_gpu()
            self._staged = upload(image)[:len(image)]
        return self

    def unstage(self):
        """Drop the HBM copy made by `stage` (and what reads have kept)."""
        self._staged = None
        self._sink, self._have = None, []

    # -- windows that were staged once stay in HBM
    ramp_windows = True     # the first two staging windows of a large read are short (pipeline fill)
    keep_staged = None      # None: keep files of at most `keep_staged_max_bytes`; True / False: always / never
    keep_staged_max_bytes = 4 << 30
    _sink = None            # device tensor of the file's size (+ slack), filled window by window
    _have = ()              # merged byte intervals of `_sink` that hold file bytes

    def _sink_tensor(self):
        """The file-sized device tensor that large reads fill window by
        window, or None when windows are not kept.  Keeping them makes a second
        pass over the same bytes -- the corruption-tolerant re-read of
        verify='fix', a repeated read -- come from HBM instead of crossing PCIe
        again.  By default only files of at most `keep_staged_max_bytes` (4
        GiB) are kept; ``fh.keep_staged = True`` keeps any file that fits,
        ``False`` none; `unstage()` / `close()` release the copy."""
        if self._sink is not None:
            return self._sink
        keep = self.keep_staged
        n = len(self._image())
        if keep is None:
            # a stated cap, not a share of the GPU: the caller's outputs are 16x
            # the input and sized by the caller; larger files rotate
            # two window buffers, and a repair pass uploads what it needs again
            keep = n <= self.keep_staged_max_bytes
        if not keep or n == 0:
            return None
        try:
            self._sink = empty_output((n + 256,), dtype=torch.uint8, create=False)
        except torch.cuda.OutOfMemoryError:
            # no room for a copy of the file next to the caller's tensors:
            # rotate two window buffers as before
            self.keep_staged = False
            return None
        self._sink[n:] = 0
        self._have = []
        return self._sink

    def _mark_have(self, lo, hi):
        if hi <= lo:
            return
        merged = []
        for a, b in self._have:
            if b < lo or a > hi:
                merged.append((a, b))
            else:
                lo, hi = min(lo, a), max(hi, b)
        merged.append((lo, hi))
        self._have = sorted(merged)

    def _has_bytes(self, lo, hi):
        return hi <= lo or any(a <= lo and hi <= b for a, b in self._have)

    def _whole_file_in_hbm(self):
        """Device tensor holding the complete file: the explicit or implicit
        resident image, or the kept windows completed by uploading whatever
        has not been staged yet (each byte crosses PCIe once)."""
        from ..staging import upload
        dev = self._resident_bytes()
        image = self._image()
        n = len(image)
        if dev is not None:
            if dev.data_ptr() % 16:             # the search kernels load 16 bytes per lane
                dev = self._staged = dev.clone()
            return dev
        sink = self._sink_tensor()
        if sink is None:
            self._staged = upload(image)[:n]
            return self._staged
        pos = 0
        for a, b in list(self._have) + [(n, n)]:
            if a > pos:
                sink[pos:a].copy_(upload(image[pos:a])[:a - pos])
            pos = max(pos, b)
        self._have = [(0, n)]
        self._staged = sink[:n]
        return self._staged

    def _resident_bytes(self):
        """Device tensor holding the file bytes, or None."""
        if self._staged is not None:
            return self._staged
        return getattr(self._image(), 'device_tensor', None)

    @staticmethod
    def _device_window(dev, lo, hi, align=8):
        """``dev[lo:hi]`` for the kernels: a view when `lo` is aligned the way
        the library wants its buffers, an aligned copy otherwise (files with
        leading junk bytes)."""
        part = dev[lo:hi]
        if part.numel() == 0:
            # nothing of the file lies here (bytes went missing): hand the
            # library a few zero bytes -- too few to hold a frame -- rather
            # than an empty tensor, whose data pointer is null
            return torch.zeros(64, dtype=torch.uint8, device=dev.device)
        if part.data_ptr() % align:
            part = part.clone()
        return part

    # -- the hot path
    def _raw_follows(self):
        """Leave the raw file pointer after the last frame (set) a read touched, where
        the reference's frame-by-frame reads leave it (base/base.py:971-1010 there): its
        callers interleave ``fh_raw.tell()`` / raw reads with stream reads.  (The seek of
        the file underneath, looked up once: this runs in every small read.)"""
        seek = self.__dict__.get('_raw_seek')
        if seek is None:
            raw = self.fh_raw
            seek = self._raw_seek = getattr(raw, 'fh_raw', raw).seek
        seek(self._file_offset0 + ((self.offset - 1) // self.samples_per_frame + 1) * self._set_nbytes)

    # ``fh.sample_dtype = torch.float16`` (or ``torch.bfloat16``; None = float32, as always):
    # ``read()`` without `out` returns samples of that element type -- ``torch.complex32`` for a
    # complex stream with float16 -- and the decoded read-ahead window is kept in it.  Where
    # the library has 16-bit decode kernels for the format (`_half_geometry`) the decode
    # writes the type itself (half the stores, no float32 copy anywhere); elsewhere the
    # samples are decoded to float32 and converted.  Same values either way: the float32
    # sample rounded once to nearest even.  ``fh.dtype`` keeps naming the stream's native
    # NumPy dtype, as the reference's does; readers with `host_results` ignore the setting.
    _sample_dtype = None

    @property
    def sample_dtype(self):
        return self._sample_dtype

    @sample_dtype.setter
    def sample_dtype(self, dtype):
        if dtype is not None and isinstance(dtype, str):
            dtype = getattr(torch, dtype, dtype)
        if dtype == torch.float32:
            dtype = None
        if dtype not in (None, torch.float16, torch.bfloat16):
            raise ValueError("sample_dtype is None (float32), torch.float16 or torch.bfloat16, not {!r}".format(dtype))
        self._refuse_complex_bfloat16(dtype)
        if dtype != self._sample_dtype:
            self._decoded = self._decoded_host = None       # (a decoded window is of one type)
        self._sample_dtype = dtype

    def _refuse_complex_bfloat16(self, dtype):
        if dtype == torch.bfloat16 and self.complex_data:
            raise ValueError("this stream is complex and torch has no complex bfloat16 type: "
                             "use torch.float16 (samples come as torch.complex32) or float32")

    @staticmethod
    def _out_elem(out):
        """Element type a caller's `out` asks the decode for (NumPy arrays: float32)."""
        if isinstance(out, torch.Tensor):
            if out.dtype in (torch.float16, torch.complex32):
                return torch.float16
            if out.dtype == torch.bfloat16:
                return torch.bfloat16
        return torch.float32

    def _half_geometry(self):
        """``(coder, bps, chunk, nslot, payload_nbytes)`` of the decode launches of this
        reader when they go through bb_decode_frames or a window call built on it, else
        None: formats whose kernels write float32 only (Mark 4, the int8 transposes,
        float32 DADA) convert afterwards."""
        return None

    def _half_direct(self, elem):
        """May the decode write `elem` (torch.float16 / torch.bfloat16) itself?  Asks the
        library (bb_decode_out_check); never with a channel subset folded into the
        decode (the selecting kernels write float32)."""
        if self._within_np is not None:
            return False
        geom = self._half_geometry()
        key = (geom, elem)
        cached = self.__dict__.get('_half_direct_cached')
        if cached is None or cached[0] != key:
            ok = geom is not None and kernels.out_supported(*geom, elem)
            cached = self._half_direct_cached = (key, ok)
        return cached[1]

    def read(self, count=None, out=None):
        """Read and decode `count` complete samples -> device tensor of shape
        ``(count,) + sample_shape`` (base/base.py:919-969)."""
        if self.closed:
            raise ValueError("I/O operation on closed stream.")
        if isinstance(out, torch.Tensor):
            self._refuse_complex_bfloat16(out.dtype)
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

        if self._pending_warning:
            warnings.warn(self._pending_warning)
            self._pending_warning = None
        host = self.host_results and out is None
        # (a decoded window is of ONE element type: it serves results of that type only --
        # float32 samples are never made from a window that was rounded to 16 bits)
        ahead = self._from_decoded_ahead(count, host) \
            if count and (out is None or self._out_elem(out) == self._elem_dtype()) else None
        if ahead is not None:
            self.offset += count
            self._seq_end = self.offset
            self._raw_follows()
            if out is None:
                if host and isinstance(ahead, torch.Tensor):
                    from ..staging import download_new
                    return download_new(ahead)
                return ahead
            if isinstance(out, torch.Tensor):
                out.copy_(ahead)
            else:
                _to_host_array(ahead, out)
            return out
        self._asked = (self.offset, count)
        data, direct = self._fill_request(out, count)
        if not self._resolve_checks():
            # verify='fix': frames are missing or out of place.  Build the
            # corruption-tolerant index (byte-granular header search) and
            # decode again through it.
            self._relocate()
            self.decode_ahead = False       # (warnings belong to the read that meets a hole)
            if self.offset + count > self.shape[0]:
                raise EOFError("cannot read from beyond end of input.")
            data, direct = self._fill_request(out, count)
        self.offset += count
        self._seq_end = self.offset
        if count:
            self._raw_follows()
        if direct:
            return out
        data = self._squeeze_and_subset(data)
        if out is None:
            if host:
                from ..staging import download_new
                return download_new(data)
            return data
        if isinstance(out, torch.Tensor):
            out.copy_(data)
        else:
            _to_host_array(data, out)
        return out

    # what `_relocate` leaves on a reader (`packed._relocated_meanwhile` sets it aside and puts it back)
    _relocation_state = ('_resident', '_nsample_found', '_located', '_relocated', '_damage', '_slips',
                         '_before_trouble')

    # ``host_results = True``: ``read()`` without `out` returns NEW NumPy arrays, as the
    # reference does (what the ``baseband.io`` plugin modules switch on): arrays on pinned
    # memory filled by the DMA engine (`staging.download_new`), and -- in loops of small
    # sequential reads -- pieces cut out of a host copy of the decoded window.
    host_results = False
    host_window_copy_below = 256 << 10  # results up to this size come out of the window's host copy
    _decoded_host = None                # (the window tensor it mirrors, NumPy array on pinned memory)

    # -- decoded read-ahead for loops of small sequential reads
    decode_ahead = True                 # set False to decode exactly what every read() asks for
    decode_ahead_bytes = 64 << 20       # decoded bytes per read-ahead window at most
    _decoded = None                     # (first sample, end sample, decoded tensor) of the window
    _seq_end = None                     # where the previous read() ended
    _seq_run = 0                        # consecutive reads that continued the one before
    _ahead_sets = 16                    # frame sets in the next window (x4 per refill)

    def _from_decoded_ahead(self, count, host=False):
        """Frame-at-a-time loops (the reference's own way through a file, and
        many user scripts) cost a scan, an index and a decode launch per
        ``read()`` -- tens of microseconds of host time for a microsecond of
        GPU work.  When the third read in a row continues exactly where the
        one before ended, a window of following frame sets is decoded at once
        (growing x4 per refill up to `decode_ahead_bytes` of output) and
        sequential reads inside it are served as views of that tensor.  Every
        sample of a window is handed out at most once, and any read that is
        not a continuation (a seek) drops the window.  If verification finds a
        problem anywhere in a window the reader goes back to decoding exactly
        what each read asks for, for good: errors, warnings and repairs then
        happen at the read that meets the problem, as without read-ahead.
        Returns the samples, or None for the ordinary path."""
        off = self.offset
        if not self.decode_ahead or self._seq_end != off:
            self._seq_run, self._decoded, self._ahead_sets = 0, None, 16
            return None
        self._seq_run += 1
        d = self._decoded
        if d is not None and d[0] <= off and off + count <= d[1]:
            return self._ahead_result(d[2][off - d[0]:off - d[0] + count], off - d[0], host)
        self._decoded = None
        if self._seq_run < 2:
            return None
        spf = self.samples_per_frame
        ncomp = 2 if self.complex_data else 1
        set_bytes = spf * int(np.prod(self._decode_shape)) * ncomp * (4 if self._elem_dtype() == torch.float32 else 2)
        max_sets = max(1, self.decode_ahead_bytes // max(1, set_bytes))
        first = off // spf
        need = -(-(off + count) // spf) - first
        if need * 4 > max_sets:
            return None                 # not a small request: the ordinary path is the fast one
        last = min(first + max(need, min(self._ahead_sets, max_sets)), -(-self.shape[0] // spf))
        if last - first < need:
            return None
        try:
            data = self._read_sets(first, last)
            ok = self._resolve_checks(quiet=True)
        except (EOFError, ValueError, HeaderNotFoundError):
            # something is wrong with the FILE inside the window (bytes
            # missing, a header that is not one): the ordinary path meets it
            # at the read it belongs to and raises or repairs there
            ok = False
        except torch.cuda.OutOfMemoryError:
            # no room for a speculative window next to the caller's tensors:
            # the request itself needs far less, so serve it the ordinary way
            warnings.warn("decoded read-ahead switched off: out of device memory for a "
                          "window of {} frame sets".format(last - first))
            ok = False
        # (library / HIP errors and programming errors are not caught)
        if not ok:
            self.decode_ahead = False
            self._reset_checks()
            return None
        self._ahead_sets = min(max_sets, self._ahead_sets * 4)
        data = self._squeeze_and_subset(data)
        self._decoded = (first * spf, min(last * spf, self.shape[0]), data)
        return self._ahead_result(data[off - first * spf:off - first * spf + count], off - first * spf, host)

    decode_ahead_copy_below = 1 << 20   # results smaller than this are copies, not views of the window

    def _ahead_result(self, part, lo=0, host=False):
        """What a read served from the decoded window returns.  The reference
        hands out fresh arrays (base/base.py:919-969); a VIEW of the window
        would keep all of it (up to `decode_ahead_bytes`) alive for as long as
        the caller keeps a few samples, so small results are copied out --
        larger ones, where the copy would cost as much as the decode, stay
        views (documented; `decode_ahead_copy_below = 0` turns copying off)."""
        nbytes = part.numel() * part.element_size()
        if host and nbytes <= self.host_window_copy_below:
            # a frame-at-a-time loop that wants NumPy arrays: one device-to-host copy per
            # WINDOW (1.2 ms for 64 MiB), then every read is a memcpy of its piece -- a
            # synchronous copy per read cost 25 us of the 38 us a read(32000) took
            window = self._decoded[2]
            mirror = self._decoded_host
            if mirror is None or mirror[0] is not window:
                from ..staging import download_new
                mirror = self._decoded_host = (window, download_new(window))
            return mirror[1][lo:lo + part.shape[0]].copy()
        if nbytes < self.decode_ahead_copy_below:
            return part.clone()
        return part

    _scan_side = None       # side stream for the scan of the window being processed (resident bytes only)
    _last_scan_side = None  # ... of the window processed last (where its verdict is fetched)
    _scan_stream = None
    _scan_ready_for = None

    def _prepare_window_state(self, device):
        """Device state a window call needs besides its scratch (the verdict
        counter; VDIF: the thread-slot map): made here, ahead of the call."""
        if self.verify:
            self._verdict_targets()

    def _scan_stream_for(self, resident):
        """The side stream the scan / index / verification launches of requests
        on `resident` go to (kernels._FrameWindow): their verdict -- all that
        read() waits for -- then does not queue behind the previous request's
        decode on the caller's stream.  The stream first waits for everything
        that is queued on the caller's stream NOW (whatever produced the
        bytes); bytes changed later, between two reads, are the caller's to
        order."""
        dev = resident.device
        if self._scan_stream is None:
            # ONE stream per device for all readers (streams share a few hardware queues in
            # creation order: a stream per reader made the early verdict a matter of luck,
            # profiles/r05j_back_to_back.log), high priority: the few microseconds of a scan
            # should not wait for a free slot behind a decode launch that fills the device
            # (normal priority: 0.954 against 0.837 ms per read of 2^15 frames back to back)
            with _scan_streams_lock:
                st = _scan_streams.get(dev.index)
                if st is None:
                    st = _scan_streams[dev.index] = torch.cuda.Stream(
                        device=dev, priority=int(os.environ.get('BB_SIDE_SCAN_PRIORITY', '-1')))
            self._scan_stream = st
        key = (resident.data_ptr(), resident.numel(), None if self._nbad is None else self._nbad.data_ptr(),
               self._side_state_key())
        if self._scan_ready_for != key:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(dev))
            self._scan_stream.wait_event(ev)
            self._scan_ready_for = key
        return self._scan_stream

    def _side_state_key(self):
        """Identity of further device state the side stream reads (subclasses)."""
        return None

    def _zero_nbad(self):
        if self._nbad is not None:
            if self._scan_stream is not None:           # (verification launches on the side stream add to it)
                self._scan_stream.synchronize()
            self._nbad.zero_()
            if self._scan_stream is not None:
                torch.cuda.current_stream(self._nbad.device).synchronize()

    def _reset_checks(self):
        """Forget the verification state of windows that were processed for a
        read that did not complete (or a read-ahead that was abandoned): the
        next read starts clean -- host counters AND the device counter."""
        self._nmissing, self._checked, self._check_recs = 0, False, 0
        self._zero_nbad()

    def _fill_request(self, out, count):
        """Decode samples [offset, offset + count).  Returns ``(data, direct)``:
        with a suitable device tensor as `out` the whole frame sets inside the
        request are decoded in place (no second pass over the 16x larger
        output) and only a partial first / last frame set goes through a
        temporary -- `direct` is True and `out` is complete; otherwise `data`
        holds the samples before squeeze / subset."""
        spf = self.samples_per_frame
        first, off0 = divmod(self.offset, spf)
        stop = self.offset + count
        last = -(-stop // spf) if count else first
        flat = self._direct_target(out)
        body0, body1 = first + (1 if off0 else 0), stop // spf
        if flat is not None and count and body1 > body0:
            row = flat.numel() // count
            o0 = body0 * spf - self.offset
            self._read_sets(body0, body1, flat[o0 * row:(o0 + (body1 - body0) * spf) * row])
            if off0:
                head = self._squeeze_and_subset(self._read_sets_as(first, body0, flat.dtype))
                out[:o0] = head[off0:]
            if body1 < last:
                ntail = stop - body1 * spf
                tail = self._squeeze_and_subset(self._read_sets_as(body1, last, flat.dtype))
                out[count - ntail:] = tail[:ntail]
            return out, True
        data = self._read_sets(first, last) if out is None else self._read_sets_as(first, last, self._out_elem(out))
        return data[off0:off0 + count], False

    def _direct_target(self, out):
        """Flat float32 (float16, bfloat16) view of `out` when the decode may write
        straight into it: a contiguous device tensor of the stream's dtype -- or of
        one of its 16-bit forms: float16 / bfloat16, complex32 for complex streams
        -- and no subset (squeezing only drops unit dimensions)."""
        if (not isinstance(out, torch.Tensor) or not out.is_cuda or not out.is_contiguous()
                or out.dtype not in ((torch.complex64, torch.complex32) if self.complex_data
                                     else (torch.float32, torch.float16, torch.bfloat16))):
            return None
        if self._within_np is None and (self.subset or getattr(self, '_frameset_subset', None)
                                     or tuple(self._decode_shape) != tuple(self._unsliced_shape)):
            return None
        flat = torch.view_as_real(out) if self.complex_data else out
        return flat.reshape(-1)

    def _elem_dtype(self):
        """Element type of what ``read()`` returns without `out`."""
        if self._sample_dtype is None or self.host_results:
            return torch.float32
        return self._sample_dtype

    _want_elem = None       # element type of the `_read_sets` call in progress, when not the default's

    def _read_sets_as(self, first, last, elem):
        """`_read_sets` into a new tensor of element type `elem`."""
        self._want_elem = elem
        try:
            return self._read_sets(first, last)
        finally:
            self._want_elem = None

    def _read_sets(self, first, last, into=None):
        """Decode frame sets [first, last) -> tensor (nsets*spf, *unsliced);
        `into` is an optional flat device tensor to decode into.  The element
        type is that of `into`, else what `_read_sets_as` asks for, else
        `sample_dtype`.  A 16-bit type the format's kernels do not write
        (`_half_direct`) is decoded to float32 and converted."""
        elem = into.dtype if into is not None else (self._want_elem or self._elem_dtype())
        if elem == torch.float32 or self._half_direct(elem):
            return self._decode_sets(first, last, into, elem)
        data = self._decode_sets(first, last, None, torch.float32)
        flat = (torch.view_as_real(data) if self.complex_data else data).reshape(-1)
        if into is not None:
            into.copy_(flat)
            flat = into
        else:
            flat = flat.to(elem)
        if self.complex_data:
            flat = torch.view_as_complex(flat.view(-1, 2))
        return flat.reshape(data.shape)

    def _decode_sets(self, first, last, into, elem):
        """`_read_sets` in an element type the decode writes itself."""
        kernels.require_gpu()
        self._last_scan_side = None
        nsets = last - first
        spf = self.samples_per_frame
        ncomp = 2 if self.complex_data else 1
        row = int(np.prod(self._decode_shape)) * ncomp
        flat = into if into is not None else kernels.empty_decoded(nsets * spf * row, dtype=elem)
        set_nbytes = self._set_nbytes
        resident = self._resident_bytes() if nsets else None
        if resident is None and nsets and self._have:
            # bytes that earlier reads left in HBM serve this one too
            lo_ = self._file_offset0 + first * set_nbytes
            hi_ = min(self._file_offset0 + (last + (1 if self.verify else 0)) * set_nbytes,
                      len(self._image()))
            if self._has_bytes(min(lo_, hi_), hi_):
                resident = self._sink[:len(self._image())]
        if resident is not None:
            # the file is in HBM already: ONE scan -> index -> decode over the
            # whole request, straight from where the bytes lie
            lo = min(self._file_offset0 + first * set_nbytes, resident.numel())
            look = 1 if self.verify else 0
            hi = max(lo, min(self._file_offset0 + (last + look) * set_nbytes, resident.numel()))
            win = self._device_window(resident, lo, hi)
            # (requests large enough for the side-stream verdict of `_resolve_checks`, bytes read in
            # place: the scan of this request need not queue behind the decode of the one before)
            if (self.verify and _SIDE_SCAN and nsets * set_nbytes >= (16 << 20)
                    and win.data_ptr() == resident.data_ptr() + lo):
                # (what the side stream's launches read or add to must exist -- and be
                # initialised on the caller's stream -- BEFORE the side stream's first
                # wait for that stream: `_scan_stream_for`)
                self._prepare_window_state(win.device)
                self._scan_side = self._scan_stream_for(resident)
            try:
                self._process_window(win, first, last, flat)
            except Exception:
                self._reset_checks()
                raise
            finally:
                self._last_scan_side, self._scan_side = self._scan_side, None
        elif nsets and nsets * set_nbytes * 8 <= self.window_bytes:
            # small request: serve it from the read-ahead window kept in HBM
            self._read_small(first, last, flat, spf * row)
        elif nsets:
            image = self._image()
            per_win = max(1, self.pipeline_window_bytes // set_nbytes)
            if self._pipeline is None:
                self._pipeline = WindowPipeline(image, (per_win + 1) * set_nbytes)
            sink = self._sink_tensor()
            ranges, spans = [], []
            # the first two windows are short (1/16 and 1/4 of a window): nothing
            # overlaps the first host copy and the first H2D, so they should be
            # small; from the third window on the pipeline runs at the link's rate
            # (profiles/r03h_prof_pipeline_windows.log -> r03i_)
            starts, s = [], first
            for size in ((max(1, per_win // 16), max(1, per_win // 4)) if self.ramp_windows else ()):
                if s < last:
                    starts.append(s)
                    s += size
            starts.extend(range(s, last, per_win))
            for i, s in enumerate(starts):
                e = min(last, starts[i + 1] if i + 1 < len(starts) else s + per_win)
                lo = min(self._file_offset0 + s * set_nbytes, len(image))
                # when verifying, the frame set after the last one requested
                # travels along: a frame only counts as good if the header
                # behind it is in place too (base/base.py:1083-1125)
                look = 1 if (self.verify and e == last) else 0
                # (a file with bytes missing ends before its last headers say:
                # such windows are short or empty, never negative)
                hi = max(lo, min(self._file_offset0 + (e + look) * set_nbytes, len(image)))
                ranges.append((lo, hi))
                spans.append((s, e))

            def process(dbuf, i):
                s, e = spans[i]
                o = flat[(s - first) * spf * row:(e - first) * spf * row]
                # (a window kept in place inside the file-sized buffer starts
                # wherever the file says: aligned copy if the library needs one)
                self._process_window(self._device_window(dbuf, 0, dbuf.numel()), s, e, o)

            try:
                self._pipeline.run(ranges, process, sink=sink)
            except Exception:
                # do not leave half a read's verification state for the next one
                self._reset_checks()
                raise
            if sink is not None:
                for lo, hi in ranges:
                    self._mark_have(lo, hi)
        if self.complex_data:
            flat = torch.view_as_complex(flat.view(-1, 2))
        return flat.reshape((nsets * spf,) + tuple(self._decode_shape))

    _ahead = None       # (first set, end set, device bytes) of the read-ahead window
    _ahead_bytes0 = 256 << 10           # first read-ahead window; grows while reads are sequential
    _ahead_bytes = 256 << 10

    def _read_small(self, first, last, flat, set_floats):
        """Requests much smaller than a staging window (frame-at-a-time loops
        like the reference's own): one whole window starting at the request is
        staged and kept in HBM; following requests inside it only launch
        kernels -- no host copy, no H2D."""
        from ..staging import upload
        set_nbytes = self._set_nbytes
        image = self._image()
        total = (len(image) - self._file_offset0) // set_nbytes     # whole sets in the file
        look = 1 if self.verify else 0
        need_end = min(last + look, total)
        ahead = self._ahead
        if ahead is None or first < ahead[0] or need_end > ahead[1]:
            # adaptive read-ahead: a request that continues where the window
            # ended (a sequential loop) quadruples the next window, up to
            # `window_bytes`; anything else (random access) starts small again,
            # so that seeking around costs tens of microseconds, not the
            # milliseconds of staging 64 MiB for one frame
            if ahead is not None and ahead[0] <= first <= ahead[1]:
                self._ahead_bytes = min(self.window_bytes, 4 * self._ahead_bytes)
            else:
                self._ahead_bytes = self._ahead_bytes0
            # (staging the NEXT window on a worker thread meanwhile, as the block
            # formats do for whole blocks, was tried here and lost: a loop of
            # read(3200000) on a 2 GiB file 38-44 -> 64-72 us per call, the
            # worker and the loop fight over the same host cores and link --
            # profiles/r02aw_bench_small_reads_prefetch.jsonl)
            per_win = max(last - first + look, self._ahead_bytes // set_nbytes)
            end = min(total, first + per_win)
            lo = self._file_offset0 + first * set_nbytes
            hi = max(lo, self._file_offset0 + end * set_nbytes)
            dev = upload(image[lo:hi])
            ahead = self._ahead = (first, max(end, first), dev)
        s0, s1, dev = ahead
        a = (first - s0) * set_nbytes
        b = max(a, (min(need_end, s1) - s0) * set_nbytes)
        self._process_window(self._device_window(dev, a, b), first, last, flat)

    def _drop_windows(self):
        """Forget the read-ahead windows."""
        self._ahead = self._decoded = self._decoded_host = None

    _nbad = None        # device counter the verification kernel adds to
    _nmissing = 0       # frames a window should have held but the file did not
    _checked = False

    def _note_checked(self, nrecs, missing=0):
        """Book the verification a window call launched (kernels.VDIFWindow,
        Mark5BWindow, Mark4Window: the library records the event behind it; the
        counter is read once per read() in `_resolve_checks`)."""
        self._check_recs += int(nrecs)
        self._nmissing += int(missing)
        self._checked = True

    def _verdict_targets(self):
        """(device counter, raw handle of the event to record behind the
        verification launch) for a fused window call."""
        if self._nbad is None:
            self._nbad = torch.zeros(1, dtype=torch.int32, device='cuda')
        if self._check_event is None:
            self._check_event = torch.cuda.Event()
            self._check_event.record()              # (creates the HIP event: the handle exists from here on)
        return self._nbad, self._check_event.cuda_event

    _check_recs = 0         # scan records queued for verification since the last verdict
    _check_event = None     # recorded behind the last verification launch
    _check_stream = None    # side stream the verdict is fetched on
    _nbad_host = None       # pinned int32[1]

    def _resolve_checks(self, quiet=False):
        """Look at the verification counters the windows left on the device
        (one host sync per read, none when verify is False).  Returns False
        when verify='fix' found a problem that `_relocate` can repair; with
        `quiet`, False for any problem, without warning or raising."""
        checked, self._checked = self._checked, False
        if not self.verify or not checked:
            return True
        # The verdict is fetched on a side stream that waits for the verification
        # launches only -- they are queued ahead of the window's decode -- so a
        # read() returns (or raises) after the scan of its frames, not after the
        # decode: 0.12 instead of 0.8 ms for 2^15 cfg2 frames, and the host side
        # of the next read() overlaps this one's decode.  The result is ordered on
        # the caller's stream as any torch result is.
        # (Small reads -- a few frames, microseconds of decode -- take the plain
        # readback on the current stream: the side stream's bookkeeping costs 15 us.)
        nrecs, self._check_recs = self._check_recs, 0
        if nrecs < 2048:
            nbad = int(self._nbad.item()) + self._nmissing
        else:
            if self._check_stream is None:
                self._check_stream = torch.cuda.Stream(device=self._nbad.device)
                self._nbad_host = torch.zeros(1, dtype=torch.int32, pin_memory=True)
            # (one library call: stream-wait-event, 4-byte copy, stream synchronise --
            # torch's stream context manager alone cost 15 us)
            # When the verification ran on the scan stream (`_scan_stream_for`) the copy is queued
            # right behind it THERE: no third stream, no event to wait for.
            on_scan = self._last_scan_side
            kernels.fetch_counter(self._nbad, self._nbad_host, None if on_scan is not None else self._check_event,
                                  on_scan if on_scan is not None else self._check_stream)
            nbad = int(self._nbad_host[0]) + self._nmissing
        self._nmissing = 0
        if nbad:
            self._zero_nbad()
            if quiet:
                return False
            msg = ("problem loading frame: {} frame header(s) failed verification "
                   "(bad sync/invariants or unexpected time index)".format(nbad))
            if self.verify == 'fix':
                if self._can_relocate and not self._relocated:
                    # (no warning here: the read is done again through the index of
                    # located frames, which names every frame it cannot supply)
                    return False
                warnings.warn(msg + "; affected samples were set to fill_value.")
            else:
                err = self._verification_error(msg)
                if err is None and self._can_relocate:
                    # (headers are off the fixed stride, yet the reference's loop would find every
                    # frame this reader asks for: read through the index of located frames)
                    return False
                raise err if err is not None else ValueError("wrong frame number. " + msg)
        return True

    def _verification_error(self, msg):
        """The exception a read under ``verify=True`` ends with when headers failed their checks."""
        return ValueError("wrong frame number. " + msg)

    _asked = None               # (first sample, count) of the read() in progress

    _can_relocate = False
    _relocated = False
    _pending_warning = None

    # After `_relocate`: which frame sets have frames missing, so that every read that
    # meets one says so, as the reference does at each load of such a set
    # (base/base.py:1127-1219, vdif/base.py:655-730) -- and `info`'s look at the last
    # frame reports 'fixable gaps' with the same sentence.
    _damage = None              # (sorted set numbers, their rows of "slot missing")
    damage_warnings_per_read = 16

    def _note_damage(self, src, nslot=1):
        """Called at the end of `_relocate`: which sets lack frames, and by how many bytes
        the complete ones are displaced from the fixed stride."""
        gone = (src.reshape(-1, nslot) < 0).cpu().numpy()
        sets = np.nonzero(gone.any(axis=1))[0]
        self._damage = (sets, gone[sets])
        starts = self._located_starts()
        n = min(len(starts), len(gone))
        whole = (starts[:n] >= 0) & ~gone[:n].any(axis=1)
        slip = starts[:n] - self._file_offset0 - np.arange(n, dtype=np.int64) * self._set_nbytes
        self._slips = (whole, slip, np.zeros(n, bool))

    def _damage_message(self, k, missing):
        return "problem loading frame {}. The frame seems to be missing.".format(k)

    def _slip_message(self, k, nbytes):
        return "problem loading frame {}. Stream off by {} bytes.".format(k, nbytes)

    _slips = None               # (set is complete, its displacement in bytes, displacement known to the caller)

    def _warn_damage(self, first, last):
        """Warnings of one read of sets [first, last) through the index of located frames: one
        for every set with frames missing, and -- as the reference, which learns where frames
        lie as it meets them (base/base.py:1127-1219, the table `_raw_offsets`) -- one where a
        complete set is not where the sets read so far put it: at the first set of the read
        whatever the difference, further on when it is not a whole number of frames (bytes
        went missing; whole missing frames are accounted for by the message of their set)."""
        if self._damage is None or self.verify is True:     # (a strict reader raises or is silent)
            return
        notes = []
        sets, rows = self._damage
        lo, hi = np.searchsorted(sets, [first, last])
        for j in range(lo, hi):
            notes.append((int(sets[j]), self._damage_message(int(sets[j]), rows[j])))
            if len(notes) > self.damage_warnings_per_read:
                break
        if self._slips is not None:
            whole, slip, known = self._slips
            ks = first + np.nonzero(whole[first:last])[0]
            if len(ks):
                before = np.nonzero(known[:ks[0]])[0]
                base = slip[before[-1]] if len(before) else 0
                step = np.diff(np.concatenate([[base], slip[ks]]))
                frame_nbytes = getattr(self, '_frame_nbytes', None) or self._set_nbytes
                told = (step != 0) & ((ks == first) | (step % frame_nbytes != 0)) & ~known[ks]
                for j in np.nonzero(told)[0][:self.damage_warnings_per_read]:
                    notes.append((int(ks[j]), self._slip_message(int(ks[j]), -int(step[j]))))     # (expected - found)
                known[ks] = True
        notes.sort()
        for _, text in notes[:self.damage_warnings_per_read]:
            warnings.warn(text)
        if len(notes) > self.damage_warnings_per_read or hi - lo > self.damage_warnings_per_read:
            warnings.warn("... and more frames of this read with data missing; set to invalid.")

    # The last header of a stream and the number of samples that follows from it are
    # looked up when first asked for, as the reference's lazy properties are
    # (base/base.py:827-841,1060-1077): a damaged file opens, and raises
    # HeaderNotFoundError where its length is needed.  Formats give
    # `_find_last_header()` and `_count_samples()`, or assign `_nsample` outright.
    @property
    def _last_header(self):
        found = self.__dict__.get('_last_header_found')
        if found is None:
            found = self._last_header_found = self._find_last_header()
        return found

    @property
    def _nsample(self):
        n = self.__dict__.get('_nsample_found')
        if n is None:
            n = self._nsample_found = self._count_samples()
        return n

    @_nsample.setter
    def _nsample(self, value):
        self._nsample_found = value

    def _find_last_header(self):
        raise NotImplementedError

    def _count_samples(self):
        raise NotImplementedError

    def _relocate(self):
        raise NotImplementedError

    _located = None             # (frame starts, records) of `_relocate`'s search

    @property
    def _raw_offsets(self):
        """Where the frames (VDIF: frame sets) of the file start, as the
        reference's table of the same name (base/base.py:1064,1081; written
        by `_bad_frame`, base/base.py:1189, vdif/base.py:615,729): a
        `RawOffsets` whose ``[k]`` is the file position of frame (set) `k`.
        Before `_relocate` that is the fixed stride from the first frame;
        after it, the positions of the frames the search found, folded into
        steps -- a frame set counts from its earliest frame that was found,
        frames of which nothing was found take the slip of the one before."""
        from .offsets import RawOffsets
        from .. import _lib
        if self._located is None:
            table = RawOffsets(frame_nbytes=self._set_nbytes)
            if self._file_offset0:
                table[0] = self._file_offset0
            return table
        start = self._located_starts()
        return RawOffsets.from_index(start, self._set_nbytes, known=start >= 0)

    def _located_starts(self):
        """File position of the earliest located frame of every frame (set), -1 where none was found."""
        from .. import _lib
        offs, recs = self._located
        nsets = self._nsample // self.samples_per_frame
        when = recs[:, 2].to(torch.int64)
        ok = (((recs[:, 3] >> 16) & _lib.FRAME_OK) != 0) & (when >= 0) & (when < nsets)
        none = torch.iinfo(torch.int64).max
        start = torch.full((nsets,), none, dtype=torch.int64, device=offs.device)
        start.scatter_reduce_(0, when[ok], offs.to(torch.int64)[ok], 'amin')
        start = start.cpu().numpy()
        start[start == none] = -1
        return start

    # -- pickling: reopen by file name at the saved offset
    # (base/base.py:123-151,1020-1032); device buffers are re-creatable
    def __reduce__(self):
        recipe = getattr(self, '_pickle_recipe', None)
        if recipe is None:
            raise TypeError("can only pickle readers opened from named files")
        reopen, opener, source, init_args = recipe
        return (reopen, (opener, source, init_args, self.offset, bool(self.closed)))


# the reference's names for these roles (base/base.py)
StreamReaderBase = VLBIStreamReaderBase = GPUStreamReaderBase

from .writer import GPUStreamWriterBase          # noqa: E402  (no import cycle: writer is self-contained)
from .opener import FormatOpener                 # noqa: E402

StreamWriterBase = VLBIStreamWriterBase = GPUStreamWriterBase
FileOpener = FormatOpener
__all__ += ['StreamReaderBase', 'VLBIStreamReaderBase', 'StreamWriterBase',
            'VLBIStreamWriterBase', 'FileOpener']
