"""Thin Python wrappers over the C ABI: torch tensors in, torch tensors out.

PyTorch is used only as the device allocator / stream provider; every
computation is a libbbdecode kernel launched on torch's current HIP stream.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from ._lib import lib, check


_gpu_checked = False


def require_gpu():
    global _gpu_checked
    if _gpu_checked:
        return
    if not torch.cuda.is_available():
        raise RuntimeError(
            "baseband_amd needs an MI355X (gfx950) GPU: torch.cuda.is_available() "
            "is False and there is no CPU decode path in this package.")
    _gpu_checked = True                 # (the check costs microseconds per call)


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def _stream(t=None):
    """Handle of torch's current HIP stream on the current device.  The raw
    getter avoids ~8 us of Python in ``torch.cuda.current_stream()`` per call
    (three calls per small read).  `t` is a tensor the launch works on: the
    library launches on the CURRENT device (its level tables are per device),
    so data living on another GPU is refused instead of being addressed from
    the wrong device's stream."""
    dev = torch.cuda.current_device()
    if t is not None and t.device.index is not None and t.device.index != dev:
        raise RuntimeError(
            "tensor lives on cuda:{} but the current device is cuda:{}: wrap the call in "
            "`with torch.cuda.device({}):`".format(t.device.index, dev, t.device.index))
    if _raw_stream is not None:
        return C.c_void_p(_raw_stream(dev))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


_stream_objects = {}        # (device index, raw handle) -> torch.cuda.Stream


def current_stream(device):
    """``torch.cuda.current_stream(device)`` without its ~5 us of Python: the Stream object
    of a raw handle is remembered (two of these per mid-size read: the arena's reuse
    ordering and the scratch sets' events)."""
    if _raw_stream is None:
        return torch.cuda.current_stream(device)
    index = device.index if isinstance(device, torch.device) else int(device)
    if index is None:
        index = torch.cuda.current_device()
    raw = _raw_stream(index)
    s = _stream_objects.get((index, raw))
    if s is None:
        s = _stream_objects[(index, raw)] = torch.cuda.current_stream(index)
        if len(_stream_objects) > 64:       # (streams come and go: do not keep every one ever seen)
            for k in list(_stream_objects)[:32]:
                del _stream_objects[k]
    return s


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def init():
    require_gpu()
    check(lib.bb_init(), 'bb_init')


def to_device_bytes(raw, device=None):
    """Host bytes-like / ndarray -> 1-D uint8 device tensor (simple upload;
    the chunked pinned pipeline lives in `staging`)."""
    require_gpu()
    if isinstance(raw, torch.Tensor):
        t = raw if raw.dtype == torch.uint8 else raw.view(torch.uint8)
        return t.reshape(-1).to(device or 'cuda')
    a = np.frombuffer(raw, dtype=np.uint8) if not isinstance(raw, np.ndarray) \
        else np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
    return torch.from_numpy(np.array(a, copy=True)).to(device or 'cuda')


def _empty_output(nelem, device=None, dtype=torch.float32):
    """Flat output tensor of a decode launch (float32, or float16 / bfloat16 for
    a 16-bit decode): from the placement arena when there is one
    (placement.empty_output), else torch.empty.  The arena hands out float32
    blocks: 16-bit outputs are views of one, so that they are placed like the
    float32 results they replace."""
    from .placement import empty_output
    if dtype in (torch.float16, torch.bfloat16):
        return empty_output((int(nelem) + 1) // 2, torch.float32, device).view(dtype)[:int(nelem)]
    return empty_output(nelem, dtype, device)


empty_decoded = _empty_output


def _out_type(dtype):
    """torch element type of a decode's output -> enum bb_out_type."""
    t = _lib.out_type_of(dtype)
    if t is None or dtype.is_complex:
        raise TypeError("decoded samples are float32, float16 or bfloat16 elements, not {}".format(dtype))
    return t


def out_supported(coder, bps, chunk, nslot, payload_nbytes, dtype):
    """Would `decode_frames(..., out_dtype=dtype)` take these parameters?  Asks the
    library (bb_decode_out_check; no device needed); readers plan a 16-bit decode
    with it and keep float32-then-convert where it says no."""
    p = _lib.DecodeParams()
    p.coder, p.bps, p.chunk, p.nslot, p.payload_nbytes = coder, bps, chunk, nslot, payload_nbytes
    p.out_type = _out_type(dtype)
    return lib.bb_decode_out_check(C.byref(p)) == _lib.BB_OK


class _Target:
    """Output tensor for a decode launch.  The kernels store 16 bytes per
    lane, so the library wants `out` 16-byte aligned; a slice of a larger
    result that starts elsewhere (a read that enters a frame at an odd row) is
    decoded into a temporary and copied into place afterwards."""
    __slots__ = ('want', 'use')

    def __init__(self, out, nelem, device, dtype=torch.float32):
        self.want = out
        if out is None:
            self.use = _empty_output(nelem, device, dtype)
        elif out.dtype != dtype:
            raise TypeError("output tensor is {}, the decode writes {}".format(out.dtype, dtype))
        elif out.data_ptr() % 16 or not out.is_contiguous():
            self.use = _empty_output(out.numel(), device, dtype)
        else:
            self.use = out

    def done(self):
        if self.want is None or self.want is self.use:
            return self.use
        self.want.copy_(self.use.view_as(self.want))
        return self.want


def vdif_scan(dbuf, nframes, frame_nbytes, header_nbytes, pattern, mask,
              ref_seconds, ref_frame_nr, frame_rate, first_offset=0, set_nframes=0):
    """-> int32 tensor (nframes, 4): payload offset lo/hi, time_index,
    thread_id | flags << 16 (the 16-byte bb_frame_rec).  `set_nframes`:
    frames per frame set in file order -- sets are then formed as the
    reference's VDIFFrameSet.fromfile forms them (include/bbdecode.h)."""
    p = _vdif_params(frame_nbytes, header_nbytes, pattern, mask, ref_seconds, ref_frame_nr, frame_rate, first_offset)
    p.set_nframes = set_nframes
    recs = torch.empty((nframes, 4), dtype=torch.int32, device=dbuf.device)
    check(lib.bb_vdif_scan(_ptr(dbuf), dbuf.numel(), C.byref(p), _ptr(recs),
                           nframes, _stream(dbuf)), 'bb_vdif_scan')
    return recs


def _vdif_params(frame_nbytes, header_nbytes, pattern, mask, ref_seconds,
                 ref_frame_nr, frame_rate, first_offset=0):
    p = _lib.VDIFScanParams()
    p.first_offset = first_offset
    p.frame_nbytes = frame_nbytes
    p.header_nbytes = header_nbytes
    for i in range(8):
        p.pattern[i] = int(pattern[i]) if i < len(pattern) else 0
        p.mask[i] = int(mask[i]) if i < len(mask) else 0
    p.ref_seconds = ref_seconds
    p.ref_frame_nr = ref_frame_nr
    p.frame_rate = frame_rate
    return p


def _mark5b_params(ref_seconds, ref_frame_nr, frame_rate, first_offset=0):
    p = _lib.Mark5BScanParams()
    p.first_offset, p.ref_seconds = first_offset, ref_seconds
    p.ref_frame_nr, p.frame_rate = ref_frame_nr, frame_rate
    return p


def _mark4_params(ntrack, ref_year, ref_qms, frame_qms, first_offset=0):
    p = _lib.Mark4ScanParams()
    p.first_offset, p.ntrack, p.ref_year = first_offset, ntrack, ref_year
    p.ref_qms, p.frame_qms = ref_qms, frame_qms
    return p


def _side_handles(verified, scan_stream):
    """(event, side stream) as the window calls take them: raw handles, null for none."""
    return (C.c_void_p(verified) if verified else C.c_void_p(0),
            C.c_void_p(scan_stream.cuda_stream) if scan_stream is not None else C.c_void_p(0))


_NSCRATCH = 4       # sets of window scratch taking turns when the scan runs on a side stream


def _pow2(n):
    return 1 << max(0, int(n) - 1).bit_length()


class _FrameWindow:
    """Scratch handling shared by the window calls: the scan records and the
    index of a window.  With the scan on a SIDE stream (`scan_stream`: the
    verdict of request k + 1 does not queue behind the decode of request k on
    the caller's stream, include/bbdecode.h) there are `_NSCRATCH` = 4 sets
    taking turns: the decode of request k still reads one set while the scans
    of the next requests fill the others -- a caller can queue a burst of three
    more reads before the host is paced by the GPU -- and before a set is filled
    again the side stream waits for the event recorded behind the decode that
    used it last (16 bytes per frame and 8 per index entry each)."""
    __slots__ = ('recs', 'src', 'fill_value', '_sets', '_turn', '_rotating')

    def set_fill(self, fill_value):
        """Fill of the windows whose decode takes a `DecodeParams` (`self.dec`)."""
        fv = complex(fill_value)
        self.dec.fill_re, self.dec.fill_im = fv.real, fv.imag
        self.fill_value = fill_value

    def _scratch(self, nframes, n, dev, scan_stream=None):
        sets = getattr(self, '_sets', None)
        if sets is None:
            sets = self._sets = [[None, None, None] for _ in range(_NSCRATCH)]
            self._turn = 0
        k = 0
        if scan_stream is not None:
            self._turn = (self._turn + 1) % _NSCRATCH
            k = self._turn
        st = sets[k]
        small = (st[0] is None or st[0].shape[0] < nframes or st[0].device != dev
                 or st[1] is None or st[1].numel() < n or st[1].device != dev)
        if small and scan_stream is None:
            st[0] = torch.empty((max(_pow2(nframes), 64), 4), dtype=torch.int32, device=dev)
            st[1] = torch.empty(max(_pow2(n), 64), dtype=torch.int64, device=dev)
            st[2] = None
        elif small:
            # ALL sets at once (with headroom: they are re-made when a request outgrows
            # them): one allocation, and ONE wait of the side stream for the caller's --
            # torch's allocator hands out memory whose last user may still have work
            # queued on the caller's stream, which is safe there and nowhere else
            # (tools/stress_side_scan.py found a scan overwritten by such work)
            cr, cs = max(_pow2(nframes), 64), max(_pow2(n), 64)
            recs = torch.empty((_NSCRATCH * cr, 4), dtype=torch.int32, device=dev)
            src = torch.empty(_NSCRATCH * cs, dtype=torch.int64, device=dev)
            for j in range(_NSCRATCH):
                sets[j][0], sets[j][1], sets[j][2] = recs[j * cr:(j + 1) * cr], src[j * cs:(j + 1) * cs], None
            scan_stream.wait_stream(torch.cuda.current_stream(dev))
        self.recs, self.src = st[0], st[1]
        if scan_stream is not None and not small and st[2] is not None:
            scan_stream.wait_event(st[2])           # the decode that read this set last
        return st

    def _decode_queued(self, st, scan_stream, dev):
        """Behind a window call: remember where the decode that reads set `st`
        stands -- also for a call that did NOT use the side stream, once the
        sets rotate (a small read between large ones uses set 0 on the caller's
        stream; a later side-stream scan must not refill that set under its
        decode: found by tools/stress_side_scan.py)."""
        if scan_stream is not None or getattr(self, '_rotating', False):
            self._rotating = True
            if st[2] is None:
                st[2] = torch.cuda.Event()
            st[2].record(current_stream(dev))


class VDIFWindow(_FrameWindow):
    """One window of a VDIF stream read -- scan, index, verification, decode --
    as ONE library call (bb_vdif_read_window) with argument blocks that are
    built once per reader: a third of the host time of a small read() went
    into marshalling the same constants for four calls."""
    __slots__ = ('scan', 'dec')

    def __init__(self, frame_nbytes, header_nbytes, pattern, mask, ref_seconds, frame_rate,
                 payload_nbytes, coder, bps, chunk, nslot, complex_data, fill_value):
        self.scan = _vdif_params(frame_nbytes, header_nbytes, pattern, mask, ref_seconds, 0, frame_rate)
        p = self.dec = _lib.DecodeParams()
        p.coder, p.bps, p.chunk, p.nslot = coder, bps, chunk, nslot
        p.payload_nbytes = payload_nbytes
        p.complex_data = int(bool(complex_data))
        self.set_fill(fill_value)
        self.recs = self.src = self._sets = None

    def run(self, dbuf, ref_frame_nr, nframes, thread_slot, nsets, within, out,
            recs_per_index, nstrict, nbad, verified, scan_stream=None):
        """Launch the window on torch's current stream.  `out`: flat float32
        (or, without `within`, float16 / bfloat16: the decode then writes that
        type, bb_decode_params.out_type) device tensor; `nbad`: int32[1] device counter, or None for no
        verification; `verified`: raw handle of the event to record behind the
        verification launch, or None; `scan_stream`: torch stream for the scan /
        index / verification launches (needs `verified`; `_FrameWindow`)."""
        dev = dbuf.device
        self.scan.ref_frame_nr = ref_frame_nr
        if not verified:
            scan_stream = None
        st = self._scratch(nframes, nsets * self.dec.nslot, dev, scan_stream)
        self.dec.out_type = _out_type(out.dtype)
        tgt = _Target(out, out.numel(), dev, out.dtype)
        nsel = within.numel() if within is not None else 0
        check(lib.bb_vdif_read_window(
            _ptr(dbuf), dbuf.numel(), C.byref(self.scan), nframes, _ptr(thread_slot), nsets,
            C.byref(self.dec), _ptr(within), nsel, _ptr(self.recs), _ptr(self.src),
            _ptr(tgt.use), tgt.use.numel(), recs_per_index, nstrict, _ptr(nbad),
            *_side_handles(verified, scan_stream), _stream(dbuf)), 'bb_vdif_read_window')
        self._decode_queued(st, scan_stream, dev)
        tgt.done()


class Mark5BWindow(_FrameWindow):
    """One window of a Mark 5B stream read as one library call
    (bb_mark5b_read_window); see `VDIFWindow`."""
    __slots__ = ('scan', 'dec')

    def __init__(self, ref_seconds, frame_rate, bps, chunk, fill_value):
        self.scan = _mark5b_params(ref_seconds, 0, frame_rate)
        d = self.dec = _lib.DecodeParams()
        d.coder, d.bps, d.chunk, d.nslot, d.payload_nbytes = _lib.CODER_MARK5B, bps, chunk, 1, 10000
        self.recs = self.src = self._sets = None
        self.set_fill(fill_value)

    def run(self, dbuf, ref_frame_nr, nframes, n, within, out, nstrict, nbad, verified, scan_stream=None):
        self.scan.ref_frame_nr = ref_frame_nr
        if not verified:
            scan_stream = None
        st = self._scratch(nframes, n, dbuf.device, scan_stream)
        self.dec.out_type = _out_type(out.dtype)
        tgt = _Target(out, out.numel(), dbuf.device, out.dtype)
        check(lib.bb_mark5b_read_window(
            _ptr(dbuf), dbuf.numel(), C.byref(self.scan), nframes, n, C.byref(self.dec), _ptr(within),
            within.numel() if within is not None else 0, _ptr(self.recs), _ptr(self.src), _ptr(tgt.use),
            tgt.use.numel(), nstrict, _ptr(nbad), *_side_handles(verified, scan_stream), _stream(dbuf)),
            'bb_mark5b_read_window')
        self._decode_queued(st, scan_stream, dbuf.device)
        tgt.done()


class Mark4Window(_FrameWindow):
    """One window of a Mark 4 stream read as one library call
    (bb_mark4_read_window); see `VDIFWindow`."""
    __slots__ = ('scan', 'dec', 'nout', 'frame_qms', 'ref_qms')

    def __init__(self, ntrack, ref_year, ref_qms, frame_qms, nwords, sign_bit, mag_bit, select, fill_words,
                 fill_value):
        self.scan = _mark4_params(ntrack, ref_year, 0, frame_qms)
        self.ref_qms, self.frame_qms = ref_qms, frame_qms
        d = self.dec = _lib.Mark4DecodeParams()
        d.ntrack, d.nwords, d.fill_words = ntrack, nwords, fill_words
        for j, (s, m) in enumerate(zip(sign_bit, mag_bit)):
            d.sign_bit[j] = s
            d.mag_bit[j] = m
        self.nout = len(sign_bit) if select else 0
        self.recs = self.src = self._sets = None
        self.set_fill(fill_value)

    def set_fill(self, fill_value):
        self.dec.fill = float(fill_value)
        self.fill_value = fill_value

    def run(self, dbuf, first, nframes, n, out, nstrict, nbad, verified, scan_stream=None):
        self.scan.ref_qms = self.ref_qms + first * self.frame_qms
        if not verified:
            scan_stream = None
        st = self._scratch(nframes, n, dbuf.device, scan_stream)
        tgt = _Target(out, out.numel(), dbuf.device)
        check(lib.bb_mark4_read_window(
            _ptr(dbuf), dbuf.numel(), C.byref(self.scan), nframes, n, C.byref(self.dec), self.nout,
            _ptr(self.recs), _ptr(self.src), _ptr(tgt.use), tgt.use.numel(), nstrict, _ptr(nbad),
            *_side_handles(verified, scan_stream), _stream(dbuf)), 'bb_mark4_read_window')
        self._decode_queued(st, scan_stream, dbuf.device)
        tgt.done()


def vdif_locate(dbuf, nbytes, frame_nbytes, header_nbytes, pattern, mask):
    """Byte-granular header search -> sorted int64 device tensor of frame
    offsets (corruption-tolerant discovery)."""
    p = _vdif_params(frame_nbytes, header_nbytes, pattern, mask, 0, 0, 0)
    cap = nbytes // frame_nbytes + 16
    offs = torch.empty(cap, dtype=torch.int64, device=dbuf.device)
    count = torch.zeros(1, dtype=torch.int64, device=dbuf.device)
    check(lib.bb_vdif_locate(_ptr(dbuf), nbytes, C.byref(p), _ptr(offs), cap,
                             _ptr(count), _stream(dbuf)), 'bb_vdif_locate')
    n = min(int(count.item()), cap)
    return torch.sort(offs[:n]).values


def vdif_scan_at(dbuf, nbytes, offsets, frame_nbytes, header_nbytes, pattern,
                 mask, ref_seconds, ref_frame_nr, frame_rate):
    p = _vdif_params(frame_nbytes, header_nbytes, pattern, mask, ref_seconds,
                     ref_frame_nr, frame_rate)
    n = offsets.numel()
    recs = torch.empty((n, 4), dtype=torch.int32, device=dbuf.device)
    check(lib.bb_vdif_scan_at(_ptr(dbuf), nbytes, C.byref(p), _ptr(offsets), n,
                              _ptr(recs), _stream(dbuf)), 'bb_vdif_scan_at')
    return recs


def mark5b_scan(dbuf, nframes, ref_seconds, ref_frame_nr, frame_rate,
                first_offset=0, by_position=False):
    p = _mark5b_params(ref_seconds, ref_frame_nr, frame_rate, first_offset)
    p.by_position = int(bool(by_position))
    recs = torch.empty((nframes, 4), dtype=torch.int32, device=dbuf.device)
    check(lib.bb_mark5b_scan(_ptr(dbuf), dbuf.numel(), C.byref(p), _ptr(recs),
                             nframes, _stream(dbuf)), 'bb_mark5b_scan')
    return recs


def _collect_offsets(launch, dbuf, cap, where):
    offs = torch.empty(cap, dtype=torch.int64, device=dbuf.device)
    count = torch.zeros(1, dtype=torch.int64, device=dbuf.device)
    check(launch(_ptr(offs), cap, _ptr(count)), where)
    n = min(int(count.item()), cap)
    return torch.sort(offs[:n]).values


def mark5b_locate(dbuf, nbytes, w1_pattern=0, w1_mask=0):
    """Byte-granular Mark 5B frame search -> sorted int64 device offsets.  With a mask, word 1 of
    the headers must agree with the pattern under it (the stream's user word)."""
    return _collect_offsets(
        lambda offs, cap, count: lib.bb_mark5b_locate_stream(_ptr(dbuf), nbytes, int(w1_pattern) & 0xffffffff,
                                                             int(w1_mask) & 0xffffffff, offs, cap, count,
                                                             _stream(dbuf)),
        dbuf, nbytes // 10016 + 16, 'bb_mark5b_locate_stream')


def mark5b_scan_at(dbuf, nbytes, offsets, ref_seconds, ref_frame_nr, frame_rate):
    p = _mark5b_params(ref_seconds, ref_frame_nr, frame_rate)
    n = offsets.numel()
    recs = torch.empty((n, 4), dtype=torch.int32, device=dbuf.device)
    check(lib.bb_mark5b_scan_at(_ptr(dbuf), nbytes, C.byref(p), _ptr(offsets), n,
                                _ptr(recs), _stream(dbuf)), 'bb_mark5b_scan_at')
    return recs


def mark4_locate(dbuf, nbytes, ntrack):
    """Byte-granular Mark 4 frame search -> sorted int64 device offsets."""
    return _collect_offsets(
        lambda offs, cap, count: lib.bb_mark4_locate(_ptr(dbuf), nbytes, ntrack, offs, cap, count,
                                                     _stream(dbuf)),
        dbuf, nbytes // (ntrack * 2500) + 16, 'bb_mark4_locate')


def mark4_header_crc(dbuf, nframes, ntrack, first_offset=0, offsets=None):
    """Per frame the set of tracks (bit mask, int64 tensor) whose 160 header
    bits fail the CRC-12 along the track (bb_mark4_header_crc; the reference's
    ``crc12.check``, mark4/header.py:34-44).  Never alters decoded samples."""
    bad = torch.empty(nframes, dtype=torch.int64, device=dbuf.device)
    check(lib.bb_mark4_header_crc(_ptr(dbuf), dbuf.numel(), ntrack, _ptr(offsets), first_offset,
                                  nframes, _ptr(bad), _stream(dbuf)), 'bb_mark4_header_crc')
    return bad


def mark4_scan_at(dbuf, nbytes, offsets, ntrack, ref_year, ref_qms, frame_qms):
    p = _mark4_params(ntrack, ref_year, ref_qms, frame_qms)
    n = offsets.numel()
    recs = torch.empty((n, 4), dtype=torch.int32, device=dbuf.device)
    check(lib.bb_mark4_scan_at(_ptr(dbuf), nbytes, C.byref(p), _ptr(offsets), n,
                               _ptr(recs), _stream(dbuf)), 'bb_mark4_scan_at')
    return recs


def verify_records(recs, nrecs, first_index, recs_per_index, nstrict, nbad):
    """Add to the device counter `nbad` (int32[1]) the number of records that
    fail verification (see bb_verify_records)."""
    check(lib.bb_verify_records(_ptr(recs), nrecs, first_index, recs_per_index, nstrict,
                                _ptr(nbad), _stream(recs)), 'bb_verify_records')


def fetch_counter(counter, host, event, side_stream):
    """``host[0] = counter[0]`` fetched on `side_stream` once `event` has
    happened (bb_fetch_counter); returns when the value is there.  `host`: a
    pinned int32 tensor; `event`: torch.cuda.Event that has been recorded."""
    check(lib.bb_fetch_counter(_ptr(counter), C.c_void_p(host.data_ptr()),
                               C.c_void_p(event.cuda_event) if event is not None else C.c_void_p(0),
                               C.c_void_p(side_stream.cuda_stream)), 'bb_fetch_counter')


def recs_fields(recs):
    """Split scan records (device int32 (n,4)) into named host arrays."""
    r = recs.cpu().numpy()
    off = r[:, :2].copy().view(np.int64)[:, 0]
    tidx = r[:, 2]
    thread = (r[:, 3] & 0xffff).astype(np.int16)
    flags = ((r[:, 3] >> 16) & 0xffff).astype(np.uint16)
    return dict(payload_offset=off, time_index=tidx, thread_id=thread, flags=flags)


def thread_slot_map(thread_ids, device):
    m = np.full(1024, -1, dtype=np.int16)
    for s, t in enumerate(thread_ids):
        m[int(t)] = s
    return torch.from_numpy(m).to(device)


def build_index(recs, nframes_out, nslot=1, thread_slot=None):
    src = torch.empty(nframes_out * nslot, dtype=torch.int64, device=recs.device)
    check(lib.bb_build_index(_ptr(recs), recs.shape[0], _ptr(thread_slot), nslot,
                             _ptr(src), nframes_out, _stream(recs)), 'bb_build_index')
    return src


def decode_frames(dbuf, nframes, payload_nbytes, coder, bps, chunk=1, nslot=1,
                  src=None, src0=0, src_stride=0, complex_data=False,
                  fill_value=0., out=None, within=None, out_dtype=torch.float32):
    """Decode `nframes` frame(set)s to a flat float32 device tensor.  `within`
    (int32 device tensor of positions inside a thread sample's `chunk`
    floats) selects channels in the kernel: only those positions are
    written (bb_decode_frames_select).  `out_dtype` torch.float16 /
    torch.bfloat16: the kernels write that type (the float32 value rounded to
    nearest even; k_half.h); KeyError with `within`."""
    p = _lib.DecodeParams()
    p.out_type = _out_type(out_dtype)
    p.coder = coder
    p.bps = bps
    p.chunk = chunk
    p.nslot = nslot
    p.payload_nbytes = payload_nbytes
    p.src0 = src0
    p.src_stride = src_stride
    p.complex_data = int(bool(complex_data))
    fv = complex(fill_value)
    p.fill_re = fv.real
    p.fill_im = fv.imag
    nelem = nframes * nslot * (payload_nbytes * 8 // bps) if bps in (1, 2, 4, 8) else 0
    if within is not None:
        if src is None:                 # the selecting kernel works through an index
            src = src0 + torch.arange(nframes * nslot, dtype=torch.int64, device=dbuf.device) * src_stride
        nsel = within.numel()
        nelem = nelem // chunk * nsel
        if out is None:
            out = _empty_output(nelem, dbuf.device, out_dtype)
        check(lib.bb_decode_frames_select(_ptr(dbuf), dbuf.numel(), _ptr(src), nframes, C.byref(p),
                                          _ptr(within), nsel, _ptr(out), out.numel(), _stream(dbuf)),
              'bb_decode_frames_select')
        return out
    tgt = _Target(out, nelem, dbuf.device, out_dtype)
    check(lib.bb_decode_frames(_ptr(dbuf), dbuf.numel(), _ptr(src), nframes,
                               C.byref(p), _ptr(tgt.use), tgt.use.numel(), _stream(dbuf)),
          'bb_decode_frames')
    return tgt.done()


def copy_frames(dbuf, nframes, nbytes_per_frame, src0=0, src_stride=0, out=None):
    """`nframes` runs of `nbytes_per_frame` bytes of `dbuf` (uint8) at ``src0 +
    f * src_stride`` -> one contiguous float32 device tensor (bb_copy_frames):
    float32 samples passed through as they are.  EXTENSION -- the reference
    has no NBIT 32 decoder (dada/payload.py:40-41)."""
    nelem = nframes * nbytes_per_frame // 4
    tgt = _Target(out, nelem, dbuf.device)
    check(lib.bb_copy_frames(_ptr(dbuf), dbuf.numel(), nframes, nbytes_per_frame, src0, src_stride,
                             _ptr(tgt.use), tgt.use.numel() * 4, _stream(dbuf)), 'bb_copy_frames')
    return tgt.done()


STATES_MAX_ROW_BITS = 128      # chunk * bps the counting kernel takes (16 byte phases on chip)


# -- what the calls on packed bytes share (count_states, count_states_bins, repack_frames, requant_frames,
#    recode_frames, recode_frames_tables)
def _default_payload(bps, chunk):
    """The smallest payload of whole dwords and rows: what `*_supported` asks about by default."""
    return max(4, chunk * bps // 8) if bps in (1, 2, 4, 8) and chunk > 0 else 4


def _all_rows(nframes, payload_nbytes, bps, chunk):
    """The default `row_hi`: all rows of `nframes` frames (0 for a geometry the library will refuse)."""
    return nframes * (payload_nbytes * 8 // bps // chunk) if bps in (1, 2, 4, 8) and chunk > 0 else 0


def _given(tensor, name, dtype):
    """Did the caller give the tensor that a call adds to or writes into?  Then it is contiguous and of `dtype`."""
    if tensor is not None and (tensor.dtype != dtype or not tensor.is_contiguous()):
        raise TypeError("{} must be a contiguous {} tensor".format(name, str(dtype).split('.')[-1]))
    return tensor is not None


def _frames_out(call, precheck, name, dbuf, src, nframes, p, nrows, payload_out, row_bits, nslot, out):
    """The end of `repack_frames`, `requant_frames` and `recode_frames`: without `out`, whole output frames (`nslot` payloads
    with rows of `row_bits` bits) that hold the output rows [0, nrows); then the call."""
    if not _given(out, 'out', torch.uint8):
        check(precheck(C.byref(p)), name)                   # (before a shape is made of the parameters)
        out = torch.empty(-(-nrows // (payload_out * 8 // row_bits)) * nslot * payload_out, dtype=torch.uint8, device=dbuf.device)
    check(call(_ptr(dbuf), dbuf.numel(), _ptr(src), nframes, C.byref(p), _ptr(out), out.numel(), _stream(dbuf)), name)
    return out


def count_states_supported(bps, chunk=1, nslot=1, payload_nbytes=None):
    """Would `count_states` take this geometry?  (bb_count_states_check; no device needed.)"""
    if payload_nbytes is None:
        payload_nbytes = _default_payload(bps, chunk)
    return _lib.count_states_check(bps, chunk, nslot, payload_nbytes) == _lib.BB_OK


def count_states(dbuf, nframes, payload_nbytes, bps, chunk=1, nslot=1, src=None, src0=0,
                 src_stride=0, row_lo=0, row_hi=None, counts=None):
    """Sampler statistics from packed bytes (bb_count_states; EXTENSION, no reference
    counterpart): how often each raw code occurs per (thread slot, position in a row) among
    rows [row_lo, row_hi) of `nframes` frame(set)s -> int64 device tensor of shape
    ``(nslot, chunk, 1 << bps)``.  Frame-slots are taken through the index `src` (-1 or an
    offset outside the buffer: not counted) or at ``src0 + k * src_stride``.  With `counts`
    (such a tensor, contiguous) the call ADDS to it.  Codes are raw: the level of code c is
    ``_lib.get_levels(coder, bps)[c]``.  Nothing is decoded and nothing synchronises."""
    if row_hi is None:
        row_hi = _all_rows(nframes, payload_nbytes, bps, chunk)
    p = _lib.states_params(bps, chunk, nslot, payload_nbytes, src0, src_stride, row_lo, row_hi)
    if not _given(counts, 'counts', torch.int64):
        check(lib.bb_count_states_check(C.byref(p)), 'bb_count_states')     # (before a shape is made of the parameters)
        counts = torch.zeros((nslot, chunk, 1 << bps), dtype=torch.int64, device=dbuf.device)
    check(lib.bb_count_states(_ptr(dbuf), dbuf.numel(), _ptr(src), nframes, C.byref(p),
                              _ptr(counts), counts.numel(), _stream(dbuf)), 'bb_count_states')
    return counts


STATES_BINS_MAX_COUNTERS = 1024    # chunk << bps the binned kernel takes (two bins in a wave's window on chip)


def count_states_bins_supported(bps, chunk=1, bin_rows=8, nslot=1, payload_nbytes=None):
    """Would `count_states_bins` take this geometry and bin length?  (bb_count_states_bins_check;
    no device needed.)"""
    if payload_nbytes is None:
        payload_nbytes = _default_payload(bps, chunk)
    if not 0 <= bin_rows < 1 << 64:
        return False
    return _lib.count_states_bins_check(bps, chunk, bin_rows, nslot, payload_nbytes) == _lib.BB_OK


def count_states_bins(dbuf, nframes, payload_nbytes, bps, chunk, nslot, bin_rows, nbins, src=None, src0=0,
                      src_stride=0, row_lo=0, row_hi=None, first_row=0, counts=None):
    """Sampler statistics per time bin from packed bytes (bb_count_states_bins; EXTENSION):
    as `count_states`, but counted row r goes to bin ``(first_row + r - row_lo) // bin_rows``
    -> int32 device tensor of shape ``(nslot, nbins, chunk, 1 << bps)``.  Bins, `first_row`
    and the row range are whole bytes of a slot's stream.  With `counts` (such a tensor,
    contiguous) the call ADDS to it: windows of a file complete each other's bins.  Nothing
    is decoded and nothing synchronises."""
    if row_hi is None:
        row_hi = _all_rows(nframes, payload_nbytes, bps, chunk)
    p = _lib.states_params(bps, chunk, nslot, payload_nbytes, src0, src_stride, row_lo, row_hi)
    if not _given(counts, 'counts', torch.int32):
        check(lib.bb_count_states_bins_check(C.byref(p), bin_rows), 'bb_count_states_bins')
        counts = torch.zeros((nslot, nbins, chunk, 1 << bps), dtype=torch.int32, device=dbuf.device)
    check(lib.bb_count_states_bins(_ptr(dbuf), dbuf.numel(), _ptr(src), nframes, C.byref(p), bin_rows, first_row,
                                   nbins, _ptr(counts), counts.numel(), _stream(dbuf)), 'bb_count_states_bins')
    return counts


def _fits(*values):
    """Are these all integers that the parameter block's fields hold?"""
    return all(0 <= v < 1 << 31 for v in values[:4]) and all(0 <= v < 1 << 63 for v in values[4:])


def i8_moments_supported(layout, npol, nchan, ncomp, ntime, t_lo=0, t_hi=None, bin_rows=1, src0=0, src_stride=0):
    """Would `i8_moments` take this geometry?  (bb_i8_moments_check; no device needed.)"""
    if t_hi is None:
        t_hi = ntime
    if not _fits(layout, npol, nchan, ncomp, ntime, t_lo, t_hi, bin_rows, src0, src_stride):
        return False
    return _lib.i8_moments_check(layout, npol, nchan, ncomp, ntime, t_lo, t_hi, bin_rows, src0, src_stride) == _lib.BB_OK


def i8_moments(dbuf, nframes, layout, npol, nchan, ncomp, ntime, t_lo, t_hi, bin_rows, nbins, first_row=0,
               src0=0, src_stride=0, src=None, sums=None):
    """Sums of x and of x * x per component and time bin from stored int8 samples (bb_i8_moments;
    EXTENSION, no reference counterpart): times [t_lo, t_hi) of `nframes` payloads of `ntime`
    times each, in `layout` (``_lib.MOMENTS_GUPPI_CF``, ``_GUPPI_TF``, ``_ROWS``), taken through
    the index `src` (-1 or an offset outside the buffer: adds nothing) or at ``src0 + k *
    src_stride``.  Time t of frame f is row ``first_row + f * (t_hi - t_lo) + (t - t_lo)`` of a
    series and lands in bin ``row // bin_rows`` -> int64 device tensor of shape ``(nbins, npol,
    nchan, ncomp, 2)``, the last axis (sum of x, sum of x * x).  With `sums` (such a tensor,
    contiguous) the call ADDS to it: windows of a file and pieces with different row ranges fill
    one answer.  Nothing is decoded and nothing synchronises."""
    p = _lib.moments_params(layout, npol, nchan, ncomp, ntime, t_lo, t_hi, bin_rows, nbins, first_row, src0, src_stride)
    if not _given(sums, 'sums', torch.int64):
        check(lib.bb_i8_moments_check(C.byref(p)), 'bb_i8_moments')          # (before a shape is made of the parameters)
        sums = torch.zeros((nbins, npol, nchan, ncomp, 2), dtype=torch.int64, device=dbuf.device)
    check(lib.bb_i8_moments(_ptr(dbuf), dbuf.numel(), _ptr(src), nframes, C.byref(p), _ptr(sums), sums.numel(),
                            _stream(dbuf)), 'bb_i8_moments')
    return sums


def i8_coherence_supported(layout, nchan, ntime, t_lo=0, t_hi=None, bin_rows=1, src0=0, src_stride=0):
    """Would `i8_coherence` take this geometry of two complex polarisations?  (bb_i8_coherence_check; no
    device needed.)"""
    if t_hi is None:
        t_hi = ntime
    if not _fits(layout, 2, nchan, 2, ntime, t_lo, t_hi, bin_rows, src0, src_stride):
        return False
    return _lib.i8_coherence_check(layout, 2, nchan, 2, ntime, t_lo, t_hi, bin_rows, src0, src_stride) == _lib.BB_OK


def i8_coherence(dbuf, nframes, layout, nchan, ntime, t_lo, t_hi, bin_rows, nbins, first_row=0,
                 src0=0, src_stride=0, src=None, sums=None):
    """Cross-polarisation products per channel and time bin from stored int8 samples of two complex
    polarisations X, Y (bb_i8_coherence; EXTENSION, no reference counterpart): frames, times, the
    series of rows and its bins as in `i8_moments` -> int64 device tensor of shape ``(nbins, nchan,
    4)``, the last axis (sum |X|^2, sum |Y|^2, Re sum X conj(Y), Im sum X conj(Y)).  With `sums`
    (such a tensor, contiguous) the call ADDS to it.  Nothing is decoded and nothing synchronises."""
    p = _lib.moments_params(layout, 2, nchan, 2, ntime, t_lo, t_hi, bin_rows, nbins, first_row, src0, src_stride)
    if not _given(sums, 'sums', torch.int64):
        check(lib.bb_i8_coherence_check(C.byref(p)), 'bb_i8_coherence')      # (before a shape is made of the parameters)
        sums = torch.zeros((nbins, nchan, 4), dtype=torch.int64, device=dbuf.device)
    check(lib.bb_i8_coherence(_ptr(dbuf), dbuf.numel(), _ptr(src), nframes, C.byref(p), _ptr(sums), sums.numel(),
                              _stream(dbuf)), 'bb_i8_coherence')
    return sums


REPACK_MAX_ROW_BITS = 256      # nslot * chunk * bps the repack kernel takes
REPACK_MAX_SLOTS = 32          # ... and thread slots on either side


def repack_supported(bps, coder_in, coder_out, chunk_in, nslot_in, chunk_out, nslot_out,
                     payload_in=None, payload_out=None):
    """Would `repack_frames` take this conversion?  (bb_repack_check; no device needed.)"""
    if payload_in is None:
        payload_in = _default_payload(bps, chunk_in)
    if payload_out is None:
        payload_out = _default_payload(bps, chunk_out)
    return _lib.repack_check(bps, coder_in, coder_out, chunk_in, nslot_in, chunk_out, nslot_out,
                             payload_in, payload_out) == _lib.BB_OK


def repack_frames(dbuf, nframes, payload_in, bps, coder_in, chunk_in, nslot_in, coder_out, chunk_out, nslot_out,
                  payload_out, fill_code=0, src=None, src0=0, src_stride=0, row_lo=0, row_hi=None, first_row=0,
                  out=None):
    """Format conversion on the packed bytes (bb_repack_frames): rows [row_lo, row_hi) of
    `nframes` input frame(set)s of `nslot_in` payloads with `chunk_in` codes per row, taken
    through the index `src` (-1 or an offset outside the buffer: `fill_code`) or at ``src0 +
    k * src_stride``, become output rows ``first_row + (r - row_lo)`` of payloads of
    `nslot_out` slots with `chunk_out` codes per row, codes mapped from `coder_in` to
    `coder_out` -> uint8 device tensor of whole output frames, payload (F, t) at ``(F *
    nslot_out + t) * payload_out``.  With `out` (such a tensor, contiguous) only the bytes
    of the rows written change.  The row range and `first_row` are whole bytes of every
    slot stream.  Nothing is decoded and nothing synchronises."""
    if row_hi is None:
        row_hi = _all_rows(nframes, payload_in, bps, chunk_in)
    p = _lib.repack_params(bps, coder_in, coder_out, chunk_in, nslot_in, chunk_out, nslot_out, payload_in,
                           payload_out, fill_code, src0, src_stride, row_lo, row_hi, first_row)
    return _frames_out(lib.bb_repack_frames, lib.bb_repack_check, 'bb_repack_frames', dbuf, src, nframes, p,
                       first_row + row_hi - row_lo, payload_out, bps * chunk_out, nslot_out, out)


REQUANT_MAX_ROW_BITS = 256     # chunk * max(bps_in, bps_out) the requantize kernel takes
REQUANT_MAX_SLOTS = 32         # ... and thread slots


def requant_supported(bps_in, bps_out, chunk=1, nslot=1, payload_in=None, payload_out=None):
    """Would `requant_frames` take these widths and this geometry?  (bb_requant_check; no device needed.)"""
    if payload_in is None:
        payload_in = _default_payload(bps_in, chunk)
    if payload_out is None:
        payload_out = _default_payload(bps_out, chunk)
    return _lib.requant_check(bps_in, bps_out, chunk, nslot, payload_in, payload_out) == _lib.BB_OK


def requant_table(coder_in, bps_in, coder_out, bps_out, scale=None):
    """The table of `requant_frames` that is decode, times `scale`, encode: uint8 NumPy array
    of ``1 << bps_in`` output codes by input code.  Made with the pieces the loop
    ``fw.write(fr.read(n) * scale)`` runs on -- the decoder's float32 levels
    (`_lib.get_levels`), a float32 product, the encode kernel (`encode_flat`) -- so it IS
    that arithmetic.  ``scale=None`` stands for 1.0, which is exact."""
    levels = _lib.get_levels(coder_in, bps_in).astype(np.float32)
    if scale is not None:
        if not np.isfinite(scale):
            raise ValueError("requant_table: scale must be finite")
        levels = levels * np.float32(scale)
    levels = np.pad(levels, (0, max(0, 8 - levels.size)))       # (whole bytes at every width the encoder has)
    packed = encode_flat(torch.from_numpy(levels).cuda(), coder_out, bps_out).cpu().numpy()
    codes = (packed[:, None] >> np.arange(0, 8, bps_out, dtype=np.uint8)) & ((1 << bps_out) - 1)
    return np.ascontiguousarray(codes.reshape(-1)[:1 << bps_in].astype(np.uint8))


def requant_frames(dbuf, nframes, payload_in, bps_in, chunk, nslot, bps_out, payload_out, table, fill_code=0,
                   src=None, src0=0, src_stride=0, row_lo=0, row_hi=None, first_row=0, out=None):
    """Conversion between sample widths on the packed bytes (bb_requant_frames): rows
    [row_lo, row_hi) of `nframes` input frame(set)s of `nslot` payloads with `chunk` codes of
    `bps_in` bits per row, taken through the index `src` (-1 or an offset outside the buffer:
    `fill_code`, not mapped) or at ``src0 + k * src_stride``, become output rows ``first_row +
    (r - row_lo)`` of payloads of the same slot structure with codes of `bps_out` bits, code
    c as ``table[c]`` -> uint8 device tensor of whole output frames, payload (F, s) at ``(F *
    nslot + s) * payload_out``.  With `out` (such a tensor, contiguous) only the bytes of
    the rows written change.  The row range and `first_row` are whole bytes of a slot stream
    on both sides.  Nothing is decoded and nothing synchronises."""
    if row_hi is None:
        row_hi = _all_rows(nframes, payload_in, bps_in, chunk)
    p = _lib.requant_params(bps_in, bps_out, chunk, nslot, payload_in, payload_out, table, fill_code,
                            src0, src_stride, row_lo, row_hi, first_row)
    return _frames_out(lib.bb_requant_frames, lib.bb_requant_check, 'bb_requant_frames', dbuf, src, nframes, p,
                       first_row + row_hi - row_lo, payload_out, bps_out * chunk, nslot, out)


RECODE_MAX_ROW_BITS = 256      # nslot * chunk * max(bps_in, bps_out) the recode kernel takes
RECODE_MAX_SLOTS = 32          # ... and thread slots on either side


def recode_supported(bps_in, bps_out, chunk_in, nslot_in, chunk_out, nslot_out, payload_in=None, payload_out=None):
    """Would `recode_frames` take these widths and this change of thread structure?  (bb_recode_check; no
    device needed.)"""
    if payload_in is None:
        payload_in = _default_payload(bps_in, chunk_in)
    if payload_out is None:
        payload_out = _default_payload(bps_out, chunk_out)
    return _lib.recode_check(bps_in, bps_out, chunk_in, nslot_in, chunk_out, nslot_out,
                             payload_in, payload_out) == _lib.BB_OK


def recode_frames(dbuf, nframes, payload_in, bps_in, chunk_in, nslot_in, bps_out, chunk_out, nslot_out, payload_out,
                  table, fill_code=0, src=None, src0=0, src_stride=0, row_lo=0, row_hi=None, first_row=0, out=None):
    """Conversion between sample widths across thread structures on the packed bytes
    (bb_recode_frames): `repack_frames` with the table of `requant_frames` in place of the
    coder pair.  Rows [row_lo, row_hi) of `nframes` input frame(set)s of `nslot_in` payloads
    with `chunk_in` codes of `bps_in` bits per row, taken through the index `src` (-1 or an
    offset outside the buffer: `fill_code`, not mapped) or at ``src0 + k * src_stride``,
    become output rows ``first_row + (r - row_lo)`` of payloads of `nslot_out` slots with
    `chunk_out` codes of `bps_out` bits per row, code c as ``table[c]`` -> uint8 device tensor
    of whole output frames, payload (F, t) at ``(F * nslot_out + t) * payload_out``.  With
    `out` (such a tensor, contiguous) only the bytes of the rows written change.  The row
    range and `first_row` are whole bytes of every slot stream on both sides.  Nothing is
    decoded and nothing synchronises."""
    if row_hi is None:
        row_hi = _all_rows(nframes, payload_in, bps_in, chunk_in)
    p = _lib.recode_params(bps_in, bps_out, chunk_in, nslot_in, chunk_out, nslot_out, payload_in, payload_out, table,
                           fill_code, src0, src_stride, row_lo, row_hi, first_row)
    return _frames_out(lib.bb_recode_frames, lib.bb_recode_check, 'bb_recode_frames', dbuf, src, nframes, p,
                       first_row + row_hi - row_lo, payload_out, bps_out * chunk_out, nslot_out, out)


def requant_tables(coder_in, bps_in, coder_out, bps_out, scales):
    """The tables of `recode_frames_tables` that are decode, times ``scales[k]``, encode for
    component k of a row: uint8 NumPy array of shape ``(ncomp, 1 << bps_in)``, row k of which is
    ``requant_table(coder_in, bps_in, coder_out, bps_out, scales[k])``.  Made as that one is --
    the decoder's float32 levels, a float32 product with ``np.float32(scales[k])``, ONE
    `encode_flat` call for all rows -- so it IS the arithmetic of the loop
    ``fw.write(fr.read(n) * gains)``."""
    scales = np.asarray(scales, dtype=np.float32).reshape(-1)
    if scales.size == 0 or not np.isfinite(scales).all():
        raise ValueError("requant_tables: scales must be finite, one per component")
    levels = _lib.get_levels(coder_in, bps_in).astype(np.float32)
    levels = (levels[None, :] * scales[:, None]).reshape(-1)
    levels = np.pad(levels, (0, -levels.size % 8))              # (whole bytes at every width the encoder has)
    packed = encode_flat(torch.from_numpy(levels).cuda(), coder_out, bps_out).cpu().numpy()
    codes = (packed[:, None] >> np.arange(0, 8, bps_out, dtype=np.uint8)) & ((1 << bps_out) - 1)
    return np.ascontiguousarray(codes.reshape(-1)[:scales.size << bps_in].astype(np.uint8).reshape(scales.size, 1 << bps_in))


def recode_tables_supported(bps_in, bps_out, chunk_in, nslot_in, chunk_out, nslot_out, payload_in=None,
                            payload_out=None):
    """Would `recode_frames_tables` take these widths and this geometry (equal thread structures
    included)?  (bb_recode_tables_check; no device needed.)"""
    if payload_in is None:
        payload_in = _default_payload(bps_in, chunk_in)
    if payload_out is None:
        payload_out = _default_payload(bps_out, chunk_out)
    return _lib.recode_tables_check(bps_in, bps_out, chunk_in, nslot_in, chunk_out, nslot_out,
                                    payload_in, payload_out) == _lib.BB_OK


def _device_tables(tables, ncomp, bps_in, bps_out, device):
    """`tables` of `recode_frames_tables` -> a contiguous uint8 device tensor of ``(ncomp, 1 << bps_in)``.  A NumPy
    array is checked against ``1 << bps_out`` here and uploaded; a device tensor's values are the kernel's to mask."""
    shape = (ncomp, 1 << bps_in) if bps_in in (1, 2, 4, 8) else None
    if isinstance(tables, np.ndarray):
        if tables.dtype != np.uint8 or (shape is not None and tables.shape != shape):
            raise ValueError("recode_frames_tables: tables must be a uint8 array of shape {}, not {} of shape {}"
                             .format(shape, tables.dtype, tables.shape))
        if bps_out in (1, 2, 4, 8) and tables.size and int(tables.max()) >= 1 << bps_out:
            raise ValueError("recode_frames_tables: a table entry is not a code of {} bits".format(bps_out))
        return torch.from_numpy(np.ascontiguousarray(tables)).to(device)
    if not torch.is_tensor(tables) or tables.dtype != torch.uint8 or not tables.is_contiguous() or \
            tables.device != device or (shape is not None and tuple(tables.shape) != shape):
        raise ValueError("recode_frames_tables: tables must be a contiguous uint8 array or device tensor of shape {}"
                         .format(shape))
    return tables


def recode_frames_tables(dbuf, nframes, payload_in, bps_in, chunk_in, nslot_in, bps_out, chunk_out, nslot_out,
                         payload_out, tables, fill_code=0, src=None, src0=0, src_stride=0, row_lo=0, row_hi=None,
                         first_row=0, out=None):
    """`recode_frames` with one table per component of a row (bb_recode_frames_tables): code c of
    component k = s * chunk_in + p becomes ``tables[k][c]``; everything else -- rows, index,
    `fill_code` (one code, not mapped), `out`, whole bytes -- is as there, and the thread
    structures may be equal.  `tables`: uint8 of shape ``(nslot_in * chunk_in, 1 << bps_in)``
    (`requant_tables`), a NumPy array (checked against ``1 << bps_out`` and uploaded once per
    call) or a device tensor (the kernel keeps the low `bps_out` bits of every entry).  Nothing
    is decoded and nothing synchronises."""
    if row_hi is None:
        row_hi = _all_rows(nframes, payload_in, bps_in, chunk_in)
    p = _lib.recode_params(bps_in, bps_out, chunk_in, nslot_in, chunk_out, nslot_out, payload_in, payload_out, (),
                           fill_code, src0, src_stride, row_lo, row_hi, first_row)
    check(lib.bb_recode_tables_check(C.byref(p)), 'bb_recode_frames_tables')    # (before a shape is made of the parameters)
    dtab = _device_tables(tables, nslot_in * chunk_in, bps_in, bps_out, dbuf.device)

    def call(buf, buf_n, src_, nfr, params, out_, out_n, stream):
        return lib.bb_recode_frames_tables(buf, buf_n, src_, nfr, params, _ptr(dtab), dtab.numel(), out_, out_n, stream)

    return _frames_out(call, lib.bb_recode_tables_check, 'bb_recode_frames_tables', dbuf, src, nframes, p,
                       first_row + row_hi - row_lo, payload_out, bps_out * chunk_out, nslot_out, out)


TOUCH_MIN_BYTES = 16 << 20
def _touch_max_bytes():
    try:                                # (as the library reads it: csrc/bbdecode.hip touch_mib_default)
        mib = int(os.environ.get('BB_TOUCH_MIB', '') or 256)
    except ValueError:
        mib = 256
    return (256 if mib < 0 else mib) << 20


TOUCH_MAX_BYTES = _touch_max_bytes()


def touch(dbuf, lo, nbytes):
    """Queue a pass that reads bytes [lo, lo + nbytes) of the uint8 device tensor `dbuf` once
    and keeps nothing (bb_touch): a decode of those bytes queued right behind it finds them in
    the device's memory-side cache.  Does nothing outside 16 MiB .. BB_TOUCH_MIB (256)."""
    if TOUCH_MIN_BYTES <= nbytes <= TOUCH_MAX_BYTES:
        check(lib.bb_touch(C.c_void_p(dbuf.data_ptr() + int(lo)), int(nbytes), _stream(dbuf)), 'bb_touch')


def select_supported(bps, chunk, nslot, nwithin, payload_nbytes=None):
    """Would `decode_frames(..., within=...)` take this geometry?  Asks the
    library's own argument / geometry checks (bb_decode_frames_select_check;
    no device needed), so that readers fold a channel subset into the decode
    only when the kernel accepts it and keep the reference's
    decode-then-index order otherwise.  `payload_nbytes` None: a payload long
    enough not to limit the work items (requests of varying length)."""
    p = _lib.DecodeParams()
    p.coder = _lib.CODER_VDIF               # (any coder that has this sample width: the limits do not depend on it)
    p.bps = bps
    p.chunk = chunk
    p.nslot = nslot
    if payload_nbytes is None:
        payload_nbytes = max(1 << 20, chunk * bps // 8 * 4) if bps in (1, 2, 4, 8) else 0
    p.payload_nbytes = payload_nbytes
    return lib.bb_decode_frames_select_check(C.byref(p), int(nwithin)) == _lib.BB_OK


def mark4_scan(dbuf, nframes, ntrack, ref_year, ref_qms, frame_qms,
               first_offset=0):
    p = _mark4_params(ntrack, ref_year, ref_qms, frame_qms, first_offset)
    recs = torch.empty((nframes, 4), dtype=torch.int32, device=dbuf.device)
    check(lib.bb_mark4_scan(_ptr(dbuf), dbuf.numel(), C.byref(p), _ptr(recs),
                            nframes, _stream(dbuf)), 'bb_mark4_scan')
    return recs


def mark4_select_maps(sign_bit, mag_bit, nchan, channels):
    """Bit maps of a Mark 4 mode restricted to `channels`: output ``fo * nchan
    + c`` of a stream word is sample `fo`, channel `c`; the result lists, for
    every sample of the word, the kept channels in the order given."""
    fanout = len(sign_bit) // nchan
    keep = [fo * nchan + int(c) for fo in range(fanout) for c in channels]
    return [sign_bit[j] for j in keep], [mag_bit[j] for j in keep]


def decode_mark4(dbuf, nframes, ntrack, nwords, sign_bit, mag_bit, fill_words=0,
                 src=None, src0=0, src_stride=0, fill_value=0., out=None, select=False,
                 out_dtype=torch.float32):
    """Track-demultiplex `nframes` units of `nwords` stream words each ->
    flat float32 device tensor of nframes * nwords * ntrack/2 values.  With
    `select` the maps may be shorter (the outputs of the channels a reader's
    subset keeps, `mark4_select_maps`): every word then gives ``len(sign_bit)``
    values (bb_decode_mark4_select).  The Mark 4 kernels write float32 only:
    KeyError (BB_ENOTSUP) for any other `out_dtype`, nothing is launched."""
    p = _lib.Mark4DecodeParams()
    p.out_type = _out_type(out_dtype)
    p.ntrack = ntrack
    p.nwords = nwords
    p.fill_words = fill_words
    p.src0 = src0
    p.src_stride = src_stride
    for j, (s, m) in enumerate(zip(sign_bit, mag_bit)):
        p.sign_bit[j] = s
        p.mag_bit[j] = m
    p.fill = float(fill_value)
    if select:
        nout = len(sign_bit)
        nelem = nframes * nwords * nout
        if out is None:
            out = _empty_output(nelem, dbuf.device, out_dtype)
        check(lib.bb_decode_mark4_select(_ptr(dbuf), dbuf.numel(), _ptr(src), nframes, C.byref(p),
                                         nout, _ptr(out), out.numel(), _stream(dbuf)),
              'bb_decode_mark4_select')
        return out
    tgt = _Target(out, nframes * nwords * (ntrack // 2), dbuf.device, out_dtype)
    check(lib.bb_decode_mark4(_ptr(dbuf), dbuf.numel(), _ptr(src), nframes,
                              C.byref(p), _ptr(tgt.use), tgt.use.numel(), _stream(dbuf)),
          'bb_decode_mark4')
    return tgt.done()


def decode_i8_tiled(dbuf, nframes, layout, npol, nchan, ntime, t_lo, t_hi,
                    src=None, src0=0, src_stride=0, fill_value=0., out=None, nchan_stored=0,
                    npol_stored=0, pol_first=0, chan_map=None, out_dtype=torch.float32):
    """int8 (re, im) -> complex64 with the (time, pol, chan) permutation of
    `layout`; rows [t_lo, t_hi) of every frame -> flat float32 tensor.  With
    `nchan_stored` the payload holds that many channels and the `nchan`
    starting at the payload offset are decoded (`tiled_channel_skip`).  A
    SELECTION -- `chan_map` (int32 device tensor of `nchan` stored-channel
    numbers) and / or `npol` of `npol_stored` polarisations from `pol_first` on
    -- is decoded from payload offsets that point at the payload start;
    KeyError when the library's fast form does not take the geometry -- and for
    an `out_dtype` other than float32: bb_tiled_params has no output type, the
    transposing kernels write float32 only (BB_ENOTSUP without a call)."""
    if _out_type(out_dtype) != _lib.OUT_F32:
        check(_lib.BB_ENOTSUP, 'bb_decode_i8_tiled')
    p = _lib.TiledParams()
    p.layout = layout
    p.npol = npol
    p.nchan = nchan
    p.nchan_stored = nchan_stored
    p.npol_stored = npol_stored
    p.pol_first = pol_first
    p.d_chan_map = chan_map.data_ptr() if chan_map is not None else None
    p.ntime = ntime
    p.t_lo = t_lo
    p.t_hi = t_hi
    p.src0 = src0
    p.src_stride = src_stride
    fv = complex(fill_value)
    p.fill_re = fv.real
    p.fill_im = fv.imag
    nelem = nframes * (t_hi - t_lo) * npol * nchan * 2
    tgt = _Target(out, nelem, dbuf.device)
    check(lib.bb_decode_i8_tiled(_ptr(dbuf), dbuf.numel(), _ptr(src), nframes,
                                 C.byref(p), _ptr(tgt.use), tgt.use.numel(), _stream(dbuf)),
          'bb_decode_i8_tiled')
    return tgt.done()


def tiled_channel_skip(layout, npol, ntime, c_lo):
    """Bytes from the start of a payload to its channel `c_lo`, for
    `decode_i8_tiled(..., nchan_stored=...)`."""
    if layout == _lib.LAYOUT_GUPPI_CF:
        return c_lo * ntime * npol * 2          # every channel is one run of all times
    if layout == _lib.LAYOUT_MKBF:
        return c_lo * 256 * 2                   # 256 times of a channel inside a (heap, pol) block
    return c_lo * npol * 2                      # channels of one time lie side by side


def as_device_samples(data):
    """Samples to encode -> float32 / complex64 tensor on the GPU (NumPy
    arrays and host tensors are uploaded)."""
    require_gpu()
    if not isinstance(data, torch.Tensor):
        from .staging import upload_array
        data = upload_array(data)
    want = torch.complex64 if data.is_complex() else torch.float32
    return data.to(device='cuda', dtype=want)


def _encode_input(values):
    """Samples as the encode kernels read them: flat contiguous float32 that
    starts on a 16-byte boundary (they load float4).  A contiguous view that
    starts elsewhere in its storage (`samples[1:]`) is copied; an aligned
    tensor is handed on as it is."""
    values = values.to(torch.float32).contiguous().reshape(-1)
    if values.data_ptr() % 16:
        values = values.clone()
    return values


def encode_flat(values, coder, bps):
    """float32 (or complex64) device tensor -> packed uint8 device tensor."""
    require_gpu()
    if values.is_complex():
        values = torch.view_as_real(values)
    values = _encode_input(values)
    nbytes = values.numel() * bps // 8 if bps in (1, 2, 4, 8) else 0
    # the kernel packs quads of samples into whole bytes: a shorter tail (item
    # assignment of a few samples) is padded here and cut off the output
    unit = max(4, 8 // bps) if bps in (1, 2, 4, 8) else 4
    short = -values.numel() % unit
    if short and (values.numel() * bps) % 8 == 0:       # whole bytes only
        values = torch.nn.functional.pad(values, (0, short))
    out = torch.empty(values.numel() * bps // 8 if bps in (1, 2, 4, 8) else 0,
                      dtype=torch.uint8, device=values.device)
    check(lib.bb_encode_flat(_ptr(values), values.numel(), coder, bps, _ptr(out),
                             out.numel(), _stream(values)), 'bb_encode_flat')
    return out[:nbytes]


def encode_mark4(values, ntrack, sign_bit, mag_bit):
    """(nsample, nchan) float32 device tensor -> stream words as uint8."""
    require_gpu()
    values = _encode_input(values)
    opw = ntrack // 2
    nwords = values.numel() // opw
    sb = (C.c_uint8 * 32)(*sign_bit)
    mb = (C.c_uint8 * 32)(*mag_bit)
    out = torch.empty(nwords * (ntrack // 8), dtype=torch.uint8, device=values.device)
    check(lib.bb_encode_mark4(_ptr(values), nwords, ntrack, sb, mb, _ptr(out),
                              out.numel(), _stream(values)), 'bb_encode_mark4')
    return out


def tune(knob, value):
    check(lib.bb_tune(knob, value), 'bb_tune')
