"""Format conversion between stream readers and stream writers (`baseband_amd.convert`).

The reference converts by decoding and encoding again (docs/tutorials/
using_baseband.rst:536-593): ``fw.write(fr.read(n))``.  Between VDIF and Mark 5B streams
of the same sample size that is an exact map from code to code and a permutation of bit
fields, which `kernels.repack_frames` does on the packed bytes: N bytes in, N out, against
34 N of traffic through float32 at 2 bits.  `convert` takes that path where it applies
and the decode / encode loop everywhere else; the file is the same byte for byte.
"""
import numpy as np
import torch

from . import _lib, kernels
from .base.packed import samples_per_byte

__all__ = ['convert']

PACKED_PIECE_BYTES = 256 << 20      # packed output per piece of the repack path
LOOP_PIECE_BYTES = 256 << 20        # decoded float32 per piece of the loop


def _writer_layout(fw):
    """(coder, nthread, nchan) of a VDIF or Mark 5B stream writer of this package, else None."""
    from .vdif.base import VDIFStreamWriter
    from .mark5b.base import Mark5BStreamWriter
    if isinstance(fw, VDIFStreamWriter):
        return (fw._coder,) + tuple(fw._unsliced_shape)
    if isinstance(fw, Mark5BStreamWriter):
        return (_lib.CODER_MARK5B, 1, fw._unsliced_shape[0])
    return None


def _channel_subset(fr):
    """Does the reader's `subset` pick anything but whole threads?"""
    if not fr.subset:
        return False
    threads_first = hasattr(fr, '_file_threads') and (len(fr._file_threads) > 1 or not fr.squeeze)
    return not threads_first or len(fr.subset) > 1


def _fill_code(value, coder, bps):
    """The code the encoder gives `value`."""
    unit = max(4, 8 // bps)
    packed = kernels.encode_flat(torch.full((unit,), float(value), dtype=torch.float32, device='cuda'), coder, bps)
    return int(packed[0].item()) & ((1 << bps) - 1)


def _packed_plan(fr, fw):
    """-> (reason, plan): why the repack path does not apply (None when it does), and the
    arguments of `read_packed` for this pair."""
    from .vdif.base import VDIFStreamReader
    from .mark5b.base import Mark5BStreamReader
    layout = _writer_layout(fw)
    if not isinstance(fr, (VDIFStreamReader, Mark5BStreamReader)) or layout is None:
        return "both ends must be VDIF or Mark 5B streams ({} -> {})".format(type(fr).__name__, type(fw).__name__), None
    coder_out, nthread, nchan = layout
    coder_in, bps, chunk_in, nslot_in, payload_in = fr._packed_geometry()
    if fw.bps != bps:
        return "bits per sample differ ({} -> {})".format(bps, fw.bps), None
    if bool(fw.complex_data) != bool(fr.complex_data):
        return "real and complex samples differ", None
    if _channel_subset(fr):
        return "the reader has a channel subset", None
    chunk_out = nchan * (2 if fw.complex_data else 1)
    if nslot_in * chunk_in != nthread * chunk_out:
        return "a sample has {} components on one side and {} on the other".format(nslot_in * chunk_in,
                                                                                  nthread * chunk_out), None
    spf = fw.samples_per_frame
    if spf * chunk_out * bps % 32:
        return "the writer's payloads are not whole 32-bit words", None
    if not kernels.repack_supported(bps, coder_in, coder_out, chunk_in, nslot_in, chunk_out, nthread,
                                    payload_in, spf * chunk_out * bps // 8):
        return "the repack kernel does not take this pair of coders and frame geometries", None
    if fw._npending:
        return "the writer holds a partial frame", None
    whole = samples_per_byte(min(chunk_in, chunk_out), bps)
    if fr.offset % whole or spf % whole:
        return "the offset is not on a byte boundary of a thread's stream (a multiple of {} samples)".format(whole), None
    fill = _fill_code(fr.fill_value, coder_out, bps)
    if fr.complex_data and fill != _fill_code(0., coder_out, bps):
        return "the fill value's real and imaginary parts encode to different codes", None
    return None, (coder_out, nthread, nchan, spf, fill)


class _Request:
    """The samples a `convert` call still owes: `count` of them from where the reader stood,
    or -- `count` None or negative -- all that the reader holds.  The reader's length is
    asked for again at every piece: a ``verify='fix'`` reader that meets damage locates its
    frames then, and the length is from there on what that index says."""

    def __init__(self, fr, count):
        self.fr, self.start = fr, fr.offset
        self.count = None if count is None or count < 0 else count
        if self.left() < 0:
            raise EOFError("cannot read from beyond end of input.")

    def left(self):
        total = self.fr.shape[0] - self.start if self.count is None else self.count
        return total - (self.fr.offset - self.start)

    def piece(self, most, call, unit=1):
        """``call(n)`` for the next ``n <= most`` samples (whole `unit`s) -> (n, what it returned).
        When the call itself made the reader locate its frames and an open-ended request ends
        earlier for it, the piece is asked for again at its new size (once: frames are located
        once)."""
        n = min(most, self.left()) // unit * unit
        length = self.fr.shape[0]
        try:
            return n, call(n)
        except EOFError:
            if self.count is not None or self.fr.shape[0] == length:
                raise
        n = min(most, self.left()) // unit * unit
        return n, call(n)


def _convert_loop(fr, fw, request):
    """``fw.write(fr.read(spf), valid=v)`` frame after frame, in pieces of many frames:
    runs of frames of equal validity are written with one call.  `fr.frames_valid` stands
    in for the read that follows it -- it repairs or raises where that read would -- so its
    answer is about the samples that read returns."""
    spf = fw.samples_per_frame
    ncomp = int(np.prod(fw._unsliced_shape)) * (2 if fw.complex_data else 1)
    per = max(1, LOOP_PIECE_BYTES // (4 * spf * ncomp))
    while request.left() > 0:
        n, valid = request.piece(per * spf, lambda n: fr.frames_valid(n, spf))
        data = fr.read(n)
        data = data.reshape((data.shape[0],) + fw.sample_shape)
        k = 0
        while k < len(valid):
            e = k + 1
            while e < len(valid) and valid[e] == valid[k]:
                e += 1
            fw.write(data[k * spf:e * spf], valid=bool(valid[k]))
            k = e


def convert(fr, fw, count=None, packed=None):
    """Write the next `count` samples of the stream reader `fr` (default: all that are
    left) to the stream writer `fw`; returns the number of samples converted.

    The file is byte for byte what ::

        d = fr.read(fw.samples_per_frame)
        fw.write(d.reshape((len(d),) + fw.sample_shape), valid=v)

    writes frame after frame, with ``v`` false where a frame draws from a missing or
    invalid frame of `fr` (``fr.frames_valid``) and a tail of less than a frame written
    last.  Between VDIF and Mark 5B streams with the same bits per sample, the same
    real / complex kind and as many components per sample (in C order), without a channel
    `subset`, the samples are never decoded: their packed bytes are rearranged on the
    GPU (`kernels.repack_frames`) in pieces of at most 256 MiB.  ``packed=None`` takes that
    path when it applies, ``packed=False`` never, ``packed=True`` raises
    NotImplementedError naming the reason when it does not.  Mark 4, DADA, GUPPI and GSB
    streams, and conversions that rescale, go through the loop.

    A damaged file is converted as ``read()`` reads it on either path: under
    ``verify='fix'`` the piece that meets the damage has the frames located and is
    answered, samples and validity alike, through that index; under ``verify=True`` it
    raises what the read raises.  Without `count` the request ends where the reader ends
    once its frames are located."""
    request = _Request(fr, count)
    kernels.require_gpu()
    reason, plan = (None, None) if packed is False else _packed_plan(fr, fw)
    if packed and reason is not None:
        raise NotImplementedError("convert(packed=True): " + reason)
    if packed is not False and reason is None:
        coder, nthread, nchan, spf, fill = plan
        payload = spf * nchan * (2 if fw.complex_data else 1) * fw.bps // 8
        per = max(1, PACKED_PIECE_BYTES // (nthread * payload))
        while request.left() >= spf:
            n, (payloads, valid) = request.piece(
                per * spf, lambda n: fr.read_packed(n, coder, nthread, nchan, spf, fill), unit=spf)
            fw._write_packed(payloads, valid)
            fw._nframes_written += n // spf
            fw.offset += n
    _convert_loop(fr, fw, request)              # (everything, or a tail of less than a frame)
    return fr.offset - request.start
