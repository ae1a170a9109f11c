"""ctypes binding of libbbdecode.so (the C ABI declared in include/bbdecode.h).

The library is the only compute path of this package: if it cannot be loaded
the import fails loudly -- there is no NumPy/PyTorch fallback.
"""
import ctypes as C
import os

# PyTorch bundles its own libamdhip64.so.7 / libhsa-runtime64.so.1.  Import it
# BEFORE loading libbbdecode.so so that the dynamic loader resolves our HIP
# dependency (same SONAME) to the runtime torch already initialised: two HIP
# runtimes in one process do not see each other's devices, streams or memory.
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
# BB_EXPERIMENTS=1 in the environment loads the experiment build (make -C
# baseband_amd/csrc EXPERIMENTS=1): the same kernels plus the measurement
# variants and knobs of include/bbdecode_exp.h.  tools/experiments/exp_*.py need it; the
# package, the tests and bench.py run on the product library.
EXPERIMENTS = os.environ.get('BB_EXPERIMENTS', '') not in ('', '0')
LIB_PATH = os.path.join(_HERE, 'libbbdecode_exp.so' if EXPERIMENTS else 'libbbdecode.so')

BB_OK = 0
BB_EIO = -5
BB_EINVAL = -22
BB_ERANGE = -34
BB_ENOTSUP = -95

CODER_VDIF = 0
CODER_MARK5B = 1
CODER_INT = 2

# enum bb_out_type (bb_decode_params.out_type)
OUT_F32 = 0
OUT_F16 = 1
OUT_BF16 = 2

FRAME_OK = 0x1
FRAME_INVALID = 0x2

# include/bbdecode_tune.h (geometry knobs of the product library)
TUNE_BLOCKS = 2
TUNE_TILE_ELEMS = 4
TUNE_ENCODE_DIRECT = 5
TUNE_GATHER_BYTES = 6
TUNE_TILES_PER_WAVE = 7
TUNE_TILED_STAGE = 10
TUNE_MKBF_CHANNELS = 11
TUNE_GATHER_CHUNKS = 12
TUNE_SEG_TILES = 13
TUNE_WORK_STRIPES = 18
TUNE_XPOSE = 19
TUNE_XPOSE_ROWS = 20
TUNE_M4_WIDEN = 22
TUNE_SELECT_BYTES = 23
TUNE_LUT_TILES = 24
TUNE_M4_TILES = 26
TUNE_XPOSE_TC = 27
TUNE_XPOSE_MIN_NC = 28
TUNE_ENCODE_RUNS = 30
TUNE_GATHER_GLDS = 36
TUNE_ENCODE_STRIPES = 38
TUNE_SELECT_PICK = 39
TUNE_PICK_BYTES = 40
TUNE_VDIF8_LDS_GIB = 41
TUNE_TOUCH_MIB = 42
# include/bbdecode_exp.h (experiment build only: bb_tune answers BB_EINVAL otherwise)
TUNE_FLAT_VARIANT = 0
TUNE_NT_STORES = 1
TUNE_NT_LOADS = 3
TUNE_TILES_PER_WAVE_8BIT = 8
TUNE_LDS_PAD = 9
TUNE_FRONT_GROUP = 14
TUNE_FRONT_STEPS = 15
TUNE_OUT_STRIPE_W = 16
TUNE_OUT_STRIPE_S = 17
TUNE_BYTE_LUT = 21
TUNE_LUT_SMALL = 25
TUNE_FLAT8_LDS = 29
TUNE_BURST = 31
TUNE_COPY = 35
TUNE_M4_LDS = 37
TUNE_BURST_BYTES = 32
TUNE_BURST_PERIOD = 33
TUNE_BURST_WAVES = 34


class BBError(RuntimeError):
    def __init__(self, code, where):
        self.code = code
        super().__init__("{}: {} (code {}, hip error {})".format(
            where, lib.bb_strerror(code).decode(), code, lib.bb_last_hip_error()))


class FrameRec(C.Structure):
    _fields_ = [('payload_offset', C.c_int64), ('time_index', C.c_int32),
                ('thread_id', C.c_int16), ('flags', C.c_uint16)]


class VDIFScanParams(C.Structure):
    _fields_ = [('first_offset', C.c_uint64), ('frame_nbytes', C.c_uint32),
                ('header_nbytes', C.c_uint32), ('pattern', C.c_uint32 * 8),
                ('mask', C.c_uint32 * 8), ('ref_seconds', C.c_int32),
                ('ref_frame_nr', C.c_int32), ('frame_rate', C.c_int32),
                ('set_nframes', C.c_int32)]


class Mark5BScanParams(C.Structure):
    _fields_ = [('first_offset', C.c_uint64), ('ref_seconds', C.c_int32),
                ('ref_frame_nr', C.c_int32), ('frame_rate', C.c_int32),
                ('by_position', C.c_int32)]


class DecodeParams(C.Structure):
    _fields_ = [('coder', C.c_int32), ('bps', C.c_int32), ('chunk', C.c_int32),
                ('nslot', C.c_int32), ('payload_nbytes', C.c_uint64),
                ('src0', C.c_int64), ('src_stride', C.c_int64),
                ('complex_data', C.c_int32), ('fill_re', C.c_float),
                ('fill_im', C.c_float), ('out_type', C.c_int32)]


class StatesParams(C.Structure):
    _fields_ = [('bps', C.c_int32), ('chunk', C.c_int32), ('nslot', C.c_int32),
                ('reserved', C.c_int32), ('payload_nbytes', C.c_uint64),
                ('src0', C.c_int64), ('src_stride', C.c_int64),
                ('row_lo', C.c_uint64), ('row_hi', C.c_uint64)]


class MomentsParams(C.Structure):
    _fields_ = [('layout', C.c_int32), ('npol', C.c_int32), ('nchan', C.c_int32), ('ncomp', C.c_int32),
                ('ntime', C.c_uint64), ('t_lo', C.c_uint64), ('t_hi', C.c_uint64),
                ('src0', C.c_int64), ('src_stride', C.c_int64),
                ('bin_rows', C.c_uint64), ('first_row', C.c_uint64), ('nbins', C.c_uint64)]


class RepackParams(C.Structure):
    _fields_ = [('bps', C.c_int32), ('coder_in', C.c_int32), ('coder_out', C.c_int32),
                ('chunk_in', C.c_int32), ('nslot_in', C.c_int32), ('chunk_out', C.c_int32),
                ('nslot_out', C.c_int32), ('fill_code', C.c_int32),
                ('payload_in', C.c_uint64), ('payload_out', C.c_uint64),
                ('src0', C.c_int64), ('src_stride', C.c_int64),
                ('row_lo', C.c_uint64), ('row_hi', C.c_uint64), ('first_row', C.c_uint64),
                ('reserved', C.c_uint64)]


class RequantParams(C.Structure):
    _fields_ = [('bps_in', C.c_int32), ('bps_out', C.c_int32), ('chunk', C.c_int32),
                ('nslot', C.c_int32), ('fill_code', C.c_int32), ('reserved', C.c_int32),
                ('payload_in', C.c_uint64), ('payload_out', C.c_uint64),
                ('src0', C.c_int64), ('src_stride', C.c_int64),
                ('row_lo', C.c_uint64), ('row_hi', C.c_uint64), ('first_row', C.c_uint64),
                ('map', C.c_uint8 * 256)]


class RecodeParams(C.Structure):
    _fields_ = [('bps_in', C.c_int32), ('bps_out', C.c_int32), ('chunk_in', C.c_int32),
                ('nslot_in', C.c_int32), ('chunk_out', C.c_int32), ('nslot_out', C.c_int32),
                ('fill_code', C.c_int32), ('reserved', C.c_int32),
                ('payload_in', C.c_uint64), ('payload_out', C.c_uint64),
                ('src0', C.c_int64), ('src_stride', C.c_int64),
                ('row_lo', C.c_uint64), ('row_hi', C.c_uint64), ('first_row', C.c_uint64),
                ('map', C.c_uint8 * 256)]


class Mark4ScanParams(C.Structure):
    _fields_ = [('first_offset', C.c_uint64), ('ntrack', C.c_int32),
                ('ref_year', C.c_int32), ('ref_qms', C.c_int64),
                ('frame_qms', C.c_int32), ('by_position', C.c_int32)]


class Mark4DecodeParams(C.Structure):
    _fields_ = [('ntrack', C.c_int32), ('out_type', C.c_int32),
                ('nwords', C.c_uint64), ('fill_words', C.c_uint64),
                ('src0', C.c_int64), ('src_stride', C.c_int64),
                ('sign_bit', C.c_uint8 * 32), ('mag_bit', C.c_uint8 * 32),
                ('fill', C.c_float), ('reserved2', C.c_int32)]


class TiledParams(C.Structure):
    _fields_ = [('layout', C.c_int32), ('npol', C.c_int32), ('nchan', C.c_int32),
                ('nchan_stored', C.c_int32), ('ntime', C.c_uint64),
                ('t_lo', C.c_uint64), ('t_hi', C.c_uint64),
                ('src0', C.c_int64), ('src_stride', C.c_int64),
                ('fill_re', C.c_float), ('fill_im', C.c_float),
                ('npol_stored', C.c_int32), ('pol_first', C.c_int32), ('d_chan_map', C.c_void_p)]


class ArenaStats(C.Structure):
    _fields_ = [('base', C.c_uint64), ('capacity', C.c_uint64), ('bytes_backed', C.c_uint64),
                ('bytes_in_use', C.c_uint64), ('largest_free', C.c_uint64), ('bytes_grown', C.c_uint64),
                ('bytes_trimmed', C.c_uint64), ('chunk_bytes', C.c_uint32), ('steps', C.c_uint32),
                ('blocks', C.c_uint32), ('probes', C.c_uint32), ('last_probe_gbps', C.c_double), ('create_ms', C.c_double),
                ('grow_ms', C.c_double), ('va_reserved', C.c_uint64), ('va_used', C.c_uint64),
                ('va_ranges', C.c_uint32), ('va_ranges_made', C.c_uint32), ('prepares', C.c_uint32),
                ('growing', C.c_uint32), ('prepare_ms', C.c_double), ('prepare_wait_ms', C.c_double),
                ('first_probe_gbps', C.c_double), ('last_create_ms', C.c_double),
                ('second_chances', C.c_uint32), ('second_chance_wins', C.c_uint32),
                ('second_chances_no_room', C.c_uint32), ('probe_history_n', C.c_uint32),
                ('probe_history', C.c_uint16 * 16)]


LAYOUT_GUPPI_CF = 0
LAYOUT_MKBF = 1
LAYOUT_GUPPI_TF = 2

# enum bb_moments_layout (bb_i8_moments; not the layouts of bb_decode_i8_tiled)
MOMENTS_GUPPI_CF = 0
MOMENTS_GUPPI_TF = 1
MOMENTS_ROWS = 2
MOMENTS_MKBF = 3


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "baseband_amd: {} not found. Build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` or "
            "`make -C baseband_amd/csrc{}` (needs hipcc, gfx950). There is no "
            "CPU fallback.".format(LIB_PATH, ' EXPERIMENTS=1' if EXPERIMENTS else ''))
    return C.CDLL(LIB_PATH)


lib = _load()

_vp = C.c_void_p
_sz = C.c_size_t

# (name, restype, argtypes) -- must list every symbol of include/bbdecode.h
# include/bbdecode_tune.h and include/bbdecode_arena.h
SIGNATURES = [
    ('bb_abi_version', C.c_int, []),
    ('bb_strerror', C.c_char_p, [C.c_int]),
    ('bb_last_hip_error', C.c_int, []),
    ('bb_last_kernel', C.c_char_p, []),
    ('bb_init', C.c_int, []),
    ('bb_get_levels', C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_float), _sz]),
    ('bb_get_levels_as', C.c_int, [C.c_int, C.c_int, C.c_int, _vp, _sz]),
    ('bb_decode_out_check', C.c_int, [C.POINTER(DecodeParams)]),
    ('bb_get_encode_thresholds', C.c_int, [C.POINTER(C.c_float)]),
    ('bb_vdif_scan', C.c_int, [_vp, _sz, C.POINTER(VDIFScanParams), _vp, _sz, _vp]),
    ('bb_vdif_locate', C.c_int, [_vp, _sz, C.POINTER(VDIFScanParams), _vp, _sz, _vp, _vp]),
    ('bb_vdif_scan_at', C.c_int, [_vp, _sz, C.POINTER(VDIFScanParams), _vp, _sz, _vp, _vp]),
    ('bb_mark5b_scan', C.c_int, [_vp, _sz, C.POINTER(Mark5BScanParams), _vp, _sz, _vp]),
    ('bb_touch', C.c_int, [_vp, _sz, _vp]),
    ('bb_mark5b_locate', C.c_int, [_vp, _sz, _vp, _sz, _vp, _vp]),
    ('bb_mark5b_locate_stream', C.c_int, [_vp, _sz, C.c_uint32, C.c_uint32, _vp, _sz, _vp, _vp]),
    ('bb_mark5b_scan_at', C.c_int, [_vp, _sz, C.POINTER(Mark5BScanParams), _vp, _sz, _vp, _vp]),
    ('bb_verify_records', C.c_int, [_vp, _sz, C.c_int32, C.c_uint32, _sz, _vp, _vp]),
    ('bb_build_index', C.c_int, [_vp, _sz, _vp, C.c_int, _vp, _sz, _vp]),
    ('bb_decode_frames', C.c_int, [_vp, _sz, _vp, _sz, C.POINTER(DecodeParams), _vp, _sz, _vp]),
    ('bb_decode_frames_select', C.c_int, [_vp, _sz, _vp, _sz, C.POINTER(DecodeParams), _vp, C.c_int, _vp, _sz, _vp]),
    ('bb_decode_frames_select_check', C.c_int, [C.POINTER(DecodeParams), C.c_int]),
    ('bb_copy_frames', C.c_int, [_vp, _sz, _sz, C.c_uint64, C.c_int64, C.c_int64, _vp, _sz, _vp]),
    ('bb_count_states', C.c_int, [_vp, _sz, _vp, _sz, C.POINTER(StatesParams), _vp, _sz, _vp]),
    ('bb_count_states_check', C.c_int, [C.POINTER(StatesParams)]),
    ('bb_count_states_bins', C.c_int, [_vp, _sz, _vp, _sz, C.POINTER(StatesParams), C.c_uint64, C.c_uint64,
                                       C.c_uint64, _vp, _sz, _vp]),
    ('bb_count_states_bins_check', C.c_int, [C.POINTER(StatesParams), C.c_uint64]),
    ('bb_i8_moments', C.c_int, [_vp, _sz, _vp, _sz, C.POINTER(MomentsParams), _vp, _sz, _vp]),
    ('bb_i8_moments_check', C.c_int, [C.POINTER(MomentsParams)]),
    ('bb_i8_coherence', C.c_int, [_vp, _sz, _vp, _sz, C.POINTER(MomentsParams), _vp, _sz, _vp]),
    ('bb_i8_coherence_check', C.c_int, [C.POINTER(MomentsParams)]),
    ('bb_repack_frames', C.c_int, [_vp, _sz, _vp, _sz, C.POINTER(RepackParams), _vp, _sz, _vp]),
    ('bb_repack_check', C.c_int, [C.POINTER(RepackParams)]),
    ('bb_requant_frames', C.c_int, [_vp, _sz, _vp, _sz, C.POINTER(RequantParams), _vp, _sz, _vp]),
    ('bb_requant_check', C.c_int, [C.POINTER(RequantParams)]),
    ('bb_recode_frames', C.c_int, [_vp, _sz, _vp, _sz, C.POINTER(RecodeParams), _vp, _sz, _vp]),
    ('bb_recode_check', C.c_int, [C.POINTER(RecodeParams)]),
    ('bb_recode_frames_tables', C.c_int, [_vp, _sz, _vp, _sz, C.POINTER(RecodeParams), _vp, _sz, _vp, _sz, _vp]),
    ('bb_recode_tables_check', C.c_int, [C.POINTER(RecodeParams)]),
    ('bb_fetch_counter', C.c_int, [_vp, _vp, _vp, _vp]),
    ('bb_mark5b_read_window', C.c_int, [_vp, _sz, C.POINTER(Mark5BScanParams), _sz, _sz, C.POINTER(DecodeParams),
                                        _vp, C.c_int, _vp, _vp, _vp, _sz, _sz, _vp, _vp, _vp, _vp]),
    ('bb_mark4_read_window', C.c_int, [_vp, _sz, C.POINTER(Mark4ScanParams), _sz, _sz,
                                       C.POINTER(Mark4DecodeParams), C.c_int, _vp, _vp, _vp, _sz, _sz, _vp, _vp,
                                       _vp, _vp]),
    ('bb_vdif_read_window', C.c_int, [_vp, _sz, C.POINTER(VDIFScanParams), _sz, _vp, _sz, C.POINTER(DecodeParams),
                                      _vp, C.c_int, _vp, _vp, _vp, _sz, C.c_uint32, _sz, _vp, _vp, _vp, _vp]),
    ('bb_mark4_scan', C.c_int, [_vp, _sz, C.POINTER(Mark4ScanParams), _vp, _sz, _vp]),
    ('bb_mark4_locate', C.c_int, [_vp, _sz, C.c_int, _vp, _sz, _vp, _vp]),
    ('bb_mark4_header_crc', C.c_int, [_vp, _sz, C.c_int, _vp, C.c_int64, _sz, _vp, _vp]),
    ('bb_mark4_scan_at', C.c_int, [_vp, _sz, C.POINTER(Mark4ScanParams), _vp, _sz, _vp, _vp]),
    ('bb_decode_mark4', C.c_int, [_vp, _sz, _vp, _sz, C.POINTER(Mark4DecodeParams), _vp, _sz, _vp]),
    ('bb_decode_mark4_select', C.c_int, [_vp, _sz, _vp, _sz, C.POINTER(Mark4DecodeParams), C.c_int,
                                         _vp, _sz, _vp]),
    ('bb_decode_i8_tiled', C.c_int, [_vp, _sz, _vp, _sz, C.POINTER(TiledParams), _vp, _sz, _vp]),
    ('bb_encode_flat', C.c_int, [_vp, _sz, C.c_int, C.c_int, _vp, _sz, _vp]),
    ('bb_encode_mark4', C.c_int, [_vp, _sz, C.c_int, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), _vp, _sz, _vp]),
    ('bb_tune', C.c_int, [C.c_int, C.c_int]),
    # include/bbdecode_arena.h
    ('bb_arena_create', C.c_int, [_sz, C.POINTER(_vp)]),
    ('bb_arena_alloc', C.c_int, [_vp, _sz, C.POINTER(_vp)]),
    ('bb_arena_prepare', C.c_int, [_vp, _sz]),
    ('bb_arena_owns', C.c_int, [_vp, _vp]),
    ('bb_arena_free', C.c_int, [_vp, _vp]),
    ('bb_arena_trim', C.c_int, [_vp, C.POINTER(_sz)]),
    ('bb_arena_get_stats', C.c_int, [_vp, C.POINTER(ArenaStats)]),
    ('bb_arena_destroy', C.c_int, [_vp]),
]

# include/bbdecode_exp.h
EXPERIMENT_SIGNATURES = [
    ('bb_debug_trace', C.c_int, [_vp]),
    ('bb_host_register', C.c_int, [_vp, _sz]),
    ('bb_host_unregister', C.c_int, [_vp]),
    ('bb_copy_to_device', C.c_int, [_vp, _vp, _sz, _vp]),
]

for _name, _res, _args in SIGNATURES + (EXPERIMENT_SIGNATURES if EXPERIMENTS else []):
    _f = getattr(lib, _name)
    _f.restype = _res
    _f.argtypes = _args


def check(code, where):
    if code != BB_OK:
        if code == BB_ENOTSUP:
            # the reference surfaces an unknown coder as KeyError from the
            # _decoders dict (base/payload.py:314-315)
            raise KeyError("{}: unsupported coder / bits per sample".format(where))
        raise BBError(code, where)


def last_kernel():
    """Name / template arguments / grid of the decode kernel this thread
    launched last (bb_last_kernel)."""
    return lib.bb_last_kernel().decode()


def get_levels(coder, bps):
    """Host copy of the code -> level table the kernels use."""
    import numpy as np
    n = 1 << bps
    out = np.empty(n, dtype=np.float32)
    check(lib.bb_get_levels(coder, bps, out.ctypes.data_as(C.POINTER(C.c_float)), n),
          'bb_get_levels')
    return out


def states_params(bps, chunk=1, nslot=1, payload_nbytes=4, src0=0, src_stride=0, row_lo=0, row_hi=0, reserved=0):
    p = StatesParams()
    p.bps, p.chunk, p.nslot, p.reserved = bps, chunk, nslot, reserved
    p.payload_nbytes, p.src0, p.src_stride = payload_nbytes, src0, src_stride
    p.row_lo, p.row_hi = row_lo, row_hi
    return p


def count_states_check(bps, chunk=1, nslot=1, payload_nbytes=4, row_lo=0, row_hi=0, reserved=0):
    """What `bb_count_states` would answer to these parameters, as far as they decide it
    (bb_count_states_check: no buffers, no device): BB_OK, BB_EINVAL or BB_ENOTSUP."""
    p = states_params(bps, chunk, nslot, payload_nbytes, 0, 0, row_lo, row_hi, reserved)
    return lib.bb_count_states_check(C.byref(p))


def count_states_bins_check(bps, chunk=1, bin_rows=8, nslot=1, payload_nbytes=4, row_lo=0, row_hi=0, reserved=0):
    """What `bb_count_states_bins` would answer to these parameters, as far as they decide
    it (bb_count_states_bins_check: no buffers, no device): BB_OK, BB_EINVAL or BB_ENOTSUP."""
    p = states_params(bps, chunk, nslot, payload_nbytes, 0, 0, row_lo, row_hi, reserved)
    return lib.bb_count_states_bins_check(C.byref(p), bin_rows)


def moments_params(layout, npol, nchan, ncomp, ntime, t_lo=0, t_hi=0, bin_rows=1, nbins=0, first_row=0,
                   src0=0, src_stride=0):
    p = MomentsParams()
    p.layout, p.npol, p.nchan, p.ncomp = layout, npol, nchan, ncomp
    p.ntime, p.t_lo, p.t_hi = ntime, t_lo, t_hi
    p.src0, p.src_stride = src0, src_stride
    p.bin_rows, p.first_row, p.nbins = bin_rows, first_row, nbins
    return p


def i8_moments_check(layout, npol, nchan, ncomp, ntime, t_lo=0, t_hi=0, bin_rows=1, src0=0, src_stride=0):
    """What `bb_i8_moments` would answer to these parameters, as far as they decide it
    (bb_i8_moments_check: no buffers, no device): BB_OK, BB_EINVAL or BB_ENOTSUP."""
    p = moments_params(layout, npol, nchan, ncomp, ntime, t_lo, t_hi, bin_rows, 0, 0, src0, src_stride)
    return lib.bb_i8_moments_check(C.byref(p))


def i8_coherence_check(layout, npol, nchan, ncomp, ntime, t_lo=0, t_hi=0, bin_rows=1, src0=0, src_stride=0):
    """What `bb_i8_coherence` would answer to these parameters, as far as they decide it
    (bb_i8_coherence_check: no buffers, no device): BB_OK, BB_EINVAL or BB_ENOTSUP."""
    p = moments_params(layout, npol, nchan, ncomp, ntime, t_lo, t_hi, bin_rows, 0, 0, src0, src_stride)
    return lib.bb_i8_coherence_check(C.byref(p))


def repack_params(bps, coder_in, coder_out, chunk_in, nslot_in, chunk_out, nslot_out, payload_in, payload_out,
                  fill_code=0, src0=0, src_stride=0, row_lo=0, row_hi=0, first_row=0, reserved=0):
    p = RepackParams()
    p.bps, p.coder_in, p.coder_out, p.fill_code = bps, coder_in, coder_out, fill_code
    p.chunk_in, p.nslot_in, p.chunk_out, p.nslot_out = chunk_in, nslot_in, chunk_out, nslot_out
    p.payload_in, p.payload_out, p.src0, p.src_stride = payload_in, payload_out, src0, src_stride
    p.row_lo, p.row_hi, p.first_row, p.reserved = row_lo, row_hi, first_row, reserved
    return p


def repack_check(bps, coder_in, coder_out, chunk_in, nslot_in, chunk_out, nslot_out, payload_in, payload_out,
                 fill_code=0, row_lo=0, row_hi=0, first_row=0, reserved=0):
    """What `bb_repack_frames` would answer to these parameters, as far as they decide it
    (bb_repack_check: no buffers, no device): BB_OK, BB_EINVAL or BB_ENOTSUP."""
    p = repack_params(bps, coder_in, coder_out, chunk_in, nslot_in, chunk_out, nslot_out, payload_in, payload_out,
                      fill_code, 0, 0, row_lo, row_hi, first_row, reserved)
    return lib.bb_repack_check(C.byref(p))


def _set_table(p, table, name):
    """`table` -> the `map` of a parameter block: at most 256 codes of 0 .. 255 (the rest are 0)."""
    import numpy as np
    codes = np.asarray(table if isinstance(table, np.ndarray) else list(table), dtype=np.int64).reshape(-1)
    if codes.size > 256 or ((codes < 0) | (codes > 255)).any():
        raise ValueError("{}: a table is at most 256 codes of 0 .. 255".format(name))
    full = np.zeros(256, np.uint8)
    full[:codes.size] = codes
    C.memmove(p.map, full.ctypes.data, 256)
    return p


def requant_params(bps_in, bps_out, chunk, nslot, payload_in, payload_out, table=(), fill_code=0, src0=0,
                   src_stride=0, row_lo=0, row_hi=0, first_row=0, reserved=0):
    """`table`: output code by input code, at most 256 entries of 0 .. 255 (the rest are 0)."""
    p = RequantParams()
    p.bps_in, p.bps_out, p.chunk, p.nslot, p.fill_code, p.reserved = bps_in, bps_out, chunk, nslot, fill_code, reserved
    p.payload_in, p.payload_out, p.src0, p.src_stride = payload_in, payload_out, src0, src_stride
    p.row_lo, p.row_hi, p.first_row = row_lo, row_hi, first_row
    return _set_table(p, table, 'requant_params')


def requant_check(bps_in, bps_out, chunk, nslot, payload_in, payload_out, table=(), fill_code=0,
                  row_lo=0, row_hi=0, first_row=0, reserved=0):
    """What `bb_requant_frames` would answer to these parameters, as far as they decide it
    (bb_requant_check: no buffers, no device): BB_OK, BB_EINVAL or BB_ENOTSUP."""
    p = requant_params(bps_in, bps_out, chunk, nslot, payload_in, payload_out, table, fill_code, 0, 0,
                       row_lo, row_hi, first_row, reserved)
    return lib.bb_requant_check(C.byref(p))


def recode_params(bps_in, bps_out, chunk_in, nslot_in, chunk_out, nslot_out, payload_in, payload_out, table=(),
                  fill_code=0, src0=0, src_stride=0, row_lo=0, row_hi=0, first_row=0, reserved=0):
    """`table`: output code by input code, at most 256 entries of 0 .. 255 (the rest are 0)."""
    p = RecodeParams()
    p.bps_in, p.bps_out, p.fill_code, p.reserved = bps_in, bps_out, fill_code, reserved
    p.chunk_in, p.nslot_in, p.chunk_out, p.nslot_out = chunk_in, nslot_in, chunk_out, nslot_out
    p.payload_in, p.payload_out, p.src0, p.src_stride = payload_in, payload_out, src0, src_stride
    p.row_lo, p.row_hi, p.first_row = row_lo, row_hi, first_row
    return _set_table(p, table, 'recode_params')


def recode_check(bps_in, bps_out, chunk_in, nslot_in, chunk_out, nslot_out, payload_in, payload_out, table=(),
                 fill_code=0, row_lo=0, row_hi=0, first_row=0, reserved=0):
    """What `bb_recode_frames` would answer to these parameters, as far as they decide it
    (bb_recode_check: no buffers, no device): BB_OK, BB_EINVAL or BB_ENOTSUP."""
    p = recode_params(bps_in, bps_out, chunk_in, nslot_in, chunk_out, nslot_out, payload_in, payload_out, table,
                      fill_code, 0, 0, row_lo, row_hi, first_row, reserved)
    return lib.bb_recode_check(C.byref(p))


def recode_tables_check(bps_in, bps_out, chunk_in, nslot_in, chunk_out, nslot_out, payload_in, payload_out,
                        fill_code=0, row_lo=0, row_hi=0, first_row=0, reserved=0):
    """What `bb_recode_frames_tables` would answer to these parameters, as far as they decide it
    (bb_recode_tables_check: no buffers, no device; the block's own map stays zero)."""
    p = recode_params(bps_in, bps_out, chunk_in, nslot_in, chunk_out, nslot_out, payload_in, payload_out, (),
                      fill_code, 0, 0, row_lo, row_hi, first_row, reserved)
    return lib.bb_recode_tables_check(C.byref(p))


def out_type_of(dtype):
    """torch dtype of decoded samples -> enum bb_out_type (complex types count as
    their (re, im) element type); None for a type the library does not write."""
    return {torch.float32: OUT_F32, torch.complex64: OUT_F32, torch.float16: OUT_F16,
            torch.complex32: OUT_F16, torch.bfloat16: OUT_BF16}.get(dtype)


def levels_as(coder, bps, out_type):
    """Host copy of the code -> level table in an output type: float32 values for
    OUT_F32, uint16 bit patterns for OUT_F16 / OUT_BF16 (bb_get_levels_as)."""
    import numpy as np
    n = 1 << bps
    out = np.empty(n, dtype=np.float32 if out_type == OUT_F32 else np.uint16)
    check(lib.bb_get_levels_as(coder, bps, out_type, out.ctypes.data_as(_vp), n), 'bb_get_levels_as')
    return out


def encode_thresholds():
    """float32[3]: inputs at which the 2-bit encoder steps to code 1, 2, 3."""
    import numpy as np
    out = np.empty(3, np.float32)
    check(lib.bb_get_encode_thresholds(out.ctypes.data_as(C.POINTER(C.c_float))),
          'bb_get_encode_thresholds')
    return out
