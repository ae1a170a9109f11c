/*
 * bbdecode.h -- C ABI of libbbdecode.so: MI355X (gfx950) frame-index scan and
 * packed-sample decode for radio-baseband formats (VDIF, Mark 5B, Mark 4,
 * GUPPI, DADA, GSB).
 *
 * This is the drop-in boundary for the hot path of mhvk/baseband
 * (open().read() -> Payload.fromfile -> Payload.data).  Every entry point
 * cites the reference interface (path:line relative to the reference tree)
 * it replaces.  The reference is pure Python; the seam a maintainer would bind
 * is PayloadBase._decoders (base/payload.py:50,314-315) plus the per-frame
 * header reads of the stream readers (base/base.py:919-1125).  See
 * INTEGRATION.md for the ctypes stub.
 *
 * Conventions
 *  - plain pointers and sizes only; all `d_*` pointers are DEVICE pointers
 *    (hipMalloc'ed or equivalent); `stream` is a hipStream_t passed as void*
 *    (NULL = the default stream).
 *  - every function of THIS header is stream-ordered and asynchronous w.r.t.
 *    the host, never allocates and never synchronises (graph-capturable).
 *    State the library keeps: the constant level tables uploaded once per
 *    device by bb_init(); per host thread, the name of the last kernel
 *    (bb_last_kernel), the last HIP error, and the geometry overrides a test or
 *    benchmark sets with bb_tune (bbdecode_tune.h: thread-local, they change
 *    the calling thread's later launches only and never a result).  No
 *    process-wide knobs.  The output arena (bbdecode_arena.h) is a separate
 *    object its creator owns: bb_arena_alloc may map memory and time a probe
 *    launch, i.e. it does synchronise -- see that header.
 *  - return value 0 = success, negative errno-style code otherwise.  No
 *    exceptions cross the ABI.  The Python host maps BB_ENOTSUP to KeyError
 *    (the reference surfaces an unknown coder as KeyError from the _decoders
 *    dict, base/payload.py:314-315).
 *  - decoded output is float32; complex64 is (re, im) interleaved float32.
 *    bb_decode_frames and the VDIF / Mark 5B window calls can instead write
 *    float16 or bfloat16 elements (bb_decode_params.out_type): the float32
 *    value rounded once to nearest even, (re, im) interleaved likewise.
 */
#ifndef BBDECODE_H
#define BBDECODE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BB_ABI_VERSION 7   /* 7, additive: bb_count_states, bb_count_states_check, bb_states_params (sampler statistics; nothing else changed) */   /* 7, additive: bb_decode_params.reserved became out_type (zero = float32, the old behaviour; same layout), bb_mark4_decode_params.reserved likewise (float32 only), bb_decode_out_check, bb_get_levels_as */   /* 7 (round 6): bb_touch; the *_read_window calls read small windows through first */   /* 6 (round 6): bb_mark5b_locate_stream */   /* 5 (round 6): bb_arena_stats grew (first_probe_gbps .. second_chance_wins) */   /* 4 (round 5): bb_arena_prepare, bb_arena_owns, bb_arena_stats grew (va_ranges .. prepare_wait_ms); the `reserved` words of the scan parameter blocks got meanings whose zero is the old behaviour (bb_vdif_scan_params.set_nframes, bb_mark5b_/bb_mark4_scan_params.by_position): same layout  */   /* 3 (round 4): bb_copy_frames; bb_arena_stats grew va_reserved / va_used; bb_tune knobs are thread-local */   /* 2: bb_tiled_params grew (npol_stored, pol_first, d_chan_map) */

/* error codes (negative errno values) */
#define BB_OK        0
#define BB_EIO      (-5)   /* a HIP runtime call failed (see bb_last_hip_error) */
#define BB_EINVAL   (-22)  /* bad argument (size, alignment, null pointer) */
#define BB_ERANGE   (-34)  /* output buffer too small / index out of range */
#define BB_ENOTSUP  (-95)  /* unsupported coder / bps / mode (-> KeyError) */

/*
 * Sample coders.  A coder plus bits-per-sample selects the code -> float32
 * level table.
 *   BB_CODER_VDIF    offset binary, LSB-first fields
 *                    (vdif/payload.py:25-103; base/encoding.py:52-56,131-144)
 *                    bps 1: {-1,+1}; 2: {-Hi,-1,+1,+Hi}; 4: (n-8)/2.95;
 *                    8: (n-127.5)/35.5   (true float32 division)
 *   BB_CODER_MARK5B  sign/magnitude (mark5b/payload.py:27-94); also VDIF
 *                    EDV 0xab (vdif/payload.py:151-154)
 *                    bps 1: bit ? -1 : +1; 2: field f -> {-Hi,+1,-1,+Hi}[f]
 *   BB_CODER_INT     two's complement integers cast to float32
 *                    bps 8: int8 (dada/payload.py:13-14, guppi/payload.py:13-14,
 *                    gsb/payload.py:39-42); bps 4: sign-extended nibbles, low
 *                    nibble first (gsb/payload.py:24-36)
 */
enum bb_coder {
    BB_CODER_VDIF   = 0,
    BB_CODER_MARK5B = 1,
    BB_CODER_INT    = 2
};

/*
 * Element type of decoded output (bb_decode_params.out_type).  The 16-bit types
 * hold the float32 value the reference produces (base/payload.py:314-330 with the
 * tables of vdif/payload.py:25-103, mark5b/payload.py:27-94, base/encoding.py:
 * 131-144) rounded once to nearest even: every sample value of the 1-, 2-, 4-bit
 * and int8 coders is a table entry, so the library converts the tables (and the
 * fill value) once on the host and the kernels move 16-bit patterns.
 */
enum bb_out_type {
    BB_OUT_F32  = 0,    /* float32 (the default: the word was `reserved`, zero) */
    BB_OUT_F16  = 1,    /* IEEE binary16 */
    BB_OUT_BF16 = 2     /* bfloat16 */
};

/* flags in bb_frame_rec.flags */
#define BB_FRAME_OK       0x0001u  /* header matches the stream invariants */
#define BB_FRAME_INVALID  0x0002u  /* frame carries invalid data -> fill_value */

/*
 * One record per frame found by a header scan, in file order.
 * Replaces the (header, file offset) pairs the reference keeps implicitly
 * while walking a file (vdif/frame.py:176-243, base/base.py:1083-1125).
 */
typedef struct bb_frame_rec {
    int64_t  payload_offset;  /* byte offset of the payload in the scanned buffer */
    int32_t  time_index;      /* frame(set) index relative to header0
                                 (vdif/base.py:386-390; mark5b/base.py:206-213) */
    int16_t  thread_id;       /* VDIF thread_id; 0 for other formats */
    uint16_t flags;           /* BB_FRAME_* */
} bb_frame_rec;

/* ---- library ---------------------------------------------------------- */

int         bb_abi_version(void);
const char *bb_strerror(int code);
/* hipError_t of the last failing HIP call on this host thread (0 if none) */
int         bb_last_hip_error(void);
/* Name, template arguments and grid of the decode kernel the calling thread
 * launched last through bb_decode_frames / bb_decode_mark4 /
 * bb_decode_i8_tiled ("" before the first launch).  The dispatcher picks
 * kernels by geometry; benchmarks and profiles report what actually ran
 * instead of assuming it.  The string is thread-local and valid until the
 * thread's next decode call.  (No reference counterpart: the reference's
 * decoders are Python callables, base/payload.py:314-315.) */
const char *bb_last_kernel(void);
/* Upload the constant level tables to the current device.  Called lazily by
 * every launch entry point; exported so hosts can front-load it.  Fails with
 * BB_EIO when no usable gfx950 device/code object is present: there is no
 * CPU fallback in this library. */
int         bb_init(void);
/* Copy the 2^bps-entry code -> level table of (coder, bps) to host memory
 * (what vdif/payload.py:25-63 and mark5b/payload.py:27-72 tabulate per byte). */
int         bb_get_levels(int coder, int bps, float *h_levels, size_t n);
/* The same table in an output type (enum bb_out_type): 2^bps uint16 bit patterns
 * for BB_OUT_F16 / BB_OUT_BF16, float32 for BB_OUT_F32 (then bb_get_levels).  The
 * single place where the 16-bit types are rounded (nearest even, on the host);
 * stands for the tables of vdif/payload.py:25-103, mark5b/payload.py:27-94 and
 * decode_8bit (base/encoding.py:131-144) followed by ndarray.astype.  No device
 * needed.  BB_EINVAL for an unknown type. */
int         bb_get_levels_as(int coder, int bps, int out_type, void *h_levels, size_t n);
/* The three float32 inputs at which the 2-bit encoder (encode_2bit_base,
 * base/encoding.py:77-102) steps to code 1, 2, 3: code(x) = #{k : x >= thr[k]}.
 * Found on the host by bisection over the reference arithmetic. */
int         bb_get_encode_thresholds(float h_thr[3]);

/* ---- frame index: header scan ------------------------------------------ */

/*
 * VDIF header scan: VDIFHeader.fromfile + verify + _get_index for every frame
 * of a fixed-stride file image (vdif/header.py:158-186,569-589;
 * vdif/base.py:386-390), and the stream-invariant match of
 * base/header.py:588-638 used by locate_frames (base/base.py:181-335).
 * Frame k is expected at first_offset + k*frame_nbytes.
 */
typedef struct bb_vdif_scan_params {
    uint64_t first_offset;    /* byte offset of the first header */
    uint32_t frame_nbytes;    /* header + payload */
    uint32_t header_nbytes;   /* 32, or 16 for legacy headers */
    uint32_t pattern[8];      /* header0 words */
    uint32_t mask[8];         /* 1-bits = stream-invariant header bits */
    int32_t  ref_seconds;     /* header0['seconds'] */
    int32_t  ref_frame_nr;    /* header0['frame_nr'] */
    int32_t  frame_rate;      /* frames per second per thread (integer Hz) */
    int32_t  set_nframes;     /* frames per frame set in file order (threads in the file), 0 or 1: every
                               * frame is placed by its own seconds.  With n > 1 the frames at positions
                               * k*n .. k*n+n-1 from first_offset form a set as VDIFFrameSet.fromfile
                               * builds it (vdif/frame.py:201-243): a frame whose frame_nr equals that of
                               * the set's FIRST frame belongs to the set and takes its time index, whatever
                               * its own seconds say ("we cannot always rely on header['seconds']": VLBA
                               * files whose threads carry different seconds, sample_vlbi.vdif).
                               * bb_vdif_read_window sets it from recs_per_index. */
} bb_vdif_scan_params;

/* Records (bb_vdif_scan and bb_vdif_scan_at): payload_offset = frame offset +
 * header_nbytes.  A header word whose four bytes do not all lie inside the
 * buffer reads as zero.  BB_FRAME_OK: the whole header lies inside the buffer
 * and agrees with `pattern` under `mask`, and the whole frame fits.
 * BB_FRAME_INVALID: the header's invalid bit.  time_index = (seconds -
 * ref_seconds) * frame_rate + frame_nr - ref_frame_nr (the set_nframes rule
 * applies to bb_vdif_scan only), or the frame's number in the call when
 * frame_rate = 0; clamped to +-(2^31 - 1). */
int bb_vdif_scan(const void *d_buf, size_t nbytes,
                 const bb_vdif_scan_params *params,
                 bb_frame_rec *d_recs, size_t nframes, void *stream);

/*
 * Corruption-tolerant frame discovery: byte-granular
 * search for VDIF headers -- the masked-pattern search of
 * VLBIFileReaderBase.locate_frames (base/base.py:181-335) that the reference's
 * _bad_frame recovery relies on (vdif/base.py:536-755).  "A header stands at
 * q" means: the header_nbytes bytes at q lie inside the buffer and agree with
 * `pattern` under `mask`.  A position p is reported when a header stands at p,
 * the complete frame fits (p + frame_nbytes <= nbytes), and
 *  - if the header_nbytes bytes one frame later lie inside the buffer: a header
 *    stands there, or -- that one being damaged in place -- the bytes two frames
 *    later lie inside the buffer too and a header stands there (the reference's
 *    recovery searches with check=1 and accepts a header two frames on when the
 *    next one is bad: vdif/base.py:655-690);
 *  - else (the last frame of the buffer): p < frame_nbytes, or a header stands
 *    one frame EARLIER (check=-1).
 * In terms of locate_frames from position 0 with maximum = nbytes: its answer
 * for check=(1,), or for check=(2,), in the first case and for check=(-1,) in
 * the second (tests/golden/locate_whole_cases.json records all three).
 * Every byte inside the buffer is seen, whatever the alignment of p and
 * nbytes; nothing behind nbytes is read.  frame_nbytes < 32: nothing is found.
 * Offsets are appended UNORDERED to d_offsets (capacity `cap`); *d_count
 * (device, caller-zeroed) receives the total number found.  bb_vdif_scan_at()
 * then produces the usual records for explicit, possibly unaligned offsets.
 */
int bb_vdif_locate(const void *d_buf, size_t nbytes,
                   const bb_vdif_scan_params *params,
                   int64_t *d_offsets, size_t cap,
                   unsigned long long *d_count, void *stream);

int bb_vdif_scan_at(const void *d_buf, size_t nbytes,
                    const bb_vdif_scan_params *params,
                    const int64_t *d_offsets, size_t nframes,
                    bb_frame_rec *d_recs, void *stream);

/*
 * Mark 5B header scan (mark5b/header.py:60-68,91-97; mark5b/base.py:206-213):
 * sync word 0xABADDEED, frame_nr, BCD seconds; fixed 10016-byte frames.  The
 * invalid-frame test (payload == 0x11223344 everywhere,
 * mark5b/frame.py:62-70) is folded into the same pass.
 */
typedef struct bb_mark5b_scan_params {
    uint64_t first_offset;
    int32_t  ref_seconds;     /* header0 BCD jday*86400+seconds, decoded */
    int32_t  ref_frame_nr;
    int32_t  frame_rate;
    int32_t  by_position;     /* nonzero: headers are not looked at -- every whole frame counts and is placed
                               * by where it lies (frame k of the call = time index k): a reader with
                               * verify=False, which in the reference reads the frame at the position of an
                               * index and checks nothing (base/base.py:1003-1010) */
} bb_mark5b_scan_params;

/* Records (bb_mark5b_scan and bb_mark5b_scan_at): payload_offset = frame offset
 * + 16.  A frame that does not lie wholly inside the buffer has no header (its
 * words read as zero) and is neither OK nor INVALID.  time_index = (jday * 86400
 * + seconds - ref_seconds) * frame_rate + frame_nr - ref_frame_nr, where a
 * difference below -500 days has 1000 days added (jday is the day modulo 1000,
 * mark5b/header.py:235-262; a stream runs forward from header0); the frame's
 * number in the call when frame_rate = 0 or by_position; clamped to
 * +-(2^31 - 1).  BCD nibbles above 9 make the reference raise
 * (base/utils.py:18-40); what the scan gives for them is not defined. */
int bb_mark5b_scan(const void *d_buf, size_t nbytes,
                   const bb_mark5b_scan_params *params,
                   bb_frame_rec *d_recs, size_t nframes, void *stream);

/*
 * Corruption-tolerant Mark 5B indexing (reference:
 * VLBIStreamReaderBase._bad_frame, base/base.py:1127-1219, with
 * Mark5BFileReader.find_header, mark5b/base.py:136-155, and locate_frames,
 * base/base.py:181-335).  bb_mark5b_locate tests EVERY byte offset: a frame
 * starts at p when the sync word 0xABADDEED sits there, the 10016-byte frame
 * fits in the buffer, the BCD time code passes its CRC-16 (whatever its
 * nibbles: the search does not decode them), and -- when MORE than four bytes
 * lie behind the frame (p + 10016 + 4 < nbytes) -- another sync word sits one
 * frame later (check=1; the reference looks at a check point c only when
 * `c < stop - offset - pattern.size`, base/base.py:329-333, strictly: a file
 * with exactly four bytes of anything behind its last frame keeps that frame).
 * A sync word that lies inside the buffer is seen whole, whatever the
 * alignment of p and of nbytes; nothing behind nbytes is read.
 * Offsets are appended unordered to d_offsets (at most `cap`; *d_count, which
 * the caller zeroes, receives the number found).  bb_mark5b_scan_at is
 * bb_mark5b_scan for frames at explicit, possibly odd, offsets
 * (params->first_offset is ignored).
 */
/*
 * Reads [d_buf, d_buf + nbytes) once, with plain loads, and keeps nothing (round 6).  What a
 * launch reads that way stays in the device's 256 MiB memory-side cache for the launches right
 * behind it -- the nontemporal stores of a decode do not push it out -- so a decode whose input
 * was just read through takes it from there: the decode launch of 2^13-2^15 frames of 8 KiB runs
 * 11-16 % faster (profiles/r06cp_exp_tiles_by_size_same_window.log against r06cq_).  The three
 * *_read_window calls do this themselves for windows of 16-256 MiB, on the decode's stream,
 * next to the scan on its own: a whole read() gains 4-7 % (profiles/r06cx_, r06cy_exp_touch_read.log;
 * BB_TUNE_TOUCH_MIB, include/bbdecode_tune.h).  No reference
 * counterpart: the reference reads a file through the page cache (base/base.py:919-969).
 */
int bb_touch(const void *d_buf, size_t nbytes, void *stream);

int bb_mark5b_locate(const void *d_buf, size_t nbytes, int64_t *d_offsets,
                     size_t cap, unsigned long long *d_count, void *stream);
/* ... for ONE stream: word 1 of the header must also agree with `w1_pattern` under
 * `w1_mask` (the bits header0.invariant_pattern() marks in that word: the user
 * word, mark5b/header.py:70-73), at p and one frame later, as the stream
 * reader's searches do, which hand header0 to locate_frames
 * (base/base.py:1083-1219).  The pattern is then eight bytes long: sync word and
 * word 1 one frame later are looked at when MORE than eight bytes lie behind the
 * frame, and not at all otherwise (the reference's rule for a mask whose top byte
 * carries bits, as the user word's does).  w1_mask = 0: bb_mark5b_locate. */
int bb_mark5b_locate_stream(const void *d_buf, size_t nbytes, uint32_t w1_pattern, uint32_t w1_mask,
                            int64_t *d_offsets, size_t cap, unsigned long long *d_count, void *stream);
int bb_mark5b_scan_at(const void *d_buf, size_t nbytes,
                      const bb_mark5b_scan_params *params,
                      const int64_t *d_offsets, size_t nframes,
                      bb_frame_rec *d_recs, void *stream);

/*
 * Turn scan records into the dense, output-ordered source table the decode
 * kernels consume: d_src[time_index*nslot + slot] = payload offset, or -1 for
 * frames that are missing or flagged invalid (they decode to fill_value:
 * base/frame.py:191-199, vdif/frame.py:79-90).  d_thread_slot maps a VDIF
 * thread_id (0..1023) to its output slot or -1 (thread not selected:
 * vdif/base.py:464-490); NULL means "slot 0 for every frame".
 * Replaces VDIFFrameSet.fromfile's gather-by-thread (vdif/frame.py:176-243)
 * and RawOffsets (base/offsets.py).
 */
/*
 * Verification of scan records (verify=True / 'fix': the checks the reference
 * makes frame by frame in VLBIStreamReaderBase._read_frame, base/base.py:
 * 1083-1125 -- header valid, frame index as expected, and a readable header
 * behind the frame).  Adds to *d_nbad the number of records that are not
 * BB_FRAME_OK or, among the first `nstrict`, whose time_index differs from
 * first_index + i / recs_per_index (recs_per_index = threads per frame set).
 */
int bb_verify_records(const bb_frame_rec *d_recs, size_t nrecs,
                      int32_t first_index, uint32_t recs_per_index,
                      size_t nstrict, uint32_t *d_nbad, void *stream);

int bb_build_index(const bb_frame_rec *d_recs, size_t nrecs,
                   const int16_t *d_thread_slot, int nslot,
                   int64_t *d_src, size_t nframes_out, void *stream);

/* ---- packed-sample decode ---------------------------------------------- */

/*
 * Flat LUT decode of whole frames (V1-V3, V8, V10, M5-1, S1, D1 of
 * SURVEY.md section 8a): replaces lut.take(words.view(u1), axis=0)
 * (vdif/payload.py:69-103, mark5b/payload.py:78-94), decode_8bit
 * (base/encoding.py:131-144), int8 astype (dada/payload.py:13-14),
 * PayloadBase._decode/.view/.reshape (base/payload.py:314-330), the frameset
 * thread interleave (vdif/frame.py:402-434) and the invalid -> fill_value
 * branch (base/frame.py:191-199).
 *
 * For output frame f and slot s the payload at d_buf + d_src[f*nslot+s]
 * (payload_nbytes bytes) is expanded to E = payload_nbytes*8/bps float32
 * values v[e]; value e lands at
 *     d_out[((f*R + e/chunk)*nslot + s)*chunk + e%chunk],  R = E/chunk
 * i.e. rows of `chunk` values (chunk = nchan * (2 if complex)) interleaved
 * over nslot threads.  A source of -1 writes fill (re, im alternating when
 * `complex_data`).  With d_src == NULL frames are taken at
 * src0 + (f*nslot + s)*src_stride (fixed-stride file, all valid; the last one
 * must end inside buf_nbytes, else BB_ERANGE).
 *
 * Bounds: every decode entry point follows an index entry only when the whole
 * unit it names (payload_nbytes here; the stream words of a Mark 4 unit; the
 * kept channels' bytes of a block) lies inside [0, buf_nbytes).  Any other
 * entry -- negative, past the end, a stale or corrupt index -- decodes as
 * fill, exactly like -1; nothing outside the buffer is read.  The reference
 * never returns garbage for bytes a file does not hold either (short read ->
 * EOFError, base/payload.py:135-136).
 *
 * An empty request (nframes == 0) launches nothing and touches no buffer.  Its
 * answer depends on the output type: for float32 it is BB_OK as soon as
 * (coder, bps) is supported -- the rest of the parameter block is not looked at;
 * for BB_OUT_F16 / BB_OUT_BF16 it is BB_OK only when the whole parameter block
 * passes (what bb_decode_out_check answers), else that check's code.
 */
typedef struct bb_decode_params {
    int32_t  coder;            /* enum bb_coder */
    int32_t  bps;              /* 1, 2, 4, 8 */
    int32_t  chunk;            /* float32 values per (sample, slot) */
    int32_t  nslot;            /* threads interleaved in one output row */
    uint64_t payload_nbytes;   /* per frame and slot */
    int64_t  src0;             /* used when d_src == NULL */
    int64_t  src_stride;       /* used when d_src == NULL */
    int32_t  complex_data;     /* selects (fill_re, fill_im) vs fill_re only */
    float    fill_re;
    float    fill_im;
    int32_t  out_type;         /* enum bb_out_type; 0 = float32.  With BB_OUT_F16 / BB_OUT_BF16
                                * d_out is REINTERPRETED: it points to out_elems 16-bit elements
                                * (out_elems keeps counting elements; 16-byte alignment as for
                                * float32), the fill value is rounded like the levels.  Honoured by
                                * bb_decode_frames, bb_vdif_read_window and bb_mark5b_read_window;
                                * bb_decode_frames_select (and a window call with nwithin > 0)
                                * answers BB_ENOTSUP, nothing is launched.  Anything else: BB_EINVAL. */
} bb_decode_params;

int bb_decode_frames(const void *d_buf, size_t buf_nbytes,
                     const int64_t *d_src, size_t nframes,
                     const bb_decode_params *params,
                     float *d_out, size_t out_elems, void *stream);

/*
 * What a bb_decode_frames launch with these parameters would answer, as far as
 * the parameters decide it (no buffers, no device): BB_OK, BB_EINVAL (unknown
 * out_type, sizes), BB_ENOTSUP (coder / bps, a chunk that is not a power of two
 * with nslot > 1, or a combination the 16-bit kernels do not take: more than
 * 2048 thread slots).  Readers plan with it: where it does not say BB_OK for a
 * 16-bit type they decode float32 and convert, which gives the same values
 * (PayloadBase._decode followed by astype: base/payload.py:314-330).
 */
int bb_decode_out_check(const bb_decode_params *params);

/*
 * bb_decode_frames with a CHANNEL SELECTION folded in: of every thread
 * sample's `chunk` floats only positions d_within[0 .. nwithin) (device array,
 * each 0 <= w < chunk, any order, repeats allowed) are written, in that order:
 *   out[((f * R + r) * nslot + s) * nwithin + k] = sample (f, r, s)[d_within[k]].
 * Replaces what the reference does for a reader `subset` that picks channels
 * (decode the whole frame, then index: base/base.py:706-717 with 957-969;
 * vdif/base.py:519-528) without writing -- and re-reading -- the channels
 * nobody asked for.  `d_src` is required (one offset per frame-slot, -1 =
 * fill); `chunk` must be a power of two.  d_out needs 4-byte alignment only.
 * BB_ENOTSUP when the thread slots do not fit the on-chip staging buffer.
 */
int bb_decode_frames_select(const void *d_buf, size_t buf_nbytes,
                            const int64_t *d_src, size_t nframes,
                            const bb_decode_params *params,
                            const int32_t *d_within, int nwithin,
                            float *d_out, size_t out_elems, void *stream);

/*
 * The argument and geometry checks of bb_decode_frames_select without a launch
 * (no device needed): BB_OK when a launch with these parameters and `nwithin`
 * kept positions would be accepted, else the code it would return (BB_EINVAL:
 * more than 4096 positions, sizes that do not fit; BB_ENOTSUP: a thread sample
 * wider than a work item can hold whole rows of -- 16 tiles of 256 bytes -- or
 * more thread slots than the on-chip staging buffer takes).  Readers ask this
 * when they plan a subset (baseband_amd/base/base.py _plan_channel_select) and
 * keep the reference's decode-then-index order otherwise (base/base.py:706-717).
 * Only coder, bps, chunk, nslot and payload_nbytes of `params` are looked at.
 */
int bb_decode_frames_select_check(const bb_decode_params *params, int nwithin);

/*
 * One window of a VDIF stream read in ONE call: bb_vdif_scan over `nframes`
 * frames at scan->first_offset, bb_build_index for `nsets` frame sets,
 * bb_verify_records (when d_nbad is given; `nstrict` records checked for their
 * time index, `recs_per_index` = threads per set in the file), then
 * bb_decode_frames -- or bb_decode_frames_select when nwithin > 0 -- through
 * that index.  The body of the reference's read loop for the frames of a
 * request (base/base.py:957-967 with 1083-1125; vdif/base.py:386-390,464-490;
 * vdif/frame.py:176-243,402-434).  Same results and error codes as the four
 * calls; what it saves is host time (three library entries and their argument
 * marshalling per read() of a binding: 25 us of 65 through ctypes).
 * `verified`: optional hipEvent_t, recorded behind the verification launch and
 * AHEAD of the decode, so that a host that only needs the verdict does not wait
 * for the decode.  `scan_stream` (round 5; NULL = `stream`): the scan, index
 * and verification launches go on THIS stream, `verified` (then required) is
 * recorded there and `stream` -- which takes the decode -- is made to wait for
 * it.  A reader that decodes request after request from bytes that are in HBM
 * already gets the verdict of request k + 1 while the decode of request k is
 * still running on `stream` (back-to-back reads of 2^15 frames: the host waits
 * 0.1 instead of 0.7 ms per read).  The CALLER orders the rest: the input must
 * be complete as far as `scan_stream` can tell, and d_recs / d_src must not be
 * in use by a decode still running on `stream` (a few sets of scratch, taking
 * turns, and a wait for the decode that read a set last:
 * baseband_amd/kernels.py).  d_recs (nframes records) and d_src
 * (nsets * dec->nslot entries) are scratch the caller provides.
 */
int bb_vdif_read_window(const void *d_buf, size_t nbytes,
                        const bb_vdif_scan_params *scan, size_t nframes,
                        const int16_t *d_thread_slot, size_t nsets,
                        const bb_decode_params *dec,
                        const int32_t *d_within, int nwithin,
                        bb_frame_rec *d_recs, int64_t *d_src,
                        float *d_out, size_t out_elems,
                        uint32_t recs_per_index, size_t nstrict, uint32_t *d_nbad,
                        void *verified, void *scan_stream, void *stream);

/*
 * The same for Mark 5B and Mark 4 (single-thread formats: one record per
 * frame, slot 0): `nframes` headers are scanned -- the readers look one header
 * beyond the request when it was staged (mark5b/base.py:136-155,
 * base/base.py:1083-1125) -- and the first `n` frames are decoded; `nstrict` of
 * the records must carry the expected time index.  Mark 4: `nout` > 0 decodes
 * through shorter bit maps (bb_decode_mark4_select), 0 through the full ones.
 */
int bb_mark5b_read_window(const void *d_buf, size_t nbytes,
                          const bb_mark5b_scan_params *scan, size_t nframes, size_t n,
                          const bb_decode_params *dec,
                          const int32_t *d_within, int nwithin,
                          bb_frame_rec *d_recs, int64_t *d_src,
                          float *d_out, size_t out_elems,
                          size_t nstrict, uint32_t *d_nbad, void *verified, void *scan_stream, void *stream);

/*
 * Fetch a device counter (the d_nbad of bb_verify_records) on `side_stream`
 * once `after` (a hipEvent_t, may be NULL) has happened: the stream waits for
 * the event, copies the counter to *h_value (pinned host memory) and the call
 * returns when that copy is done -- without waiting for work queued on other
 * streams behind the event (the decode of the window that was verified).
 */
int bb_fetch_counter(const uint32_t *d_counter, uint32_t *h_value, void *after, void *side_stream);

/* ---- Mark 4 ------------------------------------------------------------ */

/*
 * Mark 4 header scan (M4-2 of SURVEY.md section 8a): for every
 * ntrack*2500-byte frame at first_offset + k*frame_nbytes, test the sync
 * pattern (stream word 63 all zero, words 64-95 all ones:
 * mark4/header.py:345-373, mark4/base.py:110-166), read the four error flags
 * of all tracks (any set -> BB_FRAME_INVALID: mark4/frame.py:78-87) and the
 * BCD time code of track 0 (mark4/header.py:134-141,198-241) to form the
 * frame index.  Times are handled in quarter-milliseconds since the start of
 * `ref_year`; `frame_qms` is the frame duration (5 .. 640).
 * bb_frame_rec.payload_offset is the FRAME start (bb_decode_mark4 skips the
 * 160 header words itself).
 */
typedef struct bb_mark4_scan_params {
    uint64_t first_offset;
    int32_t  ntrack;          /* 16, 32 or 64 */
    int32_t  ref_year;        /* full year of header0 */
    int64_t  ref_qms;         /* header0 time, quarter-ms since start of ref_year */
    int32_t  frame_qms;       /* frame duration in quarter-ms; 0: index = position */
    int32_t  by_position;     /* nonzero: as for bb_mark5b_scan_params (verify=False) */
} bb_mark4_scan_params;

/* Records (bb_mark4_scan and bb_mark4_scan_at).  A frame that does not lie
 * wholly inside the buffer has an all-zero header and is not OK.  Track 0's
 * time q: a unit-year digit equal to (ref_year + 1) % 10 adds the length of
 * ref_year (366 days in a leap year), any digit other than that and ref_year's
 * own is not OK.  time_index = (q - ref_qms) / frame_qms rounded half away from
 * zero and clamped to +-(2^31 - 1); not OK unless the division is exact.  A BCD
 * nibble above 9 in the time code counts at face value (nibble times its power
 * of ten) and makes the record not OK (the reference raises).  frame_qms = 0:
 * time_index = the frame's number in the call.  by_position: OK = the frame is
 * whole, nothing else is looked at. */
int bb_mark4_scan(const void *d_buf, size_t nbytes,
                  const bb_mark4_scan_params *params,
                  bb_frame_rec *d_recs, size_t nframes, void *stream);

/*
 * Mark 4 longitudinal (along-track) header check -- BASELINE.json configs[3]
 * "longitudinal-parity branch", SURVEY 8a row M4-x.  The 160 header bits of
 * every track end in a CRC-12 (polynomial 0x180f; mark4/header.py:34-44,
 * CRCStack in base/utils.py:200-248).  For frame k at d_offsets[k] (or, with
 * d_offsets NULL, at first_offset + k * ntrack*2500; offsets need not be word
 * aligned) d_bad_tracks[k] receives a mask with bit t set when track t's header
 * does not divide by the polynomial -- what the reference's
 * `crc12._crc(stream)` leaves non-zero (its test asserts `crc12.check(stream)`,
 * mark4/tests/test_mark4.py:57-58).  The reference never applies this check
 * while reading; neither do the decode entry points: it is an extra report that
 * does not alter decoded samples.  Pinned by tests/golden/mark4_crc_cases.json.
 */
int bb_mark4_header_crc(const void *d_buf, size_t nbytes, int ntrack,
                        const int64_t *d_offsets, int64_t first_offset, size_t nframes,
                        uint64_t *d_bad_tracks, void *stream);

/*
 * Corruption-tolerant Mark 4 indexing (reference: _bad_frame,
 * base/base.py:1127-1219, with Mark4FileReader.locate_frames,
 * mark4/base.py:110-166).  bb_mark4_locate tests EVERY byte offset: a frame
 * starts at p when stream word 63 is zero and words 64..95 are all ones, the
 * ntrack*2500-byte frame fits in the buffer, and -- when MORE than the first 96
 * stream words of the frame one later lie inside the buffer (strictly, as in
 * locate_frames, base/base.py:329-333) -- that frame shows the same pattern
 * (check=1).  Output as
 * for bb_mark5b_locate.  bb_mark4_scan_at is bb_mark4_scan for frames at
 * explicit offsets (need not be word aligned; params->first_offset ignored).
 */
int bb_mark4_locate(const void *d_buf, size_t nbytes, int ntrack,
                    int64_t *d_offsets, size_t cap,
                    unsigned long long *d_count, void *stream);
int bb_mark4_scan_at(const void *d_buf, size_t nbytes,
                     const bb_mark4_scan_params *params,
                     const int64_t *d_offsets, size_t nframes,
                     bb_frame_rec *d_recs, void *stream);

/*
 * Mark 4 track-demultiplexing decode (M4-1, M4-2): replaces the five
 * decoders decode_{2chan_2bit_fanout4, 4chan_2bit_fanout4, 8chan_2bit_fanout2,
 * 8chan_2bit_fanout4, 16chan_2bit_fanout2_ft} (mark4/payload.py:122-288) and
 * the header-overwrite fill of Mark4Frame (mark4/frame.py:185-189,248-258).
 * Every stream word of `ntrack` bits yields ntrack/2 float32 values: output j
 * (= fanout sample t * nchan + channel c) takes its sign from bit sign_bit[j]
 * and its magnitude from bit mag_bit[j] of the word; value = {-Hi,-1,+1,+Hi}
 * [2*sign + magnitude].  The maps are data (tests/golden/mark4_bitmaps.json
 * holds the ones of the reference's five decoders).  Unit f is read at
 * d_src[f] (or src0 + f*src_stride); its first `fill_words` words and whole
 * units with source -1 are written as `fill`.
 */
typedef struct bb_mark4_decode_params {
    int32_t  ntrack;          /* 16, 32 or 64 */
    int32_t  out_type;        /* enum bb_out_type; only BB_OUT_F32 (0): BB_ENOTSUP for the 16-bit types */
    uint64_t nwords;          /* stream words per unit: 20000 (frame) or payload size */
    uint64_t fill_words;      /* 160 for frames, 0 for bare payloads */
    int64_t  src0;
    int64_t  src_stride;
    uint8_t  sign_bit[32];
    uint8_t  mag_bit[32];
    float    fill;
    int32_t  reserved2;
} bb_mark4_decode_params;

int bb_decode_mark4(const void *d_buf, size_t buf_nbytes,
                    const int64_t *d_src, size_t nframes,
                    const bb_mark4_decode_params *params,
                    float *d_out, size_t out_elems, void *stream);

/*
 * bb_decode_mark4 with a CHANNEL SELECTION folded in.  Output j of a stream
 * word is sample j / nchan, channel j % nchan of that word (ntrack/2 =
 * fanout * nchan outputs); a reader `subset` that keeps channels c_0 .. c_{m-1}
 * (base/base.py:706-717 applied after mark4/payload.py:333-342 in the
 * reference) is the same decode with the SHORTER maps
 *     sign_bit'[fo * m + k] = sign_bit[fo * nchan + c_k]   (mag_bit alike)
 * of nout = fanout * m entries: every word then yields `nout` floats and a
 * unit nwords * nout, written contiguously -- the channels nobody asked for
 * are neither written nor re-read.  Only the first `nout` (1 .. 32) entries of
 * params->sign_bit / mag_bit are used.  d_out needs 4-byte alignment (16 for
 * the float4 store path, taken when nwords * nout is a multiple of 4).
 */
int bb_decode_mark4_select(const void *d_buf, size_t buf_nbytes,
                           const int64_t *d_src, size_t nframes,
                           const bb_mark4_decode_params *params, int nout,
                           float *d_out, size_t out_elems, void *stream);

/* One window of a Mark 4 stream read in one call (see bb_mark5b_read_window). */
int bb_mark4_read_window(const void *d_buf, size_t nbytes,
                         const bb_mark4_scan_params *scan, size_t nframes, size_t n,
                         const bb_mark4_decode_params *dec, int nout,
                         bb_frame_rec *d_recs, int64_t *d_src,
                         float *d_out, size_t out_elems,
                         size_t nstrict, uint32_t *d_nbad, void *verified, void *scan_stream, void *stream);

/* ---- float32 samples (extension) ---------------------------------------- */

/*
 * `nframes` runs of `nbytes_per_frame` bytes at src0 + f * src_stride of d_buf
 * -> d_out, contiguous: what "decoding" float32 samples amounts to.  EXTENSION
 * -- the reference has no such decoder: DADAPayload._decoders = {8: ...}
 * (dada/payload.py:40-41), NBIT 32 raises KeyError(32) there; BASELINE.json
 * configs[4] names "DADA float32 passthrough".  Nothing to be bit-exact
 * against except the file's own bytes: parity is unpinned by construction and
 * the test is byte identity.  Sizes, offsets and pointers are multiples of 4
 * (BB_EINVAL otherwise); 16-byte loads and stores when they are multiples of
 * 16 (DADA: 4096-byte headers).  BB_ERANGE when a run ends outside
 * buf_nbytes or the output is too small.  Stream-ordered, no host sync.
 */
int bb_copy_frames(const void *d_buf, size_t buf_nbytes, size_t nframes,
                   uint64_t nbytes_per_frame, int64_t src0, int64_t src_stride,
                   void *d_out, size_t out_nbytes, void *stream);

/* ---- sampler statistics (extension) -------------------------------------- */

/*
 * How often every raw code occurs, per thread slot and position in a row,
 * counted from the packed bytes without decoding them.  EXTENSION -- the
 * reference has no counterpart (its users decode and compare, or run m5bstate /
 * vdifbstate on the file).  A "code" is a field of the payload taken LSB first,
 * the order of vdif/payload.py:25-103 and mark5b/payload.py:27-94: code e of
 * the payload of frame f, slot s is field e % (8/bps) of byte e / (8/bps); with
 * raw value c it ADDS one to
 *     d_counts[((s * chunk + e % chunk) << bps) + c]
 * when its global row f * R + e / chunk lies in [row_lo, row_hi) and the
 * frame-slot's source passes the bounds rule of bb_decode_frames: a source of
 * -1, any negative one, or one whose payload does not lie wholly inside the
 * buffer counts nothing, and nothing outside the buffer is read.  Counts are of
 * raw codes, whatever the coder: the level of code c is
 * bb_get_levels(coder, bps)[c].  The call adds to d_counts (the caller zeroes
 * it: windows and files accumulate); integer adds commute, so the result is the
 * same bit for bit from run to run.
 *
 * Pointers and payloads as for bb_decode_frames: payloads at any byte address
 * through an index, a fixed-stride request (d_src == NULL) with src0 and
 * src_stride multiples of 4 and its last payload inside the buffer (else
 * BB_ERANGE); d_counts 8-byte aligned; ncounts >= (nslot * chunk) << bps and
 * row_hi <= nframes * R, else BB_ERANGE.  Stream-ordered, never allocates,
 * never synchronises; nframes == 0 or row_lo == row_hi launches nothing.
 *
 * bb_count_states_check answers what the parameters alone decide (no buffers,
 * no device): BB_EINVAL (a NULL block, sizes, reserved != 0, a payload that is
 * not a multiple of 4 or not whole rows, row_lo > row_hi), BB_ENOTSUP (bps not
 * in {1, 2, 4, 8}, a chunk that is not a power of two, or chunk * bps > 128:
 * the kernel keeps the at most 16 byte phases of a row on chip).
 */
typedef struct bb_states_params {
    int32_t  bps;             /* 1, 2, 4, 8 */
    int32_t  chunk;           /* codes per (sample, slot): nchan * (2 if complex); a power of two */
    int32_t  nslot;           /* thread slots, as in bb_decode_params */
    int32_t  reserved;        /* 0 */
    uint64_t payload_nbytes;  /* per frame and slot; a multiple of 4; whole rows */
    int64_t  src0, src_stride;/* used when d_src == NULL, as in bb_decode_frames */
    uint64_t row_lo, row_hi;  /* rows (complete samples) [row_lo, row_hi) of the request's
                                 nframes * R rows are counted, R = payload_nbytes*8/bps/chunk */
} bb_states_params;

int bb_count_states(const void *d_buf, size_t buf_nbytes,
                    const int64_t *d_src, size_t nframes,
                    const bb_states_params *params,
                    unsigned long long *d_counts, size_t ncounts, void *stream);
int bb_count_states_check(const bb_states_params *params);

/*
 * The same counts as a time series: per thread slot, TIME BIN and position in a
 * row.  Buffer, index, fixed stride, row_lo / row_hi and code order are those of
 * bb_count_states.  Counted row r of the request has the series index
 * g = first_row + (r - row_lo) and lands in bin g / bin_rows: a reader hands a
 * file in window by window, and a bin that straddles two windows is completed
 * by two calls.  Code c at position pos of a row of slot s in bin b ADDS one to
 *     d_counts[(((s * nbins + b) * chunk + pos) << bps) + c]
 * (uint32 counters, slot-major: the bins a wave finishes one after the other
 * are contiguous memory; the caller zeroes them; bit-reproducible).  A counter
 * of one call never exceeds bin_rows.
 *
 * bb_count_states_bins_check answers what the parameters alone decide:
 * everything bb_count_states_check refuses, BB_EINVAL for bin_rows == 0 or
 * bin_rows > 2^31 - 1, BB_ENOTSUP when bin_rows * chunk * bps is not a multiple
 * of 8 (bins are whole bytes) or chunk << bps > 1024 (8-bit samples with chunk
 * 8 and 16: two bins' counters must fit a wave's 8 KiB window on chip).
 *
 * The call itself answers in addition BB_ENOTSUP when first_row, row_lo or
 * row_hi times chunk * bps is not a multiple of 8 (whole bytes only: there is
 * no field-by-field edge), BB_ERANGE when ncounts < nslot * nbins * (chunk <<
 * bps), when row_hi > nframes * R or when the last counted row's bin is >=
 * nbins, BB_EINVAL when d_counts is NULL or not 4-byte aligned.  Stream-ordered,
 * never allocates, never synchronises; nframes == 0 or row_lo == row_hi
 * launches nothing; an argument error leaves d_counts untouched.
 */
int bb_count_states_bins(const void *d_buf, size_t buf_nbytes,
                         const int64_t *d_src, size_t nframes,
                         const bb_states_params *params,
                         uint64_t bin_rows, uint64_t first_row, uint64_t nbins,
                         uint32_t *d_counts, size_t ncounts, void *stream);
int bb_count_states_bins_check(const bb_states_params *params, uint64_t bin_rows);

/* ---- power and moments from int8 block streams (EXTENSION) ---------------- */

/*
 * The sums of x and of x * x of every real component of every sample, per time
 * bin, from the stored int8 bytes of GUPPI raw blocks and plain DADA frames:
 * one read of the payloads, nothing is decoded.  The reference has no
 * counterpart (there: a read, then a reduction over the float32 samples).
 *
 * Time t in [t_lo, t_hi) of frame f of the call is row
 *     first_row + f * (t_hi - t_lo) + (t - t_lo)
 * of a series and lands in bin row / bin_rows.  Component k (0: real, 1:
 * imaginary; ncomp = 1: real data) of polarisation p and channel c of that
 * time ADDS x to
 *     d_sums[(((bin * npol + p) * nchan + c) * ncomp + k) * 2]
 * and x * x to the element behind it (int64; the reader's sample order).  The
 * caller zeroes d_sums: windows of a file and pieces with different row ranges
 * fill one answer by several calls with continuing first_row.  Integer adds
 * commute: the result is the same bit for bit from run to run.
 *
 * Layouts (an enum of their own; enum bb_layout is not touched):
 *   BB_MOMENTS_GUPPI_CF  (chan, time, pol, re/im), npol 1 or 2, ncomp 2
 *   BB_MOMENTS_GUPPI_TF  (time, chan, pol, re/im), npol 2, ncomp 2
 *   BB_MOMENTS_ROWS      (time, pol, chan, comp) as plain DADA stores them, with
 *                        R = npol * nchan * ncomp in {1, 2, 4} or a multiple of 4
 *   BB_MOMENTS_MKBF      MeerKAT beamformer heaps: NOT taken (BB_ENOTSUP); decode
 *                        and reduce instead
 *
 * Frames as for bb_decode_frames: through the index d_src (offsets that are
 * multiples of 4; -1, any negative one, one whose payload of ntime times does
 * not lie wholly inside the buffer or one off a dword adds nothing) or at
 * src0 + f * src_stride.  Nothing outside times [t_lo, t_hi) of a payload is
 * read, but for the rest of a dword that holds an edge.
 *
 * bb_i8_moments_check answers what the parameters alone decide (no buffers, no
 * device), in this order: BB_EINVAL for a NULL block; BB_ENOTSUP for
 * BB_MOMENTS_MKBF, BB_EINVAL for an unknown layout; BB_EINVAL for npol, nchan
 * or ntime < 1, ncomp not 1 or 2, t_lo > t_hi, t_hi > ntime, bin_rows == 0, a
 * negative src0 or src_stride; BB_ENOTSUP for a geometry the kernel does not
 * take (npol > 2 or real data in a GUPPI layout, npol 1 time first, R not as
 * above, R > 2^22, more than 2^20 channels or polarisations, ntime > 2^40);
 * BB_ENOTSUP when src0, src_stride or the channel pitch ntime * npol * 2 of
 * BB_MOMENTS_GUPPI_CF is not a multiple of 4.
 *
 * The call answers in addition BB_EINVAL when d_sums is NULL or not 8-byte
 * aligned, BB_ERANGE when sums_elems < nbins * npol * nchan * ncomp * 2, when
 * first_row or nframes * (t_hi - t_lo) exceeds 2^56 or when the last row's bin
 * is >= nbins, BB_EINVAL for a NULL d_buf, BB_ENOTSUP for one that is not
 * 4-byte aligned, BB_ERANGE when a fixed-stride payload ends outside the
 * buffer.  Stream-ordered, never allocates, never synchronises; nframes == 0 or
 * t_lo == t_hi launches nothing; an argument error leaves d_sums untouched.
 */
enum bb_moments_layout {
    BB_MOMENTS_GUPPI_CF = 0,
    BB_MOMENTS_GUPPI_TF = 1,
    BB_MOMENTS_ROWS     = 2,
    BB_MOMENTS_MKBF     = 3
};
#define BB_MOMENTS_MAX_ROW (1u << 22)   /* npol * nchan * ncomp at most */

typedef struct bb_moments_params {
    int32_t  layout;          /* enum bb_moments_layout */
    int32_t  npol, nchan;
    int32_t  ncomp;           /* 2: complex, 1: real */
    uint64_t ntime;           /* times stored in a payload */
    uint64_t t_lo, t_hi;      /* times [t_lo, t_hi) of every payload are added */
    int64_t  src0, src_stride;/* used when d_src == NULL */
    uint64_t bin_rows;        /* rows of the series per bin */
    uint64_t first_row;       /* place of the call's first row in the series */
    uint64_t nbins;           /* bins of d_sums */
} bb_moments_params;

int bb_i8_moments(const void *d_buf, size_t buf_nbytes,
                  const int64_t *d_src, size_t nframes,
                  const bb_moments_params *params,
                  int64_t *d_sums, size_t sums_elems, void *stream);
int bb_i8_moments_check(const bb_moments_params *params);

/*
 * The cross-polarisation products of two-polarisation complex int8 streams, per
 * channel and time bin, from the same stored bytes: with X the sample of
 * polarisation 0 and Y that of polarisation 1, the times of a (bin, channel c)
 * ADD four int64 values to d_sums[(bin * nchan + c) * 4 + k]:
 *     k = 0: sum |X|^2 = xr * xr + xi * xi
 *     k = 1: sum |Y|^2 = yr * yr + yi * yi
 *     k = 2: sum Re X * conj(Y) = xr * yr + xi * yi
 *     k = 3: sum Im X * conj(Y) = xi * yr - xr * yi
 * (the coherency matrix, hence Stokes I, Q, U, V per time and frequency; the
 * sums of x * x above cannot give k = 2, 3).  Exact for every stored byte, -128
 * included.  The parameter block, the layouts, the frames, the series of rows,
 * first_row and the bins are those of bb_i8_moments, and so is the rule that
 * the caller zeroes d_sums and several calls fill one answer.
 *
 * bb_i8_coherence_check answers what bb_i8_moments_check answers, in its order
 * (BB_MOMENTS_MKBF stays BB_ENOTSUP), and then BB_ENOTSUP for npol != 2, for
 * ncomp != 2, and for BB_MOMENTS_ROWS with nchan > 1 and odd (the row's Y half
 * would begin inside a dword): decode and reduce instead.
 *
 * The call answers in addition what bb_i8_moments answers, in its order, with
 * BB_ERANGE when sums_elems < nbins * nchan * 4.  Stream-ordered, never
 * allocates, never synchronises; nframes == 0 or t_lo == t_hi launches
 * nothing; an argument error leaves d_sums untouched.
 */
int bb_i8_coherence(const void *d_buf, size_t buf_nbytes,
                    const int64_t *d_src, size_t nframes,
                    const bb_moments_params *params,
                    int64_t *d_sums, size_t sums_elems, void *stream);
int bb_i8_coherence_check(const bb_moments_params *params);

/* ---- format conversion on the packed bytes -------------------------------- */

/*
 * Decode of one format and encode of another applied back to back, without the
 * floats in between: base/payload.py:314-330 (fromdata / data) with
 * vdif/payload.py:25-114 and mark5b/payload.py:27-106.  Samples of the same
 * size have the same scale in these formats (docs/tutorials/
 * using_baseband.rst:589-591), so decode-then-encode is an exact map from code
 * to code:
 *     same coder (VDIF, Mark 5B, INT), every bps it has     identity
 *     VDIF <-> Mark 5B, 1 bit                               0 <-> 1
 *     VDIF <-> Mark 5B, 2 bits                              {0, 2, 1, 3}
 * Every other pair (VDIF <-> INT needs rescaling) is BB_ENOTSUP.
 *
 * Input as for bb_decode_frames and bb_count_states: frame-slot (f, s) of the
 * request has its payload_in bytes at d_src[f * nslot_in + s] (-1, any negative
 * offset or a payload not wholly inside the buffer: a source that counts
 * nothing) or, with d_src == NULL, at src0 + (f * nslot_in + s) * src_stride
 * (multiples of 4; the last payload inside the buffer, else BB_ERANGE).  Fields
 * are taken LSB first.  With R_in = payload_in * 8 / bps / chunk_in rows per
 * frame, component k = s * chunk_in + p of input row r has the code c in field
 * (r % R_in) * chunk_in + p of payload (r / R_in, s).  The output is a
 * contiguous buffer of payloads only, payload (F, t) at (F * nslot_out + t) *
 * payload_out, the payload order of the VDIF writer (vdif/base.py:792-794;
 * Mark 5B's for nslot_out == 1).  Counted row r in [row_lo, row_hi) has the
 * output row G = first_row + (r - row_lo), and with t = k / chunk_out,
 * q = k % chunk_out
 *     field (G % R_out) * chunk_out + q of output payload (G / R_out, t) = map[c]
 * or fill_code (not mapped) where the source counts nothing.  Nothing outside
 * the buffer is read; output bytes outside the rows written are not touched, so
 * one request may be split over several calls into one output buffer.
 *
 * row_lo, row_hi and first_row must fall on a byte boundary of every input and
 * every output slot stream (times chunk_in * bps and times chunk_out * bps a
 * multiple of 8), else BB_ENOTSUP: whole bytes only, there is no field-by-field
 * edge.  BB_ERANGE: row_hi > nframes * R_in, the last output row beyond
 * out_nbytes, the last fixed-stride payload outside the buffer.  BB_EINVAL:
 * NULL pointers, d_buf not 4-byte or d_out not 16-byte aligned, and what
 * bb_repack_check answers with it.  Stream-ordered, never allocates, never
 * synchronises; nframes == 0 or row_lo == row_hi launches nothing; an argument
 * error leaves d_out untouched.
 *
 * bb_repack_check answers what the parameters alone decide (no buffers, no
 * device): BB_EINVAL (a NULL block, reserved != 0, counts below 1, payloads
 * that are 0, not multiples of 4 or not whole rows, row_lo > row_hi, nslot_in *
 * chunk_in != nslot_out * chunk_out, fill_code outside [0, 1 << bps)),
 * BB_ENOTSUP (bps not in {1, 2, 4, 8}, a coder pair outside the table above,
 * chunks or slot counts that are not powers of two, more than 32 slots on a
 * side, a row of more than 256 bits).  Every power-of-two geometry with rows of
 * at most 256 bits and at most 32 slots on either side is BB_OK.
 */
typedef struct bb_repack_params {
    int32_t  bps;               /* 1, 2, 4, 8: the same on both sides */
    int32_t  coder_in, coder_out;
    int32_t  chunk_in;          /* codes per (sample, slot) of the input; a power of two */
    int32_t  nslot_in;          /* thread slots of the input; a power of two */
    int32_t  chunk_out, nslot_out;
    int32_t  fill_code;         /* code of the OUTPUT coder written where a source counts nothing */
    uint64_t payload_in;        /* bytes per frame and slot; multiples of 4; whole rows */
    uint64_t payload_out;
    int64_t  src0, src_stride;  /* used when d_src == NULL, as in bb_decode_frames */
    uint64_t row_lo, row_hi;    /* rows [row_lo, row_hi) of the request's nframes * R_in */
    uint64_t first_row;         /* output row of row_lo */
    uint64_t reserved;          /* 0 */
} bb_repack_params;

int bb_repack_frames(const void *d_buf, size_t buf_nbytes,
                     const int64_t *d_src, size_t nframes,
                     const bb_repack_params *params,
                     void *d_out, size_t out_nbytes, void *stream);
int bb_repack_check(const bb_repack_params *params);

/*
 * Conversion between sample widths on the packed bytes.  Decode, one float32
 * gain and encode applied back to back (base/payload.py:314-330 with
 * vdif/payload.py:25-114 and mark5b/payload.py:27-106; the loop of
 * docs/tutorials/using_baseband.rst:536-593) are an exact function from input
 * code to output code whatever the two widths are: a table of 1 << bps_in
 * entries.  The caller supplies it (no coder appears here), so every pair of
 * coders and every gain is the same call.
 *
 * Input exactly as for bb_repack_frames and bb_count_states: frame-slot (f, s)
 * has its payload_in bytes at d_src[f * nslot + s] (-1, any negative offset or
 * a payload not wholly inside the buffer: a source that counts nothing) or,
 * with d_src == NULL, at src0 + (f * nslot + s) * src_stride (multiples of 4;
 * the last payload inside the buffer, else BB_ERANGE).  Fields are taken LSB
 * first; payloads may lie at any byte address; nothing outside the buffer is
 * read.  nslot and chunk are the same on both sides, so a slot is one stream of
 * codes: with R_in = payload_in * 8 / bps_in / chunk and R_out = payload_out *
 * 8 / bps_out / chunk rows per frame, code p of counted row r in [row_lo,
 * row_hi) of slot s has the output row G = first_row + (r - row_lo) and
 *     field (G % R_out) * chunk + p of output payload (G / R_out, s) = map[c]
 * or fill_code (not mapped) where the source counts nothing; payload (F, s)
 * lies at (F * nslot + s) * payload_out.  Output bytes outside the rows written
 * are not touched, so one request may be split over several calls into one
 * output buffer.
 *
 * row_lo, row_hi and first_row must fall on a byte boundary of a slot stream on
 * BOTH sides (times chunk * bps_in and times chunk * bps_out a multiple of 8),
 * else BB_ENOTSUP: whole bytes only, there is no field-by-field edge.
 * BB_ERANGE: row_hi > nframes * R_in, the last output row beyond out_nbytes,
 * the last fixed-stride payload outside the buffer.  BB_EINVAL: NULL pointers,
 * d_buf not 4-byte or d_out not 16-byte aligned, and what bb_requant_check
 * answers with it.  Stream-ordered, never allocates, never synchronises;
 * nframes == 0 or row_lo == row_hi launches nothing; an argument error leaves
 * d_out untouched.
 *
 * bb_requant_check answers what the parameters alone decide (no buffers, no
 * device): BB_EINVAL (a NULL block, reserved != 0, counts below 1, payloads
 * that are 0, not multiples of 4 or not whole rows, row_lo > row_hi, fill_code
 * or a used table entry outside [0, 1 << bps_out)), BB_ENOTSUP (a width not in
 * {1, 2, 4, 8}, a chunk or slot count that is not a power of two, more than 32
 * slots, chunk * max(bps_in, bps_out) > 256).  All 16 pairs of widths are BB_OK.
 */
typedef struct bb_requant_params {
    int32_t  bps_in, bps_out;   /* 1, 2, 4, 8 each */
    int32_t  chunk;             /* codes per (sample, slot), both sides; a power of two */
    int32_t  nslot;             /* thread slots, both sides; a power of two */
    int32_t  fill_code;         /* output code written where a source counts nothing */
    int32_t  reserved;          /* 0 */
    uint64_t payload_in;        /* bytes per frame and slot; multiples of 4; whole rows */
    uint64_t payload_out;
    int64_t  src0, src_stride;  /* used when d_src == NULL, as in bb_decode_frames */
    uint64_t row_lo, row_hi;    /* rows [row_lo, row_hi) of the request's nframes * R_in */
    uint64_t first_row;         /* output row of row_lo */
    uint8_t  map[256];          /* output code by input code; entries >= 1 << bps_in are ignored */
} bb_requant_params;

int bb_requant_frames(const void *d_buf, size_t buf_nbytes,
                      const int64_t *d_src, size_t nframes,
                      const bb_requant_params *params,
                      void *d_out, size_t out_nbytes, void *stream);
int bb_requant_check(const bb_requant_params *params);

/*
 * Conversion between sample widths ACROSS thread layouts on the packed bytes:
 * bb_repack_frames' permutation of components with bb_requant_frames' table in
 * place of the coder pair, in one pass (8-bit VDIF of one channel per thread ->
 * 2-bit VDIF of one thread, or 2-bit Mark 5B).  Input exactly as for those two:
 * frame-slot (f, s) has its payload_in bytes at d_src[f * nslot_in + s] (-1,
 * any negative offset or a payload not wholly inside the buffer: a source that
 * counts nothing) or, with d_src == NULL, at src0 + (f * nslot_in + s) *
 * src_stride (multiples of 4; the last payload inside the buffer, else
 * BB_ERANGE).  A row has nslot_in * chunk_in = nslot_out * chunk_out
 * components; fields are LSB first.  With R_in = payload_in * 8 / bps_in /
 * chunk_in and R_out = payload_out * 8 / bps_out / chunk_out rows per frame,
 * component k = s * chunk_in + p of input row r has the code c in field
 * (r % R_in) * chunk_in + p (of bps_in bits) of payload (r / R_in, s).  Counted
 * row r in [row_lo, row_hi) has the output row G = first_row + (r - row_lo),
 * and with t = k / chunk_out, q = k % chunk_out
 *     field (G % R_out) * chunk_out + q (of bps_out bits) of output payload
 *     (G / R_out, t) = map[c]
 * or fill_code (not mapped) where the source counts nothing; payload (F, t)
 * lies at (F * nslot_out + t) * payload_out.  Nothing outside the buffer is
 * read; output bytes outside the rows written are not touched, so one request
 * may be split over several calls into one output buffer.
 *
 * row_lo, row_hi and first_row must fall on a byte boundary of every input and
 * every output slot stream (times chunk_in * bps_in and times chunk_out *
 * bps_out a multiple of 8), else BB_ENOTSUP: whole bytes only.  BB_ERANGE:
 * row_hi > nframes * R_in, the last output row beyond out_nbytes, the last
 * fixed-stride payload outside the buffer.  BB_EINVAL: NULL pointers, d_buf not
 * 4-byte or d_out not 16-byte aligned, and what bb_recode_check answers with
 * it.  Stream-ordered, never allocates, never synchronises; nframes == 0 or
 * row_lo == row_hi launches nothing; an argument error leaves d_out untouched.
 *
 * bb_recode_check answers what the parameters alone decide (no buffers, no
 * device), in this order: a NULL block (BB_EINVAL); a width not in {1, 2, 4, 8}
 * (BB_ENOTSUP); reserved != 0 or a chunk or slot count below 1 (BB_EINVAL); a
 * chunk or slot count that is not a power of two (BB_ENOTSUP); nslot_in *
 * chunk_in != nslot_out * chunk_out (BB_EINVAL); more than 32 slots on a side
 * (BB_ENOTSUP); nslot * chunk * max(bps_in, bps_out) > 256 (BB_ENOTSUP);
 * payloads that are 0, not multiples of 4 or not whole rows (BB_EINVAL);
 * fill_code, then a used table entry, outside [0, 1 << bps_out) (BB_EINVAL);
 * row_lo > row_hi (BB_EINVAL).
 */
typedef struct bb_recode_params {
    int32_t  bps_in, bps_out;   /* 1, 2, 4, 8 each */
    int32_t  chunk_in;          /* codes per (sample, slot) of the input; a power of two */
    int32_t  nslot_in;          /* thread slots of the input; a power of two */
    int32_t  chunk_out, nslot_out;
    int32_t  fill_code;         /* output code written where a source counts nothing */
    int32_t  reserved;          /* 0 */
    uint64_t payload_in;        /* bytes per frame and slot; multiples of 4; whole rows */
    uint64_t payload_out;
    int64_t  src0, src_stride;  /* used when d_src == NULL, as in bb_decode_frames */
    uint64_t row_lo, row_hi;    /* rows [row_lo, row_hi) of the request's nframes * R_in */
    uint64_t first_row;         /* output row of row_lo */
    uint8_t  map[256];          /* output code by input code; entries >= 1 << bps_in are ignored */
} bb_recode_params;

int bb_recode_frames(const void *d_buf, size_t buf_nbytes,
                     const int64_t *d_src, size_t nframes,
                     const bb_recode_params *params,
                     void *d_out, size_t out_nbytes, void *stream);
int bb_recode_check(const bb_recode_params *params);

/*
 * bb_recode_frames with ONE TABLE PER COMPONENT of a row: a gain per (thread,
 * channel) in front of the requantizer.  Everything is as for bb_recode_frames
 * -- the same parameter block, geometry, limits and whole-byte rule; equal
 * thread structures on both sides are a legal geometry -- but the output field
 * of component k = s * chunk_in + p is
 *     d_tables[(k << bps_in) + c]
 * or fill_code (not mapped) where the source counts nothing.  d_tables is
 * DEVICE memory on a 4-byte boundary: ncomp << bps_in bytes (ncomp = nslot_in *
 * chunk_in; at most 8 KiB), one table of 1 << bps_in output codes after the
 * other.  The host cannot see the values, so the kernel keeps the low bps_out
 * bits of every table byte: a bad table never sets bits of a neighbouring
 * field.  The block's own map is checked as bb_recode_check checks it and is
 * otherwise ignored; leave it zero.
 *
 * Checks: everything bb_recode_frames checks, in its order (a request of no
 * rows is BB_OK there and then); then d_tables NULL or not 4-byte aligned
 * (BB_EINVAL); then tables_nbytes < ncomp << bps_in (BB_ERANGE).
 * Stream-ordered, never allocates, never synchronises; nframes == 0 or row_lo
 * == row_hi launches nothing; an argument error leaves d_out untouched.
 * bb_recode_tables_check answers what bb_recode_check answers.
 */
int bb_recode_frames_tables(const void *d_buf, size_t buf_nbytes,
                            const int64_t *d_src, size_t nframes,
                            const bb_recode_params *params,
                            const uint8_t *d_tables, size_t tables_nbytes,
                            void *d_out, size_t out_nbytes, void *stream);
int bb_recode_tables_check(const bb_recode_params *params);

/* ---- byte-aligned formats with an axis permutation --------------------- */

/*
 * int8 (re, im) -> complex64 decode with the axis permutation of
 *   BB_LAYOUT_GUPPI_CF  GUPPI channels-first payloads, (chan, time, pol) ->
 *                       (time, pol, chan)            (guppi/payload.py:90-96)
 *   BB_LAYOUT_MKBF      MeerKAT beamformer DADA heaps, (heap, pol, chan, 256)
 *                       -> (heap*256, pol, chan)     (dada/payload.py:54-89)
 *   BB_LAYOUT_GUPPI_TF  GUPPI time-first ('SIMPLE') payloads, (time, chan, pol)
 *                       -> (time, pol, chan)         (guppi/payload.py:97-102)
 * (G1 and D1 of SURVEY.md section 8a).  From every frame only times
 * [t_lo, t_hi) are decoded -- this is how the GUPPI OVERLAP is dropped
 * (guppi/base.py:203-225) and how partial reads avoid touching whole blocks.
 * Output: frame f, time t, pol p, chan c at
 *   d_out[(((f*(t_hi-t_lo) + t-t_lo)*npol + p)*nchan + c)*2 + {0,1}].
 * Real-valued byte data needs no permutation and goes through
 * bb_decode_frames(BB_CODER_INT, 8).
 */
enum bb_layout {
    BB_LAYOUT_GUPPI_CF = 0,
    BB_LAYOUT_MKBF     = 1,
    BB_LAYOUT_GUPPI_TF = 2
};

typedef struct bb_tiled_params {
    int32_t  layout;          /* enum bb_layout */
    int32_t  npol;
    int32_t  nchan;           /* channels decoded */
    int32_t  nchan_stored;    /* channels the payload holds, when only the `nchan` starting at the
                                 payload offset are decoded (a reader subset that keeps a channel
                                 range: point src0 / d_src at the first kept channel -- c_lo *
                                 ntime * npol * 2 bytes into a GUPPI_CF payload, c_lo * 512 into an
                                 MKBF heap, c_lo * npol * 2 into a GUPPI_TF time); 0 = nchan */
    uint64_t ntime;           /* complete samples stored per frame */
    uint64_t t_lo, t_hi;      /* local sample range to decode, t_hi <= ntime */
    int64_t  src0;            /* payload offsets when d_src == NULL */
    int64_t  src_stride;
    float    fill_re, fill_im;
    /* A reader subset that keeps a LIST of channels and / or one of two
     * polarisations, folded into the decode (the reference decodes whole blocks
     * and indexes afterwards: base/base.py:706-717 after guppi/payload.py:90-102,
     * dada/payload.py:76-79).  The payload offsets point at the payload START
     * (no channel skip), nchan_stored / npol_stored give the stored counts:
     *   out[f, t, p, c] = stored[f, t, pol_first + p, d_chan_map[c]]
     * for p < npol, c < nchan.  d_chan_map: device array of `nchan` stored-channel
     * numbers (each < nchan_stored; any order, repeats allowed), NULL = channels
     * 0 .. nchan-1.  npol_stored 0 = npol.  Only the 16-byte-aligned fast form
     * takes a selection (payload and buffer 16-byte aligned, even nchan, fixed
     * stride); anything else answers BB_ENOTSUP and the caller decodes whole
     * blocks and indexes, like the reference. */
    int32_t  npol_stored;
    int32_t  pol_first;
    const int32_t *d_chan_map;
} bb_tiled_params;

int bb_decode_i8_tiled(const void *d_buf, size_t buf_nbytes,
                       const int64_t *d_src, size_t nframes,
                       const bb_tiled_params *params,
                       float *d_out, size_t out_elems, void *stream);

/* ---- encoders (write side) ----------------------------------------------- */

/*
 * float32 samples -> packed codes, the inverse of bb_decode_frames for one
 * contiguous run.  Thresholds and rounding follow
 * the reference encoders operation by operation: encode_1bit_base /
 * encode_2bit_base (incl. NumPy's floor_divide) / encode_4bit_base /
 * encode_8bit (base/encoding.py:63-158; vdif/payload.py:77-114), Mark 5B
 * sign/magnitude ordering (mark5b/payload.py:84-106), integer formats
 * (gsb/payload.py:44-52, dada/payload.py:17-18).  Complex data are passed as
 * interleaved (re, im) float32.  nelem must be a multiple of 4 and of 8/bps.
 */
int bb_encode_flat(const float *d_in, size_t nelem, int coder, int bps,
                   void *d_out, size_t out_nbytes, void *stream);

/*
 * Mark 4 track multiplexing (mark4/payload.py:138-300): nwords stream words
 * from nwords * ntrack/2 float32 values laid out (sample, channel); the bit
 * maps are those of bb_decode_mark4.
 */
int bb_encode_mark4(const float *d_in, size_t nwords, int ntrack,
                    const uint8_t sign_bit[32], const uint8_t mag_bit[32],
                    void *d_out, size_t out_nbytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BBDECODE_H */
