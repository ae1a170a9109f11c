// The packed-byte entries of bbdecode.hip (bb_count_states, bb_count_states_bins, bb_repack_frames,
// bb_requant_frames, bb_recode_frames, bb_recode_frames_tables, bb_i8_moments, bb_i8_coherence), their argument checks and what they share.  The ORDER of the checks is part of
// the ABI: tests/golden/abi_return_codes.json holds it in place.
extern "C++" { namespace {                                   // (the entries have C linkage: the include stands among them)
// A slot's stream of rows: payloads of whole dwords that hold whole rows of `chunk` codes
// of `bps` bits (both checked by the caller) -> *R rows in a payload.
inline int slot_rows(uint64_t payload_nbytes, int bps, int chunk, uint64_t *R)
{
    if (payload_nbytes == 0 || (payload_nbytes & 3) || payload_nbytes > (1ull << 56)) return BB_EINVAL;
    const uint64_t codes = payload_nbytes * 8 / (uint64_t)bps;
    *R = codes / (uint64_t)chunk;
    return codes % (uint64_t)chunk ? BB_EINVAL : BB_OK;
}

// Rows [row_lo, row_hi) of `nframes` frame(set)s of R rows each, row_lo <= row_hi (the parameter
// checks); *nrows == 0: nothing is asked for, which is BB_OK whatever the buffers are.
inline int rows_check(size_t nframes, uint64_t R, uint64_t row_lo, uint64_t row_hi, uint64_t *nrows)
{
    if ((nframes && R > (~0ull) / (uint64_t)nframes) || row_hi > (uint64_t)nframes * R) return BB_ERANGE;
    *nrows = row_hi - row_lo;                                // (no frames: row_hi is 0)
    return BB_OK;
}

// The source: `n` payloads of `span` bytes of the buffer, through the index or at the fixed
// stride -> the source members of a kernel's arguments (every bb_*_args names them alike).
template <class Args>
inline int packed_source(Args &a, const void *d_buf, size_t buf_nbytes, const int64_t *d_src,
                         int64_t src0, int64_t src_stride, uint64_t n, uint64_t span)
{
    if (!d_buf || ((uintptr_t)d_buf & 3)) return BB_EINVAL;
    a.buf = (const uint8_t *)d_buf;
    a.src = d_src;
    a.src_lim = src_limit(buf_nbytes, span);
    a.src0 = src0; a.src_stride = src_stride;
    return d_src ? BB_OK : fixed_stride_check(src0, src_stride, 4, n, span, buf_nbytes);
}

// The output side of repack and requantize: rows [row_lo, row_hi) of the request become the
// output rows from first_row on, R_out of them in each payload of payload_out bytes, nslot_out
// payloads in a frame set; bi, bo: bits per row and slot, in and out.
struct packed_out { uint64_t nrows, g_last, f_last; };       // rows asked for (rows_check), the last output row, its frame
inline int packed_output(const void *d_out, size_t out_nbytes, size_t nframes, uint64_t payload_in, uint64_t R_in,
                         uint64_t R_out, uint64_t payload_out, uint64_t nslot_out, uint64_t bi, uint64_t bo,
                         uint64_t row_lo, uint64_t row_hi, uint64_t first_row, packed_out *o)
{
    if (!d_out || ((uintptr_t)d_out & 15)) return BB_EINVAL;
    if (first_row > (1ull << 56)) return BB_ERANGE;
    if ((((row_lo & 7) | (row_hi & 7) | (first_row & 7)) * (bi | bo)) & 7) return BB_ENOTSUP;   // whole bytes only (bi, bo are powers of two)
    if (nframes && payload_in > (1ull << 58) / (uint64_t)nframes) return BB_ERANGE;
    const int rc = rows_check(nframes, R_in, row_lo, row_hi, &o->nrows);
    if (rc || !o->nrows) return rc;
    o->g_last = first_row + (o->nrows - 1);                  // in slot nslot_out - 1
    o->f_last = o->g_last / R_out;
    if (o->f_last >= (1ull << 58) / (payload_out * nslot_out)) return BB_ERANGE;
    const uint64_t end = (o->f_last * nslot_out + nslot_out - 1) * payload_out + ((o->g_last % R_out + 1) * bo + 7) / 8;
    return end > out_nbytes ? BB_ERANGE : BB_OK;
}

// A payload as even pieces of at most `seg_max` bytes, multiples of 16 like seg_max -> their number, *seg_bytes of each.
inline uint64_t even_pieces(uint64_t payload, uint64_t seg_max, uint32_t *seg_bytes)
{
    const uint64_t nseg = (payload + seg_max - 1) / seg_max;
    *seg_bytes = (uint32_t)((((payload + nseg - 1) / nseg) + 15) & ~15ull);
    return nseg;
}

// `fill_code` in every field of a dword; the grid of repack and requantize: a wave per work item
inline uint32_t fill_word(int fill_code, int bps) { return (uint32_t)fill_code * (0xffffffffu / ((1u << bps) - 1u)); }
#define BB_WAVE_ITEM_GRID 4096ull                    // workgroups: several rounds of what 256 CUs hold (repack: 4 each, 37 KiB of LDS)
inline dim3 wave_grid(uint64_t nwork) { return capped_grid((nwork + BB_WAVES_PER_BLOCK - 1) / BB_WAVES_PER_BLOCK, BB_WAVE_ITEM_GRID); }
// ... of k_recode_tables, whose LDS depends on the launch: the same four rounds of what 256 CUs hold, 160 KiB and at most 8 workgroups each
inline dim3 tables_grid(uint64_t nwork, size_t lds)
{
    return capped_grid((nwork + BB_WAVES_PER_BLOCK - 1) / BB_WAVES_PER_BLOCK, 4ull * 256ull * std::min<uint64_t>(8, (160ull << 10) / lds));
}

// What bb_repack_frames and both recode entries do after the parameter check: the output check, the source check and
// the overflow of the item count, in this order, and the members that the arguments of k_repack, k_recode and
// k_recode_tables name alike (the item geometry and the staging read them).  Params: bb_repack_params or bb_recode_params, which name
// what is read here alike; an item has item_bits bits on its wider side.  a.nwork == 0: nothing is asked for.
template <class Args, class Params>
inline int piece_args(Args &a, const void *d_buf, size_t buf_nbytes, const int64_t *d_src, size_t nframes,
                      const Params *p, int bps_in, int bps_out, uint64_t R_in, uint64_t R_out, void *d_out, size_t out_nbytes,
                      uint32_t item_bits)
{
    packed_out o;
    a.nwork = 0;
    const uint64_t bi = (uint64_t)p->chunk_in * (uint64_t)bps_in, bo = (uint64_t)p->chunk_out * (uint64_t)bps_out;   // bits per row and slot
    int rc = packed_output(d_out, out_nbytes, nframes, p->payload_in, R_in, R_out, p->payload_out, (uint64_t)p->nslot_out, bi, bo,
                           p->row_lo, p->row_hi, p->first_row, &o);
    if (rc || !o.nrows) return rc;
    rc = packed_source(a, d_buf, buf_nbytes, d_src, p->src0, p->src_stride,
                       (uint64_t)nframes * (uint64_t)p->nslot_in, p->payload_in);
    if (rc) return rc;
    a.out = (uint8_t *)d_out;
    a.buf_n = buf_nbytes;
    a.pay_in = p->payload_in; a.pay_out = p->payload_out;
    a.row_lo = p->row_lo; a.first_row = p->first_row; a.nrows = o.nrows;
    a.R_out = R_out;
    a.F0 = p->first_row / R_out;
    a.nslot_in = (uint32_t)p->nslot_in; a.nslot_out = (uint32_t)p->nslot_out;
    a.lbi = ceil_log2(bi); a.lbo = ceil_log2(bo);
    // at least 256 rows of 8 KiB, 128 of 4 KiB: 16 bytes or more of every slot on either side
    a.T = item_bits / ((uint32_t)p->nslot_in * (uint32_t)p->chunk_in * (uint32_t)std::max(bps_in, bps_out));
    a.sstride = ((a.T << a.lbi) >> 3) + BB_REPACK_SLACK;
    a.nseg = (R_out + a.T - 1) / a.T;
    const uint64_t nf = o.f_last - a.F0 + 1;
    if (nf > (~0ull) / a.nseg) return BB_ERANGE;
    a.nwork = nf * a.nseg;
    return BB_OK;
}
} }

// ---- sampler statistics (k_states.h).  EXTENSION: no reference counterpart. ----
static int states_params_check(const bb_states_params *p, uint64_t *R)
{
    if (!p) return BB_EINVAL;
    if (log2_bps(p->bps) < 0) return BB_ENOTSUP;
    if (p->reserved != 0 || p->nslot < 1 || p->chunk < 1) return BB_EINVAL;
    if (p->chunk & (p->chunk - 1)) return BB_ENOTSUP;
    if ((int64_t)p->chunk * p->bps > 8 * (int64_t)BB_STATES_MAX_PHASES) return BB_ENOTSUP;   // the byte phases kept on chip
    if (slot_rows(p->payload_nbytes, p->bps, p->chunk, R)) return BB_EINVAL;
    if (p->row_lo > p->row_hi) return BB_EINVAL;
    return BB_OK;
}

int bb_count_states_check(const bb_states_params *p) { uint64_t R; return states_params_check(p, &R); }

#define BB_STATES_GRID 2048ull                       // workgroups: what 256 CUs hold at once; each flushes once
#define BB_STATES_WAVE_ITEMS (1ull << 19)            // work items a wave may see: 2^31 bytes, its 32-bit counters cannot wrap

int bb_count_states(const void *d_buf, size_t buf_nbytes, const int64_t *d_src, size_t nframes,
                    const bb_states_params *p, unsigned long long *d_counts, size_t ncounts, void *stream)
{
    uint64_t R, nrows;
    int rc = states_params_check(p, &R);
    if (rc) return rc;
    if (!d_counts || ((uintptr_t)d_counts & 7)) return BB_EINVAL;
    const uint64_t nbins = ((uint64_t)p->nslot * (uint64_t)p->chunk) << p->bps;
    if (ncounts < nbins) return BB_ERANGE;
    rc = rows_check(nframes, R, p->row_lo, p->row_hi, &nrows);
    if (rc || !nrows) return rc;
    bb_states_args a;
    rc = packed_source(a, d_buf, buf_nbytes, d_src, p->src0, p->src_stride,
                       (uint64_t)nframes * (uint64_t)p->nslot, p->payload_nbytes);
    if (rc) return rc;
    a.counts = d_counts;
    a.payload = p->payload_nbytes;
    a.R = R;
    a.row_lo = p->row_lo; a.row_hi = p->row_hi;
    a.f_lo = p->row_lo / R;
    const uint64_t nfr = (p->row_hi + R - 1) / R - a.f_lo;          // frames that hold a counted row
    const uint64_t nseg = even_pieces(p->payload_nbytes, BB_STATES_SEG, &a.seg_bytes);
    if (nseg > 0xffffffffull || nfr > (~0ull) / nseg) return BB_ERANGE;
    a.nseg = (uint32_t)nseg;
    a.nwork = nfr * nseg;
    a.nslot = (uint32_t)p->nslot; a.chunk = (uint32_t)p->chunk;
    a.bps = (uint32_t)p->bps; a.lbps = (uint32_t)log2_bps(p->bps);
    const uint32_t cb = a.chunk * a.bps;
    a.lphase = cb > 8 ? ceil_log2(cb / 8) : 0;
    // workgroups per slot: one wave per work item up to what the device holds at once, and
    // enough of them that no wave walks more than BB_STATES_WAVE_ITEMS
    const int tb = g_tune_blocks.load();
    const uint64_t cap = std::max<uint64_t>(1, (tb > 0 ? (uint64_t)tb : BB_STATES_GRID) / a.nslot);
    uint64_t g = std::min<uint64_t>((a.nwork + BB_WAVES_PER_BLOCK - 1) / BB_WAVES_PER_BLOCK, cap);
    const uint64_t need = (a.nwork + BB_WAVES_PER_BLOCK * BB_STATES_WAVE_ITEMS - 1) / (BB_WAVES_PER_BLOCK * BB_STATES_WAVE_ITEMS);
    if (g < need) g = need;
    if (g * a.nslot > BB_GRID_MAX) return BB_ERANGE;
    const size_t lds = ((size_t)BB_WAVES_PER_BLOCK << (8 + a.lphase)) * 4 + (cb < 8 ? 64 : 0);
    hipLaunchKernelGGL(k_count_states, dim3((unsigned)(g * a.nslot)), dim3(BB_BLOCK), lds, (hipStream_t)stream, a);
    BB_HIP(hipGetLastError());
    return BB_OK;
}

// ---- ... per time bin (k_state_bins.h) ----
static int state_bins_params_check(const bb_states_params *p, uint64_t bin_rows, uint64_t *R)
{
    int rc = states_params_check(p, R);
    if (rc) return rc;
    if (bin_rows == 0 || bin_rows > 0x7fffffffull) return BB_EINVAL;          // a counter never exceeds bin_rows: int32 holds it
    if ((bin_rows * (uint64_t)p->chunk * (uint64_t)p->bps) & 7) return BB_ENOTSUP;   // bins are whole bytes
    if (((uint64_t)p->chunk << p->bps) > BB_BINS_MAX_PER_BIN) return BB_ENOTSUP;     // two bins fit a wave's window
    return BB_OK;
}

int bb_count_states_bins_check(const bb_states_params *p, uint64_t bin_rows) { uint64_t R; return state_bins_params_check(p, bin_rows, &R); }

#define BB_BINS_GRID 1280ull                         // workgroups: what 256 CUs hold at once with 32 KiB of LDS each

int bb_count_states_bins(const void *d_buf, size_t buf_nbytes, const int64_t *d_src, size_t nframes,
                         const bb_states_params *p, uint64_t bin_rows, uint64_t first_row, uint64_t nbins,
                         uint32_t *d_counts, size_t ncounts, void *stream)
{
    uint64_t R, nrows;
    int rc = state_bins_params_check(p, bin_rows, &R);
    if (rc) return rc;
    if (!d_counts || ((uintptr_t)d_counts & 3)) return BB_EINVAL;
    const uint64_t cb = (uint64_t)p->chunk * (uint64_t)p->bps;                // bits per row, at most 128
    if (first_row > (1ull << 56)) return BB_ERANGE;
    if (((first_row * cb) | ((p->row_lo & 7) * cb) | ((p->row_hi & 7) * cb)) & 7) return BB_ENOTSUP;   // whole bytes only
    const uint64_t nc = (uint64_t)p->chunk << p->bps;                         // counters per bin and slot
    if (nbins > (~0ull) / (nc * (uint64_t)p->nslot) || ncounts < nbins * nc * (uint64_t)p->nslot) return BB_ERANGE;
    if (nframes && p->payload_nbytes > (1ull << 62) / (uint64_t)nframes) return BB_ERANGE;
    rc = rows_check(nframes, R, p->row_lo, p->row_hi, &nrows);
    if (rc || !nrows) return rc;
    if (nrows > (~0ull) - first_row) return BB_ERANGE;
    if ((first_row + (nrows - 1)) / bin_rows >= nbins) return BB_ERANGE;   // the last counted row's bin
    bb_state_bins_args a;
    rc = packed_source(a, d_buf, buf_nbytes, d_src, p->src0, p->src_stride,
                       (uint64_t)nframes * (uint64_t)p->nslot, p->payload_nbytes);
    if (rc) return rc;
    a.counts = d_counts;
    a.payload = p->payload_nbytes;
    // rows -> bytes of a slot's stream (R * cb / 8 = payload: a frame begins on a byte)
    a.lo_byte = (p->row_lo / R) * a.payload + (p->row_lo % R) * cb / 8;
    a.hi_byte = (p->row_hi / R) * a.payload + (p->row_hi % R) * cb / 8;
    a.first_byte = first_row * cb / 8;
    a.bin_bytes = bin_rows * cb / 8;
    a.nbins = nbins;
    a.f_lo = a.lo_byte / a.payload;
    a.nfr = (a.hi_byte + a.payload - 1) / a.payload - a.f_lo;               // frames that hold a counted byte
    a.nslot = (uint32_t)p->nslot; a.chunk = (uint32_t)p->chunk; a.bps = (uint32_t)p->bps;
    a.lnc = (uint32_t)ceil_log2((uint32_t)nc);
    a.win_bins = BB_BINS_WIN >> a.lnc;
    // work items: even pieces of at most BB_STATES_SEG bytes that meet no more bins than a window holds
    uint64_t seg_max = BB_STATES_SEG;
    if (a.bin_bytes < seg_max && (a.win_bins - 1) * a.bin_bytes < seg_max) seg_max = (a.win_bins - 1) * a.bin_bytes;
    a.nseg = (a.payload + seg_max - 1) / seg_max;                             // (bins of fewer than 16 bytes: pieces of seg_max)
    a.seg_bytes = (uint32_t)seg_max;
    if (seg_max >= 16) a.nseg = even_pieces(a.payload, seg_max & ~15ull, &a.seg_bytes);
    if (a.nfr > (~0ull) / a.nseg || a.nfr * a.nseg > (~0ull) / a.nslot) return BB_ERANGE;
    a.nwork = a.nfr * a.nseg * a.nslot;
    // one contiguous run of items per wave, as many waves as the device holds at once
    const uint64_t waves = std::min<uint64_t>(a.nwork, BB_BINS_GRID * BB_WAVES_PER_BLOCK);
    a.per = (a.nwork + waves - 1) / waves;
    const uint64_t runs = (a.nwork + a.per - 1) / a.per;
    const uint64_t g = (runs + BB_WAVES_PER_BLOCK - 1) / BB_WAVES_PER_BLOCK;
    hipLaunchKernelGGL(k_count_state_bins, dim3((unsigned)g), dim3(BB_BLOCK), 0, (hipStream_t)stream, a);
    BB_HIP(hipGetLastError());
    return BB_OK;
}

// ---- format conversion on the packed bytes (k_repack.h): decode and encode of
//      base/payload.py:314-330, vdif/payload.py:25-114, mark5b/payload.py:27-106 back to back ----
// The code map of a coder pair at `bps`: 0 identity, 1 invert every bit, 2 swap the two bits of a field; -1: none.
static int repack_code_map(int coder_in, int coder_out, int bps)
{
    if (!coder_supported(coder_in, bps) || !coder_supported(coder_out, bps)) return -1;
    if (coder_in == coder_out) return 0;
    const bool vm = (coder_in == BB_CODER_VDIF && coder_out == BB_CODER_MARK5B) ||
                    (coder_in == BB_CODER_MARK5B && coder_out == BB_CODER_VDIF);
    if (vm && bps == 1) return 1;
    if (vm && bps == 2) return 2;
    return -1;                                              // VDIF <-> INT needs rescaling
}

static int repack_params_check(const bb_repack_params *p, uint64_t *R_in, uint64_t *R_out)
{
    if (!p) return BB_EINVAL;
    if (log2_bps(p->bps) < 0) return BB_ENOTSUP;
    if (p->reserved != 0 || p->chunk_in < 1 || p->nslot_in < 1 || p->chunk_out < 1 || p->nslot_out < 1) return BB_EINVAL;
    if (repack_code_map(p->coder_in, p->coder_out, p->bps) < 0) return BB_ENOTSUP;
    if ((p->chunk_in & (p->chunk_in - 1)) || (p->nslot_in & (p->nslot_in - 1)) ||
        (p->chunk_out & (p->chunk_out - 1)) || (p->nslot_out & (p->nslot_out - 1))) return BB_ENOTSUP;
    if ((int64_t)p->nslot_in * p->chunk_in != (int64_t)p->nslot_out * p->chunk_out) return BB_EINVAL;
    if ((uint32_t)p->nslot_in > BB_REPACK_MAX_SLOTS || (uint32_t)p->nslot_out > BB_REPACK_MAX_SLOTS) return BB_ENOTSUP;
    if ((int64_t)p->nslot_in * p->chunk_in * p->bps > (int64_t)BB_REPACK_MAX_ROW_BITS) return BB_ENOTSUP;
    if (slot_rows(p->payload_in, p->bps, p->chunk_in, R_in) ||
        slot_rows(p->payload_out, p->bps, p->chunk_out, R_out)) return BB_EINVAL;
    if (p->fill_code < 0 || p->fill_code >= (1 << p->bps)) return BB_EINVAL;
    if (p->row_lo > p->row_hi) return BB_EINVAL;
    return BB_OK;
}

int bb_repack_check(const bb_repack_params *p) { uint64_t R_in, R_out; return repack_params_check(p, &R_in, &R_out); }

int bb_repack_frames(const void *d_buf, size_t buf_nbytes, const int64_t *d_src, size_t nframes,
                     const bb_repack_params *p, void *d_out, size_t out_nbytes, void *stream)
{
    uint64_t R_in, R_out;
    int rc = repack_params_check(p, &R_in, &R_out);
    if (rc) return rc;
    bb_repack_args a;
    rc = piece_args(a, d_buf, buf_nbytes, d_src, nframes, p, p->bps, p->bps, R_in, R_out, d_out, out_nbytes, BB_REPACK_ITEM_BITS);
    if (rc || !a.nwork) return rc;
    a.map = (uint32_t)repack_code_map(p->coder_in, p->coder_out, p->bps);
    a.fillw = fill_word(p->fill_code, p->bps);
    // chunks of min(bi, bo) bits stay together; equal slot structures are a stream of whole dwords
    a.lg = a.lbi == a.lbo ? 5u : std::min(5u, std::min(a.lbi, a.lbo));
    const dim3 grid = wave_grid(a.nwork);
    hipLaunchKernelGGL(k_repack, grid, dim3(BB_BLOCK), 0, (hipStream_t)stream, a);
    BB_HIP(hipGetLastError());
    return BB_OK;
}

// ---- conversion between sample widths on the packed bytes (k_requant.h): decode, one gain and
//      encode of base/payload.py:314-330, vdif/payload.py:25-114, mark5b/payload.py:27-106 as a table ----
static int requant_params_check(const bb_requant_params *p, uint64_t *R_in, uint64_t *R_out)
{
    if (!p) return BB_EINVAL;
    if (log2_bps(p->bps_in) < 0 || log2_bps(p->bps_out) < 0) return BB_ENOTSUP;
    if (p->reserved != 0 || p->chunk < 1 || p->nslot < 1) return BB_EINVAL;
    if ((p->chunk & (p->chunk - 1)) || (p->nslot & (p->nslot - 1))) return BB_ENOTSUP;
    if ((uint32_t)p->nslot > BB_REQUANT_MAX_SLOTS) return BB_ENOTSUP;
    if ((int64_t)p->chunk * std::max(p->bps_in, p->bps_out) > (int64_t)BB_REQUANT_MAX_ROW_BITS) return BB_ENOTSUP;
    if (slot_rows(p->payload_in, p->bps_in, p->chunk, R_in) ||
        slot_rows(p->payload_out, p->bps_out, p->chunk, R_out)) return BB_EINVAL;
    if (p->fill_code < 0 || p->fill_code >= (1 << p->bps_out)) return BB_EINVAL;
    for (int c = 0; c < (1 << p->bps_in); ++c)
        if ((int)p->map[c] >= (1 << p->bps_out)) return BB_EINVAL;
    if (p->row_lo > p->row_hi) return BB_EINVAL;
    return BB_OK;
}

int bb_requant_check(const bb_requant_params *p) { uint64_t R_in, R_out; return requant_params_check(p, &R_in, &R_out); }

int bb_requant_frames(const void *d_buf, size_t buf_nbytes, const int64_t *d_src, size_t nframes,
                      const bb_requant_params *p, void *d_out, size_t out_nbytes, void *stream)
{
    uint64_t R_in, R_out; packed_out o;
    int rc = requant_params_check(p, &R_in, &R_out);
    if (rc) return rc;
    const uint64_t bi = (uint64_t)p->chunk * (uint64_t)p->bps_in, bo = (uint64_t)p->chunk * (uint64_t)p->bps_out;   // bits per row and slot
    rc = packed_output(d_out, out_nbytes, nframes, p->payload_in, R_in, R_out, p->payload_out, (uint64_t)p->nslot, bi, bo,
                       p->row_lo, p->row_hi, p->first_row, &o);
    if (rc || !o.nrows) return rc;
    bb_requant_args a;
    rc = packed_source(a, d_buf, buf_nbytes, d_src, p->src0, p->src_stride,
                       (uint64_t)nframes * (uint64_t)p->nslot, p->payload_in);
    if (rc) return rc;
    a.out = (uint8_t *)d_out;
    a.buf_n = buf_nbytes;
    a.pay_in = p->payload_in; a.pay_out = p->payload_out;
    // rows -> bytes of a slot's output stream and bits of its input stream (R * bo / 8 = payload_out: a frame begins on a byte)
    a.ya = (p->first_row / R_out) * a.pay_out + (p->first_row % R_out) * bo / 8;
    a.yb = a.ya + ((o.nrows / 8) * bo + (o.nrows % 8) * bo / 8);
    a.xbit_a = p->row_lo * bi;
    a.F0 = p->first_row / R_out;
    a.nslot = (uint32_t)p->nslot;
    a.lbi = (uint32_t)log2_bps(p->bps_in); a.lbo = (uint32_t)log2_bps(p->bps_out);
    a.seg = a.lbi > a.lbo ? BB_REQUANT_ITEM_BYTES >> (a.lbi - a.lbo) : BB_REQUANT_ITEM_BYTES;
    a.nseg = (a.pay_out + a.seg - 1) / a.seg;
    const uint64_t nf = o.f_last - a.F0 + 1;
    if (nf > (~0ull) / (a.nseg * a.nslot)) return BB_ERANGE;
    a.nwork = nf * a.nseg * a.nslot;
    a.fillw = fill_word(p->fill_code, p->bps_out);
    uint8_t *m = reinterpret_cast<uint8_t *>(a.map);                          // (entries the input cannot have: 0)
    for (int c = 0; c < 256; ++c) m[c] = c < (1 << p->bps_in) ? p->map[c] : 0;
    const dim3 grid = wave_grid(a.nwork);
    hipLaunchKernelGGL(k_requant, grid, dim3(BB_BLOCK), 0, (hipStream_t)stream, a);
    BB_HIP(hipGetLastError());
    return BB_OK;
}


// ---- conversion between sample widths across thread layouts on the packed bytes (k_recode.h):
//      bb_repack_frames' permutation of components with bb_requant_frames' table ----
static int recode_params_check(const bb_recode_params *p, uint64_t *R_in, uint64_t *R_out)
{
    if (!p) return BB_EINVAL;
    if (log2_bps(p->bps_in) < 0 || log2_bps(p->bps_out) < 0) return BB_ENOTSUP;
    if (p->reserved != 0 || p->chunk_in < 1 || p->nslot_in < 1 || p->chunk_out < 1 || p->nslot_out < 1) return BB_EINVAL;
    if ((p->chunk_in & (p->chunk_in - 1)) || (p->nslot_in & (p->nslot_in - 1)) ||
        (p->chunk_out & (p->chunk_out - 1)) || (p->nslot_out & (p->nslot_out - 1))) return BB_ENOTSUP;
    if ((int64_t)p->nslot_in * p->chunk_in != (int64_t)p->nslot_out * p->chunk_out) return BB_EINVAL;
    if ((uint32_t)p->nslot_in > BB_RECODE_MAX_SLOTS || (uint32_t)p->nslot_out > BB_RECODE_MAX_SLOTS) return BB_ENOTSUP;
    if ((int64_t)p->nslot_in * p->chunk_in * std::max(p->bps_in, p->bps_out) > (int64_t)BB_RECODE_MAX_ROW_BITS) return BB_ENOTSUP;
    if (slot_rows(p->payload_in, p->bps_in, p->chunk_in, R_in) ||
        slot_rows(p->payload_out, p->bps_out, p->chunk_out, R_out)) return BB_EINVAL;
    if (p->fill_code < 0 || p->fill_code >= (1 << p->bps_out)) return BB_EINVAL;
    for (int c = 0; c < (1 << p->bps_in); ++c)
        if ((int)p->map[c] >= (1 << p->bps_out)) return BB_EINVAL;
    if (p->row_lo > p->row_hi) return BB_EINVAL;
    return BB_OK;
}

int bb_recode_check(const bb_recode_params *p) { uint64_t R_in, R_out; return recode_params_check(p, &R_in, &R_out); }

// What both recode entries do after the parameter check: piece_args, and the members only the recode kernels have.
extern "C++" { namespace {
template <class Args>
inline int recode_args(Args &a, const void *d_buf, size_t buf_nbytes, const int64_t *d_src, size_t nframes,
                       const bb_recode_params *p, uint64_t R_in, uint64_t R_out, void *d_out, size_t out_nbytes,
                       uint32_t item_bits)
{
    const int rc = piece_args(a, d_buf, buf_nbytes, d_src, nframes, p, p->bps_in, p->bps_out, R_in, R_out, d_out, out_nbytes, item_bits);
    if (rc || !a.nwork) return rc;
    a.lpi = (uint32_t)log2_bps(p->bps_in); a.lpo = (uint32_t)log2_bps(p->bps_out);
    // the codes that stay adjacent on both sides, as far as a dword of either side holds them
    a.lgc = std::min(std::min(ceil_log2((uint32_t)p->chunk_in), ceil_log2((uint32_t)p->chunk_out)), std::min(5u - a.lpi, 5u - a.lpo));
    a.fill = (uint32_t)p->fill_code;
    return BB_OK;
}
} }

int bb_recode_frames(const void *d_buf, size_t buf_nbytes, const int64_t *d_src, size_t nframes,
                     const bb_recode_params *p, void *d_out, size_t out_nbytes, void *stream)
{
    uint64_t R_in, R_out;
    int rc = recode_params_check(p, &R_in, &R_out);
    if (rc) return rc;
    bb_recode_args a;
    rc = recode_args(a, d_buf, buf_nbytes, d_src, nframes, p, R_in, R_out, d_out, out_nbytes, BB_RECODE_ITEM_BITS);
    if (rc || !a.nwork) return rc;
    uint8_t *m = reinterpret_cast<uint8_t *>(a.map);                          // (entries the input cannot have: 0)
    for (int c = 0; c < 256; ++c) m[c] = c < (1 << p->bps_in) ? p->map[c] : 0;
    const dim3 grid = wave_grid(a.nwork);
    hipLaunchKernelGGL(k_recode, grid, dim3(BB_BLOCK), 0, (hipStream_t)stream, a);
    BB_HIP(hipGetLastError());
    return BB_OK;
}

// ---- ... with one table per component of a row (k_recode_tables.h): a gain per (thread, channel).  The parameter
//      block and its check are bb_recode_frames'; the block's own map is checked as there and not used. ----
int bb_recode_tables_check(const bb_recode_params *p) { uint64_t R_in, R_out; return recode_params_check(p, &R_in, &R_out); }

int bb_recode_frames_tables(const void *d_buf, size_t buf_nbytes, const int64_t *d_src, size_t nframes,
                            const bb_recode_params *p, const uint8_t *d_tables, size_t tables_nbytes,
                            void *d_out, size_t out_nbytes, void *stream)
{
    uint64_t R_in, R_out;
    int rc = recode_params_check(p, &R_in, &R_out);
    if (rc) return rc;
    bb_recode_tables_args a;
    // items of 4 KiB on the wider side where the input is it, of 8 KiB where the output is wider (DESIGN.md 3.12:
    // measured); at least 128 rows: 16 bytes or more of every slot on either side
    const uint32_t item_bits = p->bps_in >= p->bps_out ? BB_RECODE_ITEM_BITS / 2 : BB_RECODE_ITEM_BITS;
    rc = recode_args(a, d_buf, buf_nbytes, d_src, nframes, p, R_in, R_out, d_out, out_nbytes, item_bits);
    if (rc || !a.nwork) return rc;
    if (!d_tables || ((uintptr_t)d_tables & 3)) return BB_EINVAL;
    a.tab_n = ((uint32_t)p->nslot_in * (uint32_t)p->chunk_in) << p->bps_in;   // at most 8 KiB (recode_params_check)
    if (tables_nbytes < a.tab_n) return BB_ERANGE;
    a.tables = d_tables;
    a.tab_lds = (a.tab_n + 255u) & ~255u;
    a.in_lds = bb_recode_tables_lds(item_bits);
    a.ok_words = bb_recode_tables_flat(item_bits) / 4u / 32u;
    const size_t lds = a.tab_lds + (size_t)BB_WAVES_PER_BLOCK * (a.in_lds + 4u * a.ok_words);   // 22 .. 46 KiB
    const dim3 grid = tables_grid(a.nwork, lds);
    hipLaunchKernelGGL(k_recode_tables, grid, dim3(BB_BLOCK), lds, (hipStream_t)stream, a);
    BB_HIP(hipGetLastError());
    return BB_OK;
}

// ---- power and moments per component and time bin from int8 block streams (k_moments.h).
//      EXTENSION: no reference counterpart. ----
// What the parameters alone decide, and with it the access shape and the output map of the kernel's arguments.
static int moments_params_check(const bb_moments_params *p, bb_moments_args *a)
{
    if (!p) return BB_EINVAL;
    if (p->layout == BB_MOMENTS_MKBF) return BB_ENOTSUP;                      // heaps of 256 times: not taken
    if (p->layout != BB_MOMENTS_GUPPI_CF && p->layout != BB_MOMENTS_GUPPI_TF && p->layout != BB_MOMENTS_ROWS) return BB_EINVAL;
    if (p->npol < 1 || p->nchan < 1 || (p->ncomp != 1 && p->ncomp != 2) || p->ntime < 1) return BB_EINVAL;
    if (p->t_lo > p->t_hi || p->t_hi > p->ntime || p->bin_rows == 0 || p->src0 < 0 || p->src_stride < 0) return BB_EINVAL;
    if (p->npol > (1 << 20) || p->nchan > (1 << 20) || p->ntime > (1ull << 40)) return BB_ENOTSUP;
    const uint64_t R = (uint64_t)p->npol * (uint64_t)p->nchan * (uint64_t)p->ncomp;   // components of a time
    if (R > BB_MOMENTS_MAX_ROW) return BB_ENOTSUP;
    a->bin_elems = (uint32_t)R;
    a->pay_bytes = p->ntime * R;
    a->pitch = 0; a->nrun = 1; a->c_stride = 0; a->tf = 0; a->nchan = (uint32_t)p->nchan;
    a->P = 0; a->Rb = 0;
    if (p->layout == BB_MOMENTS_ROWS) {
        if (R == 1 || R == 2 || R == 4) a->P = (uint32_t)R;                   // one run; component = byte phase
        else if (R % 4 == 0) a->Rb = (uint32_t)R;
        else return BB_ENOTSUP;
        for (uint32_t j = 0; j < 4; ++j) a->ph_off[j] = a->P ? j % a->P : 0;
    } else {
        if (p->ncomp != 2 || p->npol > 2 || (p->layout == BB_MOMENTS_GUPPI_TF && p->npol != 2)) return BB_ENOTSUP;
        const uint32_t P = (uint32_t)p->npol * 2;                             // bytes per time of a channel
        if (p->layout == BB_MOMENTS_GUPPI_TF && p->nchan > 1) {
            a->Rb = (uint32_t)R; a->tf = 1;
        } else {                                                              // (time first with one channel is a run as well)
            a->P = P;
            if (p->layout == BB_MOMENTS_GUPPI_CF) { a->nrun = (uint32_t)p->nchan; a->pitch = p->ntime * P; a->c_stride = 2; }
        }
        for (uint32_t j = 0; j < 4; ++j) a->ph_off[j] = ((j % P) / 2) * (uint32_t)p->nchan * 2 + (j & 1);
    }
    if (((uint64_t)p->src0 | (uint64_t)p->src_stride | a->pitch) & 3) return BB_ENOTSUP;   // payloads and runs begin on dwords
    return BB_OK;
}

int bb_i8_moments_check(const bb_moments_params *p) { bb_moments_args a; return moments_params_check(p, &a); }

#define BB_MOMENTS_GRID 1024ull                      // workgroups: what 256 CUs hold at once at 4 waves per SIMD; every wave flushes at its end, and 2048 took twice as long on one bin

// What bb_i8_moments and bb_i8_coherence check at call time, in this order, after the parameters: the sums
// (`per_bin` int64 values a bin), the series' rows (*nrows == 0: nothing is asked for), the source
// -> the members of the kernel's arguments that do not depend on the access shape.
static int moments_request(bb_moments_args &a, const bb_moments_params *p, const void *d_buf, size_t buf_nbytes,
                           const int64_t *d_src, size_t nframes, int64_t *d_sums, size_t sums_elems, uint64_t per_bin,
                           uint64_t *nrows)
{
    if (!d_sums || ((uintptr_t)d_sums & 7)) return BB_EINVAL;
    if (p->nbins > (~0ull) / per_bin || sums_elems < p->nbins * per_bin) return BB_ERANGE;
    if (p->first_row > (1ull << 56)) return BB_ERANGE;
    a.nt = p->t_hi - p->t_lo;
    if (nframes && a.nt > (1ull << 56) / (uint64_t)nframes) return BB_ERANGE;
    *nrows = (uint64_t)nframes * a.nt;                                        // rows of the series that this call adds
    if (!*nrows) return BB_OK;
    if ((p->first_row + (*nrows - 1)) / p->bin_rows >= p->nbins) return BB_ERANGE;   // the last row's bin
    if (!d_buf) return BB_EINVAL;
    if ((uintptr_t)d_buf & 3) return BB_ENOTSUP;
    if (!d_src && (uint64_t)p->src_stride > (1ull << 62) / (uint64_t)nframes) return BB_ERANGE;
    const int rc = packed_source(a, d_buf, buf_nbytes, d_src, p->src0, p->src_stride, (uint64_t)nframes, a.pay_bytes);
    if (rc) return rc;
    a.sums = (long long *)d_sums;
    a.nframes = nframes;
    a.t_lo = p->t_lo;
    a.first_row = p->first_row; a.bin_rows = p->bin_rows; a.nbins = p->nbins;
    return BB_OK;
}

// The run form's split: a.nseg items of BB_MOM_RUN_STEPS wave loads per (run, frame).
static void moments_run_split(bb_moments_args &a)
{
    const uint64_t nst = (a.nt * a.P + 15 + BB_MOM_STEP - 1) / BB_MOM_STEP;   // wave loads of a run, at most
    a.nseg = (nst + BB_MOM_RUN_STEPS - 1) / BB_MOM_RUN_STEPS;
    a.NV = a.rpl = a.chunk_rows = 0;
}

// The row forms' split: `nv` lane columns of a row -> rows of a wave load, of an item, items per (column block,
// frame), column blocks (a.nrun).
static void moments_rows_split(bb_moments_args &a, uint32_t nv)
{
    a.NV = nv;
    a.rpl = a.NV < BB_WAVE ? BB_WAVE / a.NV : 1u;
    a.chunk_rows = a.rpl * BB_MOM_ROW_STEPS;
    a.nseg = (a.nt + a.chunk_rows - 1) / a.chunk_rows;
    a.nrun = (a.NV + BB_WAVE - 1) / BB_WAVE;
}

// 16 bytes per lane are possible where every row of every payload begins on 16 bytes
static bool moments_wide(const bb_moments_params *p, const void *d_buf, const int64_t *d_src)
{
    return !d_src && !((uintptr_t)d_buf & 15) && !(((uint64_t)p->src0 | (uint64_t)p->src_stride) & 15);
}

// a.nseg items per (unit, frame), a.nrun units -> a.nwork, a.per and *g workgroups: one contiguous range of
// items per wave, as many waves as the device holds at once
static int moments_ranges(bb_moments_args &a, size_t nframes, unsigned *g)
{
    const uint64_t units = a.nrun;                                            // runs or column blocks
    if (a.nseg > (~0ull) / (uint64_t)nframes || a.nseg * (uint64_t)nframes > (~0ull) / units) return BB_ERANGE;
    a.nwork = a.nseg * (uint64_t)nframes * units;
    const uint64_t waves = std::min<uint64_t>(a.nwork, BB_MOMENTS_GRID * BB_WAVES_PER_BLOCK);
    a.per = (a.nwork + waves - 1) / waves;
    const uint64_t ranges = (a.nwork + a.per - 1) / a.per;
    *g = (unsigned)((ranges + BB_WAVES_PER_BLOCK - 1) / BB_WAVES_PER_BLOCK);
    return BB_OK;
}

// What both entries do once the split is made: the wave ranges, the launch, the note of bb_last_kernel.
static int moments_launch(bb_moments_args &a, size_t nframes, void (*kernel)(bb_moments_args), const char *name,
                          const char *shape, void *stream)
{
    unsigned g;
    const int rc = moments_ranges(a, nframes, &g);
    if (rc) return rc;
    hipLaunchKernelGGL(kernel, dim3(g), dim3(BB_BLOCK), 0, (hipStream_t)stream, a);
    BB_NOTE("%s<%s> grid %u items %llu", name, shape, g, (unsigned long long)a.nwork);
    BB_HIP(hipGetLastError());
    return BB_OK;
}

int bb_i8_moments(const void *d_buf, size_t buf_nbytes, const int64_t *d_src, size_t nframes,
                  const bb_moments_params *p, int64_t *d_sums, size_t sums_elems, void *stream)
{
    bb_moments_args a;
    uint64_t nrows;
    int rc = moments_params_check(p, &a);
    if (rc) return rc;
    rc = moments_request(a, p, d_buf, buf_nbytes, d_src, nframes, d_sums, sums_elems, 2 * (uint64_t)a.bin_elems, &nrows);
    if (rc || !nrows) return rc;
    if (a.P) {
        a.mode = BB_MOM_RUN;
        moments_run_split(a);
    } else {
        const bool v4 = a.Rb % 16 == 0 && moments_wide(p, d_buf, d_src);
        a.mode = v4 ? BB_MOM_ROW4 : BB_MOM_ROW1;
        moments_rows_split(a, a.Rb / (v4 ? 16u : 4u));
    }
    return moments_launch(a, nframes, k_i8_moments, "k_i8_moments",
                          a.mode == BB_MOM_RUN ? "run" : a.mode == BB_MOM_ROW4 ? "rows16" : "rows4", stream);
}

// ---- cross-polarisation products per channel and time bin (k_coherence.h).  EXTENSION: no reference
//      counterpart.  The parameter block, the frame, first_row and bin rules are those of bb_i8_moments. ----
static int coherence_params_check(const bb_moments_params *p, bb_moments_args *a)
{
    const int rc = moments_params_check(p, a);
    if (rc) return rc;
    if (p->npol != 2 || p->ncomp != 2) return BB_ENOTSUP;                     // X and Y, both complex
    if (p->layout == BB_MOMENTS_ROWS && p->nchan > 1 && (p->nchan & 1)) return BB_ENOTSUP;   // the Y half begins inside a dword
    return BB_OK;
}

int bb_i8_coherence_check(const bb_moments_params *p) { bb_moments_args a; return coherence_params_check(p, &a); }

int bb_i8_coherence(const void *d_buf, size_t buf_nbytes, const int64_t *d_src, size_t nframes,
                    const bb_moments_params *p, int64_t *d_sums, size_t sums_elems, void *stream)
{
    bb_moments_args a;
    uint64_t nrows;
    int rc = coherence_params_check(p, &a);
    if (rc) return rc;
    rc = moments_request(a, p, d_buf, buf_nbytes, d_src, nframes, d_sums, sums_elems, 4 * (uint64_t)a.nchan, &nrows);
    if (rc || !nrows) return rc;
    if (a.P) {                                                                // 4: a run of quads per channel
        a.mode = BB_COH_RUN;
        moments_run_split(a);
    } else if (p->layout == BB_MOMENTS_GUPPI_TF) {                            // rows of nchan quads
        const bool v4 = a.Rb % 16 == 0 && moments_wide(p, d_buf, d_src);
        a.mode = v4 ? BB_COH_ROW4 : BB_COH_ROW1;
        moments_rows_split(a, a.Rb / (v4 ? 16u : 4u));
    } else {                                                                  // rows of an X and a Y half: lane columns of the X half
        const bool v4 = a.Rb % 32 == 0 && moments_wide(p, d_buf, d_src);
        a.mode = v4 ? BB_COH_SPLIT4 : BB_COH_SPLIT1;
        moments_rows_split(a, a.Rb / (v4 ? 32u : 8u));
    }
    static const char *const shape[] = {"run", "rows4", "rows16", "split4", "split16"};
    return moments_launch(a, nframes, k_i8_coherence, "k_i8_coherence", shape[a.mode], stream);
}
