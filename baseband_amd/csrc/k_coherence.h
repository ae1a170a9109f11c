// Cross-polarisation products from two-polarisation complex int8 block streams: per channel and
// time bin the sums of |X|^2, |Y|^2 and of X * conj(Y), straight from the stored bytes
// (bb_i8_coherence).  EXTENSION -- the reference has no counterpart: there the numbers come from
// a read followed by a reduction.  The companion of k_moments.h, whose arguments, work split and
// helpers it shares; the sums of x * x there cannot give the cross term, so this is a pass of
// its own over the same bytes.
//
// Shape (gfx950): a read-only stream, BB_MOM_U wave loads issued before the first use,
// nontemporal, int32 lane partials, int64 totals that leave as 64-bit atomics, no LDS.  Per
// (bin, channel c) the kernel ADDS to sums[(bin * nchan + c) * 4 + k]
//     k = 0: sum xr * xr + xi * xi      1: sum yr * yr + yi * yi
//     k = 2: sum xr * yr + xi * yi      3: sum xi * yr - xr * yi       (Re, Im of X * conj(Y))
// with v_dot4 on a dword and masked or shifted copies of it.  A quad w = (xr, xi, yr, yi):
//     sdot4(w, w & 0x0000ffff), sdot4(w, w & 0xffff0000), sdot4(w, w >> 16),
//     sdot4(w, (w >> 8) & 0xff00) - sdot4(w, w >> 24)                  (logical shifts)
// The two halves of the imaginary part stay apart until both are int32: -yi is never formed in
// a byte (-(-128) is no int8).  Three access shapes, one kernel (a.mode, wave-uniform):
//
//   RUN   (GUPPI channels first; time first and plain rows with one channel): a run of quads
//         along time, one run per channel.  The walk is that of the moments kernel's run form
//         with 4 bytes per time: 16-byte pieces of memory, a piece that is not wholly inside the
//         run loaded dword by dword; every sample is a whole dword, so range and bin edges
//         select dwords and no byte masks exist.  A group of wave loads that meets several bins
//         is walked once per bin over the loads that bin meets.  A wave adds its lanes up into
//         four int64 totals, one in each of its first four lanes.
//   ROWS  (GUPPI time first): rows of nchan quads.  A lane owns V quads of fixed channels (V = 4
//         where rows, offsets and the buffer are multiples of 16 bytes, else 1) and walks down
//         the rows; rows narrower than a wave load take several rows per load.
//   SPLIT (plain rows, nchan even): a row is [X: 2 nchan bytes][Y: 2 nchan bytes].  A lane pairs
//         V dwords of the X half (two channels each) with the dwords 2 nchan bytes behind them
//         (V = 4 where halves, offsets and the buffer are multiples of 16 bytes, else 1); with
//         x = (xr0, xi0, xr1, xi1) and y = (yr0, yi0, yr1, yi1) the lower channel takes
//         sdot4(x, x & 0xffff), sdot4(y, y & 0xffff), sdot4(x, y & 0xffff),
//         sdot4(x, (y << 8) & 0xff00) - sdot4(x, (y >> 8) & 0xff), the upper one the same masks
//         16 bits up.  Two groups of rows are in flight: four wave loads, as in the other shapes.
//   In both row shapes groups of loads end at bin edges, and the partials leave as atomics (lanes
//   on the same columns added up first where their number is a power of two) when the (column
//   block, bin) changes and at the wave's end.
//
// Widths.  A dword adds at most 2 * 128 * 128 = 2^15 to a partial (|X|^2 of (-128, -128); the
// halves of Im at most 2^14 each, their difference 2^15): twice what a byte phase of the moments
// kernel gets, so the folds come twice as often.  RUN folds after BB_COH_RUN_FOLD = 32 passes (a
// lane adds at most 16 dwords a pass: 32 * 16 * 2^15 = 2^24 a lane, 2^30 over the 64 lanes that
// the fold adds up in int32); the row shapes after at most BB_COH_ROW_FOLD = 2^15 rows over ALL
// lanes (a channel gets at most 2^15 * 2^15 = 2^30, also after the lanes are added).  With 64
// and 2^16 the bound would be 2^31 itself, which quads of -128 reach.  Everything that lives
// longer is int64.
//
// Work items, their numbering (unit-major, frames and pieces in time order inside) and a wave's
// contiguous range of them are those of k_i8_moments.
#pragma once
#include "k_moments.h"

#define BB_COH_RUN    0u
#define BB_COH_ROW1   1u
#define BB_COH_ROW4   2u
#define BB_COH_SPLIT1 3u
#define BB_COH_SPLIT4 4u
#define BB_COH_RUN_FOLD 32u
#define BB_COH_ROW_FOLD 32768u

// One quad (xr, xi, yr, yi) -> s: |X|^2, |Y|^2, Re, and the halves xi * yr, xr * yi of Im.
__device__ __forceinline__ void bb_coh_quad(uint32_t w, int32_t (&s)[5])
{
    s[0] = __builtin_amdgcn_sdot4((int)w, (int)(w & 0x0000ffffu), s[0], false);
    s[1] = __builtin_amdgcn_sdot4((int)w, (int)(w & 0xffff0000u), s[1], false);
    s[2] = __builtin_amdgcn_sdot4((int)w, (int)(w >> 16), s[2], false);
    s[3] = __builtin_amdgcn_sdot4((int)w, (int)((w >> 8) & 0x0000ff00u), s[3], false);
    s[4] = __builtin_amdgcn_sdot4((int)w, (int)(w >> 24), s[4], false);
}

// A dword of the X half and its partner of the Y half: two channels, lo and hi.
__device__ __forceinline__ void bb_coh_pair(uint32_t x, uint32_t y, int32_t (&lo)[5], int32_t (&hi)[5])
{
    lo[0] = __builtin_amdgcn_sdot4((int)x, (int)(x & 0x0000ffffu), lo[0], false);
    lo[1] = __builtin_amdgcn_sdot4((int)y, (int)(y & 0x0000ffffu), lo[1], false);
    lo[2] = __builtin_amdgcn_sdot4((int)x, (int)(y & 0x0000ffffu), lo[2], false);
    lo[3] = __builtin_amdgcn_sdot4((int)x, (int)((y << 8) & 0x0000ff00u), lo[3], false);
    lo[4] = __builtin_amdgcn_sdot4((int)x, (int)((y >> 8) & 0x000000ffu), lo[4], false);
    hi[0] = __builtin_amdgcn_sdot4((int)x, (int)(x & 0xffff0000u), hi[0], false);
    hi[1] = __builtin_amdgcn_sdot4((int)y, (int)(y & 0xffff0000u), hi[1], false);
    hi[2] = __builtin_amdgcn_sdot4((int)x, (int)(y & 0xffff0000u), hi[2], false);
    hi[3] = __builtin_amdgcn_sdot4((int)x, (int)((y << 8) & 0xff000000u), hi[3], false);
    hi[4] = __builtin_amdgcn_sdot4((int)x, (int)((y >> 8) & 0x00ff0000u), hi[4], false);
}

__device__ __forceinline__ void bb_coh_run(const bb_moments_args &a, const int lane, uint64_t w, const uint64_t wend)
{
    int32_t s[5] = {0, 0, 0, 0, 0};                          // this lane's partials of the current (run, bin)
    bb_i64 tot = 0;                                          // lane k < 4: the wave's total k of it
    uint32_t nacc = 0;                                       // passes since the last fold
    bool have = false;
    uint64_t cur_c = 0, cur_bin = 0;
    const uint64_t bin_bytes = a.bin_rows * 4u;
    const uint64_t per_c = a.nframes * a.nseg;

    auto fold = [&]() {
        s[3] -= s[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int32_t x = s[k];
#pragma unroll
            for (int off = 32; off; off >>= 1) x += __shfl_xor(x, off);
            if (lane == k) tot += x;
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) s[k] = 0;
        nacc = 0;
    };
    auto flush = [&]() {
        fold();
        if (lane < 4 && cur_bin < a.nbins)                   // (the host lets no counted row past nbins)
            bb_mom_atomic(a.sums + (cur_bin * a.nchan + cur_c) * 4u + (uint32_t)lane, tot);
        tot = 0;
    };

    uint64_t c = bb_mom_uniform(w / per_c);
    uint64_t fi = bb_mom_uniform((w - c * per_c) / a.nseg);
    uint64_t seg = w - c * per_c - fi * a.nseg;
    for (; w < wend; ++w) {
        const uint64_t c_ = c, fi_ = fi, seg_ = seg;
        if (++seg == a.nseg) { seg = 0; if (++fi == a.nframes) { fi = 0; ++c; } }   // (the item after this one)
        const int64_t so = bb_src_at(a, fi_);
        if (!bb_src_ok(so, a.src_lim) || (so & 3)) continue; // missing, outside the buffer or not on a dword: adds nothing
        // offsets into the buffer: the run's counted bytes [A0, A1), the 16-byte boundary of memory at or below A0
        const int64_t A0 = so + (int64_t)(c_ * a.pitch + a.t_lo * 4u), A1 = A0 + (int64_t)(a.nt * 4u);
        const int64_t base = A0 - (int64_t)((reinterpret_cast<uintptr_t>(a.buf) + (uint64_t)A0) & 15u);
        const uint64_t nst = ((uint64_t)(A1 - base) + BB_MOM_STEP - 1) / BB_MOM_STEP;   // (a shift)
        uint64_t st = seg_ * BB_MOM_RUN_STEPS;
        if (st >= nst) continue;
        const uint64_t st_end = st + BB_MOM_RUN_STEPS < nst ? st + BB_MOM_RUN_STEPS : nst;
        // where the item's first counted byte lies in the run's series
        const int64_t x0 = base + (int64_t)(st * BB_MOM_STEP) > A0 ? base + (int64_t)(st * BB_MOM_STEP) : A0;
        const uint64_t g = (a.first_row + fi_ * a.nt) * 4u + (uint64_t)(x0 - A0);
        uint64_t bin = bb_mom_uniform(g / bin_bytes);
        uint64_t left = bin_bytes - (g - bin * bin_bytes);
#pragma nounroll
        for (; st < st_end; st += BB_MOM_U) {                // a group of BB_MOM_U wave loads
            const int64_t gb = base + (int64_t)(st * BB_MOM_STEP);
            const uint8_t *gp = a.buf + gb;                  // (nothing in front of the payload is read)
            // the group's counted bytes [lo, hi), whole dwords, relative to the group
            uint32_t lo = gb < A0 ? (uint32_t)(A0 - gb) : 0u;
            const uint64_t gend = (st_end - st < BB_MOM_U ? st_end - st : BB_MOM_U) * BB_MOM_STEP;
            const uint32_t hi = (uint64_t)(A1 - gb) < gend ? (uint32_t)(A1 - gb) : (uint32_t)gend;
            bb_u4 v[BB_MOM_U];
#pragma unroll
            for (int u = 0; u < BB_MOM_U; ++u)               // (payloads are whole dwords: hi is no further than their end)
                v[u] = bb_mom_piece(gp, (uint32_t)u * BB_MOM_STEP + 16u * (uint32_t)lane, lo, hi, hi);
            if (lo == 0u && hi == BB_MOM_U * BB_MOM_STEP && left >= hi) {
                // the whole group lies in one bin: every dword counts
                if (!have || c_ != cur_c || bin != cur_bin) {
                    if (have) flush();
                    have = true; cur_c = c_; cur_bin = bin;
                }
#pragma unroll
                for (int u = 0; u < BB_MOM_U; ++u) {
                    bb_coh_quad(v[u].x, s); bb_coh_quad(v[u].y, s);
                    bb_coh_quad(v[u].z, s); bb_coh_quad(v[u].w, s);
                }
                if (++nacc >= BB_COH_RUN_FOLD) fold();
                left -= hi;
                if (left == 0) { ++bin; left = bin_bytes; }
                continue;
            }
#pragma nounroll
            while (lo < hi) {                                // bin after bin: the dwords of [lo, lo + n)
                const uint32_t n = (uint64_t)(hi - lo) < left ? hi - lo : (uint32_t)left;
                if (!have || c_ != cur_c || bin != cur_bin) {
                    if (have) flush();
                    have = true; cur_c = c_; cur_bin = bin;
                }
#pragma unroll
                for (int u = 0; u < BB_MOM_U; ++u) {
                    const uint32_t s0 = (uint32_t)u * BB_MOM_STEP;
                    if (lo + n <= s0 || lo >= s0 + BB_MOM_STEP) continue;    // (wave-uniform: a load that this bin does not meet)
                    const uint32_t rel = s0 + 16u * (uint32_t)lane;
                    // (a dword of zeros adds nothing to any of the sums)
                    bb_coh_quad(rel - lo < n ? v[u].x : 0u, s);
                    bb_coh_quad(rel + 4u - lo < n ? v[u].y : 0u, s);
                    bb_coh_quad(rel + 8u - lo < n ? v[u].z : 0u, s);
                    bb_coh_quad(rel + 12u - lo < n ? v[u].w : 0u, s);
                }
                if (++nacc >= BB_COH_RUN_FOLD) fold();
                lo += n;
                left -= n;
                if (left == 0) { ++bin; left = bin_bytes; }
            }
        }
    }
    if (have) flush();
}

// V dwords a lane: quads of V channels (SPLIT false), or V dwords of the X half, two channels
// each, with their partners of the Y half (SPLIT true).
template <int V, bool SPLIT>
__device__ __forceinline__ void bb_coh_rows(const bb_moments_args &a, const int lane, uint64_t w, const uint64_t wend)
{
    typedef typename bb_mom_vec<V>::type vec_t;
    constexpr int C = SPLIT ? 2 * V : V;                     // channels of a lane
    constexpr int U = SPLIT ? BB_MOM_U / 2 : BB_MOM_U;       // groups of rows in flight: BB_MOM_U wave loads
    int32_t s[C][5];                                         // this lane's partials of the current (column block, bin)
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int k = 0; k < 5; ++k) s[c][k] = 0;
    uint32_t nacc = 0;                                       // rows since the last flush, over all lanes
    bool have = false;
    uint64_t cur_cb = 0, cur_bin = 0;
    const uint32_t NV = a.NV;
    const uint32_t dr = NV < BB_WAVE ? (uint32_t)lane / NV : 0u;                        // row of a wave load that this lane reads
    const uint32_t lc = NV < BB_WAVE ? (uint32_t)lane - dr * NV : (uint32_t)lane;      // ... and its lane column in the block
    const bool pow2 = NV < BB_WAVE && (NV & (NV - 1u)) == 0; // lanes NV apart share columns, all 64 read: add them up by shuffles
    const uint64_t per_cb = a.nframes * a.nseg;
    const uint32_t half = a.Rb / 2u;                         // SPLIT: bytes from a dword of X to its partner of Y

    auto flush = [&]() {
        const uint32_t vc = (uint32_t)cur_cb * BB_WAVE + lc;
#pragma unroll
        for (int c = 0; c < C; ++c) s[c][3] -= s[c][4];
        if (pow2) {
            for (uint32_t off = NV; off < BB_WAVE; off <<= 1) {
#pragma unroll
                for (int c = 0; c < C; ++c)
#pragma unroll
                    for (int k = 0; k < 4; ++k) s[c][k] += __shfl_xor(s[c][k], (int)off);
            }
        }
        const bool mine = pow2 ? dr == 0 : (vc < NV && dr < a.rpl);
        if (mine && cur_bin < a.nbins) {                     // (the host lets no counted row past nbins)
            bb_i64 *out = a.sums + (cur_bin * a.nchan + (uint64_t)vc * C) * 4u;
#pragma unroll
            for (int c = 0; c < C; ++c)
#pragma unroll
                for (int k = 0; k < 4; ++k) bb_mom_atomic(out + 4 * c + k, (bb_i64)s[c][k]);
        }
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int k = 0; k < 5; ++k) s[c][k] = 0;
        nacc = 0;
    };

    uint64_t cb = bb_mom_uniform(w / per_cb);
    uint64_t fi = bb_mom_uniform((w - cb * per_cb) / a.nseg);
    uint64_t seg = w - cb * per_cb - fi * a.nseg;
    for (; w < wend; ++w) {
        const uint64_t cb_ = cb, fi_ = fi, seg_ = seg;
        if (++seg == a.nseg) { seg = 0; if (++fi == a.nframes) { fi = 0; ++cb; } }   // (the item after this one)
        const int64_t so = bb_src_at(a, fi_);
        if (!bb_src_ok(so, a.src_lim) || (so & (4 * V - 1))) continue;   // missing, outside the buffer or not aligned: adds nothing
        const uint32_t vc = (uint32_t)cb_ * BB_WAVE + lc;
        const bool col_ok = vc < NV && dr < a.rpl;
        uint64_t r = a.t_lo + seg_ * a.chunk_rows;
        const uint64_t t_hi = a.t_lo + a.nt;
        const uint64_t rb = r + a.chunk_rows < t_hi ? r + a.chunk_rows : t_hi;
        const uint64_t g = a.first_row + fi_ * a.nt + (r - a.t_lo);
        uint64_t bin = bb_mom_uniform(g / a.bin_rows);
        uint64_t left = a.bin_rows - (g - bin * a.bin_rows);
        const uint8_t *pl = a.buf + (uint64_t)so + (uint64_t)vc * (4u * V);             // this lane's columns in row 0
#pragma nounroll
        while (r < rb) {
            // U groups of rpl rows: they end at the item's last row and at a bin edge
            uint64_t m64 = rb - r < left ? rb - r : left;
            if (m64 > (uint64_t)U * a.rpl) m64 = (uint64_t)U * a.rpl;
            const uint32_t m = (uint32_t)m64;
            if (!have || cb_ != cur_cb || bin != cur_bin || nacc + m > BB_COH_ROW_FOLD) {
                if (have) flush();
                have = true; cur_cb = cb_; cur_bin = bin;
            }
            vec_t x[U], y[SPLIT ? U : 1];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t row = (uint32_t)u * a.rpl + dr;
                x[u] = vec_t{};
                if constexpr (SPLIT) y[u] = vec_t{};
                if (col_ok && row < m) {
                    const uint8_t *p = pl + (r + row) * a.Rb;
                    x[u] = __builtin_nontemporal_load(reinterpret_cast<const vec_t *>(p));
                    if constexpr (SPLIT) y[u] = __builtin_nontemporal_load(reinterpret_cast<const vec_t *>(p + half));
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int d = 0; d < V; ++d) {
                    if constexpr (SPLIT) bb_coh_pair(bb_mom_word(x[u], d), bb_mom_word(y[u], d), s[2 * d], s[2 * d + 1]);
                    else       bb_coh_quad(bb_mom_word(x[u], d), s[d]);
                }
            nacc += m;
            r += m;
            left -= m;
            if (left == 0) { ++bin; left = a.bin_rows; }
        }
    }
    if (have) flush();
}

__global__ __launch_bounds__(BB_BLOCK, 4)                    // at least 4 waves per SIMD: 128 VGPRs at most
void k_i8_coherence(bb_moments_args a)
{
    const int lane = bb_lane();
    const int wave = __builtin_amdgcn_readfirstlane(bb_wave());
    // this wave's contiguous range of work items
    const uint64_t w = ((uint64_t)blockIdx.x * BB_WAVES_PER_BLOCK + (uint64_t)wave) * a.per;
    if (w >= a.nwork) return;
    const uint64_t wend = a.nwork - w < a.per ? a.nwork : w + a.per;
    switch (a.mode) {                                        // (wave-uniform)
    case BB_COH_RUN:    bb_coh_run(a, lane, w, wend); break;
    case BB_COH_ROW1:   bb_coh_rows<1, false>(a, lane, w, wend); break;
    case BB_COH_ROW4:   bb_coh_rows<4, false>(a, lane, w, wend); break;
    case BB_COH_SPLIT1: bb_coh_rows<1, true>(a, lane, w, wend); break;
    default:            bb_coh_rows<4, true>(a, lane, w, wend); break;
    }
}
