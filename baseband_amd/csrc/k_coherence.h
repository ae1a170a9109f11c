// Cross-polarisation products from two-polarisation complex int8 block streams: per channel and
// time bin the sums of |X|^2, |Y|^2 and of X * conj(Y), straight from the stored bytes
// (bb_i8_coherence).  EXTENSION -- the reference has no counterpart: there the numbers come from
// a read followed by a reduction.  The sums of x * x of k_moments.h cannot give the cross term, so
// this is a pass of its own over the same bytes: the arguments, the work split and the two walks
// (bb_binned_run, bb_binned_rows) are those of k_moments.h, the accumulators are below.
//
// Per (bin, channel c) the kernel ADDS to sums[(bin * nchan + c) * 4 + k]
//     k = 0: sum xr * xr + xi * xi      1: sum yr * yr + yi * yi
//     k = 2: sum xr * yr + xi * yi      3: sum xi * yr - xr * yi       (Re, Im of X * conj(Y))
// with v_dot4 on a dword and masked or shifted copies of it.  A quad w = (xr, xi, yr, yi):
//     sdot4(w, w & 0x0000ffff), sdot4(w, w & 0xffff0000), sdot4(w, w >> 16),
//     sdot4(w, (w >> 8) & 0xff00) - sdot4(w, w >> 24)                  (logical shifts)
// The two halves of the imaginary part stay apart until both are int32: -yi is never formed in
// a byte (-(-128) is no int8).  Three access shapes, one kernel (a.mode, wave-uniform):
//
//   RUN   (GUPPI channels first; time first and plain rows with one channel): a run of quads
//         along time, one run per channel, 4 bytes per time.  Every sample is a whole dword, so
//         range and bin edges select dwords and no byte masks exist.  A wave adds its lanes up
//         into four int64 totals, one in each of its first four lanes.
//   ROWS  (GUPPI time first): rows of nchan quads; a lane owns the quads of V channels.
//   SPLIT (plain rows, nchan even): a row is [X: 2 nchan bytes][Y: 2 nchan bytes].  A lane pairs
//         V dwords of the X half (two channels each) with the dwords 2 nchan bytes behind them
//         (V = 4 where halves, offsets and the buffer are multiples of 16 bytes, else 1); with
//         x = (xr0, xi0, xr1, xi1) and y = (yr0, yi0, yr1, yi1) the lower channel takes
//         sdot4(x, x & 0xffff), sdot4(y, y & 0xffff), sdot4(x, y & 0xffff),
//         sdot4(x, (y << 8) & 0xff00) - sdot4(x, (y >> 8) & 0xff), the upper one the same masks
//         16 bits up.  Two groups of rows are in flight: four wave loads, as in the other shapes.
#pragma once
#include "k_moments.h"

#define BB_COH_RUN    0u
#define BB_COH_ROW1   1u
#define BB_COH_ROW4   2u
#define BB_COH_SPLIT1 3u
#define BB_COH_SPLIT4 4u
// A dword adds at most 2 * 128 * 128 = 2^15 to a partial (|X|^2 of (-128, -128); the halves of Im
// at most 2^14 each, their difference 2^15): twice what a byte phase of the moments kernel gets,
// so the folds come twice as often.  RUN: a lane adds at most 16 dwords a pass, so 32 passes give
// 32 * 16 * 2^15 = 2^24 a lane, 2^30 over the 64 lanes that the fold adds up in int32.
#define BB_COH_RUN_FOLD 32u
// ROWS, SPLIT: rows over ALL lanes; a channel gets at most 2^15 * 2^15 = 2^30, also after the lanes
// are added.  With 64 and 2^16 the bound would be 2^31 itself, which quads of -128 reach.
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

struct bb_coh_run_acc {
    static constexpr uint32_t FOLD = BB_COH_RUN_FOLD;
    int32_t s[5] = {0, 0, 0, 0, 0};                          // this lane's partials
    bb_i64 tot = 0;                                          // lane k < 4: the wave's total k

    static __device__ __forceinline__ uint32_t bytes_per_time(const bb_moments_args &) { return 4u; }
    // (payloads are whole dwords: the counted bytes end no further than they do)
    static __device__ __forceinline__ uint32_t payload_end(const bb_moments_args &, int64_t, int64_t, uint32_t hi) { return hi; }
    __device__ __forceinline__ void add(uint32_t w) { bb_coh_quad(w, s); }
    // (a dword of zeros adds nothing to any of the sums)
    __device__ __forceinline__ void add(uint32_t w, uint32_t rel, uint32_t lo, uint32_t n) { bb_coh_quad(rel - lo < n ? w : 0u, s); }
    __device__ __forceinline__ void fold(const int lane)
    {
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
    }
    __device__ __forceinline__ void flush(const bb_moments_args &a, const int lane, uint64_t c, uint64_t bin)
    {
        fold(lane);
        if (lane < 4 && bin < a.nbins)                       // (the host lets no counted row past nbins)
            bb_mom_atomic(a.sums + (bin * a.nchan + c) * 4u + (uint32_t)lane, tot);
        tot = 0;
    }
};

// What a lane loads of a row: V dwords (vec_t) of quads, or of the X half with their partners of the Y half.
template <class vec_t, bool SPLIT> struct bb_coh_row { vec_t x{}; };
template <class vec_t> struct bb_coh_row<vec_t, true> { vec_t x{}, y{}; };

// V dwords a lane: quads of V channels (SPLIT false), or V dwords of the X half, two channels
// each, with their partners of the Y half (SPLIT true).
template <int V_, bool SPLIT>
struct bb_coh_rows_acc {
    static constexpr int V = V_;
    static constexpr int C = SPLIT ? 2 * V : V;              // channels of a lane
    static constexpr int U = SPLIT ? BB_MOM_U / 2 : BB_MOM_U;
    static constexpr uint32_t FOLD = BB_COH_ROW_FOLD;
    typedef typename bb_mom_vec<V>::type vec_t;
    typedef bb_coh_row<vec_t, SPLIT> row_t;
    int32_t s[C][5] = {};                                    // this lane's partials, by channel

    static __device__ __forceinline__ row_t load(const bb_moments_args &a, const uint8_t *p)
    {
        row_t r;
        r.x = __builtin_nontemporal_load(reinterpret_cast<const vec_t *>(p));
        if constexpr (SPLIT) r.y = __builtin_nontemporal_load(reinterpret_cast<const vec_t *>(p + a.Rb / 2u));
        return r;
    }
    __device__ __forceinline__ void add(const row_t &v)
    {
#pragma unroll
        for (int d = 0; d < V; ++d) {
            if constexpr (SPLIT) bb_coh_pair(bb_mom_word(v.x, d), bb_mom_word(v.y, d), s[2 * d], s[2 * d + 1]);
            else       bb_coh_quad(bb_mom_word(v.x, d), s[d]);
        }
    }
    __device__ __forceinline__ void flush(const bb_moments_args &a, uint64_t bin, uint32_t vc, uint32_t off0, bool mine)
    {
#pragma unroll
        for (int c = 0; c < C; ++c) s[c][3] -= s[c][4];
        for (uint32_t off = off0; off < BB_WAVE; off <<= 1) {
#pragma unroll
            for (int c = 0; c < C; ++c)
#pragma unroll
                for (int k = 0; k < 4; ++k) s[c][k] += __shfl_xor(s[c][k], (int)off);
        }
        if (mine && bin < a.nbins) {                         // (the host lets no counted row past nbins)
            bb_i64 *out = a.sums + (bin * a.nchan + (uint64_t)vc * C) * 4u;
#pragma unroll
            for (int c = 0; c < C; ++c)
#pragma unroll
                for (int k = 0; k < 4; ++k) bb_mom_atomic(out + 4 * c + k, (bb_i64)s[c][k]);
        }
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int k = 0; k < 5; ++k) s[c][k] = 0;
    }
};

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
    case BB_COH_RUN:    bb_binned_run<bb_coh_run_acc>(a, lane, w, wend); break;
    case BB_COH_ROW1:   bb_binned_rows<bb_coh_rows_acc<1, false>>(a, lane, w, wend); break;
    case BB_COH_ROW4:   bb_binned_rows<bb_coh_rows_acc<4, false>>(a, lane, w, wend); break;
    case BB_COH_SPLIT1: bb_binned_rows<bb_coh_rows_acc<1, true>>(a, lane, w, wend); break;
    default:            bb_binned_rows<bb_coh_rows_acc<4, true>>(a, lane, w, wend); break;
    }
}
