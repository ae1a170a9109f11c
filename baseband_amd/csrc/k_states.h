// Sampler statistics: how often each raw code occurs per (thread slot, position in
// the row), counted from the packed bytes (bb_count_states).  EXTENSION -- the
// reference has no counterpart; a "code" is a field of the payload taken LSB first,
// the order of vdif/payload.py:25-103 and mark5b/payload.py:27-94.
//
// Shape (gfx950): the kernel reads every payload byte once and writes a few dozen
// integers, so it is a read-only stream.  It does not count codes but BYTES: a
// histogram of 256 byte values x P byte phases in LDS, P = max(1, chunk * bps / 8)
// being the bytes of one row (the byte at payload offset q holds the same row
// positions as the one at q + P), at most 16.  One LDS add per byte instead of 8 / bps,
// and the expansion to code counts happens once, when the workgroup ends.  Every wave
// owns a copy of the histogram, so the waves of a workgroup neither collide nor meet
// at a barrier while they stream; a wave walks work items of at most 4 KiB of one
// frame-slot (four 16-byte loads per lane, all issued before the first add).  A wave
// load, whole or partial, that repeats one dword throughout (a fill pattern, a dead
// channel) is added by a few lanes in one step: 64 lanes on one LDS address would
// serialise.  Payloads
// may lie at any byte address: the bytes in front of and behind the 16-byte aligned
// middle of a work item are read one by one, nothing outside the payload is read.
// When a row is shorter than a byte (chunk * bps < 8) a row range can begin or end
// inside a byte; those at most two bytes per frame-slot are counted field by field
// into 16 bins of their own.
//
// A workgroup counts ONE thread slot (blockIdx.x % nslot).  At its end it sums the
// four copies into code counts -- 64-bit, the on-chip counters are 32-bit and the host
// sizes the grid so that none can wrap -- and adds each non-zero one to d_counts with
// one 64-bit integer atomic: integer adds commute, the result is the same bit for bit
// whatever the order.
#pragma once
#include "bb_common.h"

#define BB_STATES_NL 4                                       // 16-byte loads per lane and work item
#define BB_STATES_SEG (BB_STATES_NL * BB_WAVE * 16u)         // bytes of a work item, at most
#define BB_STATES_MAX_PHASES 16u

struct bb_states_args {
    const uint8_t *buf;
    const int64_t *src;          // payload offsets, NULL: src0 + (f * nslot + slot) * src_stride
    unsigned long long *counts;
    uint64_t src_lim;            // bb_src_ok
    int64_t  src0, src_stride;
    uint64_t payload;            // bytes per frame-slot
    uint64_t R;                  // rows per frame
    uint64_t row_lo, row_hi;     // rows of the request that count
    uint64_t f_lo;               // first frame with such a row
    uint64_t nwork;              // (frames with such a row) * nseg
    uint32_t nseg, seg_bytes;    // work items per frame-slot, bytes of each (a multiple of 16)
    uint32_t nslot, chunk;
    uint32_t bps, lbps;
    uint32_t lphase;             // log2(P)
};

__device__ __forceinline__ void bb_states_add16(uint32_t *hist, const bb_u4 &v, uint32_t lP, uint32_t pm, uint32_t phA)
{
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t ph = (phA + (uint32_t)(4 * i + j)) & pm;          // (wave-uniform)
            atomicAdd(&hist[(((w[i] >> (8 * j)) & 0xffu) << lP) + ph], 1u);
        }
    }
}

// ---- a work item's bytes [p0, p0 + n) as this kernel and k_count_state_bins walk them (above).  The helpers
// are cut where both kernels keep the instructions of the text written out (tools/check_isa.py --against) ----
struct bb_pieces { uint32_t nhead, nmid, ntail; };           // bytes in front, 16-byte pieces, bytes behind

__device__ __forceinline__ bb_pieces bb_pieces_split(const uint8_t *p0, uint32_t n)
{
    const uint32_t mis = (uint32_t)reinterpret_cast<uintptr_t>(p0) & 15u;
    uint32_t nhead = mis ? 16u - mis : 0u;
    if (nhead > n) nhead = n;
    const uint32_t nmid = (n - nhead) >> 4;
    return bb_pieces{nhead, nmid, n - nhead - (nmid << 4)};
}

// Piece c of the middle, zero past the last.  A lane loads its BB_STATES_NL pieces k * BB_WAVE + lane before the first add.
__device__ __forceinline__ void bb_piece_load(bb_u4 &v, const bb_u4 *pmid, uint32_t nmid, uint32_t c)
{
    v = bb_u4{0u, 0u, 0u, 0u};
    if (c < nmid) v = pmid[c];
}

// The bytes around the middle, one per lane: lanes 0-31 the head, 32-63 the tail -> this lane has p0[off].
__device__ __forceinline__ bool bb_pieces_edge_byte(bb_pieces x, int lane, uint32_t &off)
{
    const uint32_t t = (uint32_t)lane & 31u;
    off = lane < 32 ? t : x.nhead + (x.nmid << 4) + t;
    return t < (lane < 32 ? x.nhead : x.ntail);
}

// A piece repeats the dword W; a wave load does when __all of its lanes that hold a piece say so.
__device__ __forceinline__ bool bb_piece_repeats(const bb_u4 &v, uint32_t W) { return v.x == W && v.y == W && v.z == W && v.w == W; }

__global__ __launch_bounds__(BB_BLOCK)
void k_count_states(bb_states_args a)
{
    extern __shared__ uint32_t s_states[];
    const int lane = bb_lane();
    const int wave = __builtin_amdgcn_readfirstlane(bb_wave());
    const uint32_t lP = a.lphase, pm = (1u << lP) - 1u;
    const uint32_t cb = a.chunk << a.lbps;                   // bits per row
    uint32_t *hist = s_states + ((uint32_t)wave << (8 + lP));
    uint32_t *s_edge = s_states + ((uint32_t)BB_WAVES_PER_BLOCK << (8 + lP));   // (only there when cb < 8)
    for (uint32_t i = lane; i < (256u << lP); i += BB_WAVE) hist[i] = 0;
    if (cb < 8 && threadIdx.x < 16) s_edge[threadIdx.x] = 0;
    __syncthreads();

    const uint32_t slot = blockIdx.x % a.nslot;
    const uint64_t nwaves = (uint64_t)(gridDim.x / a.nslot) * BB_WAVES_PER_BLOCK;
    const uint32_t mask = (1u << a.bps) - 1u;
    for (uint64_t w = (uint64_t)(blockIdx.x / a.nslot) * BB_WAVES_PER_BLOCK + (uint64_t)wave; w < a.nwork; w += nwaves) {
        const uint64_t fr = a.nseg == 1 ? w : w / a.nseg;
        const uint32_t seg = (uint32_t)(w - fr * a.nseg);
        const uint64_t f = a.f_lo + fr;
        const uint64_t fs = f * a.nslot + slot;
        const int64_t so = bb_src_at(a, fs);
        if (!bb_src_ok(so, a.src_lim)) continue;             // missing, invalid or outside the buffer: counts nothing
        // the bits of this frame-slot that count
        const uint64_t g0 = f * a.R;
        const uint64_t r0 = a.row_lo > g0 ? a.row_lo - g0 : 0;
        const uint64_t r1 = a.row_hi - g0 < a.R ? a.row_hi - g0 : a.R;
        const uint64_t bit0 = r0 * cb, bit1 = r1 * cb;
        const uint8_t *pay = a.buf + (uint64_t)so;
        if (cb < 8 && seg == 0 && lane < 2) {
            // a range that begins or ends inside a byte: that byte field by field
            const uint32_t f0 = (uint32_t)bit0 & 7u, f1 = (uint32_t)bit1 & 7u;
            const uint64_t y0 = bit0 >> 3, y1 = bit1 >> 3;
            const bool on = lane == 0 ? f0 != 0 : (f1 != 0 && !(f0 != 0 && y0 == y1));
            if (on) {
                const uint32_t v = pay[lane == 0 ? y0 : y1];
                const uint32_t lo = lane == 0 ? f0 : 0u, hi = (lane == 0 && y1 != y0) ? 8u : f1;
                for (uint32_t b = lo; b < hi; b += a.bps)
                    atomicAdd(&s_edge[((((b >> a.lbps) & (a.chunk - 1u)) << a.bps)) + ((v >> b) & mask)], 1u);
            }
        }
        // whole bytes [q0, q1) of this work item
        uint64_t q0 = (uint64_t)seg * a.seg_bytes, q1 = q0 + a.seg_bytes;
        const uint64_t B0 = (bit0 + 7) >> 3, B1 = bit1 >> 3;
        if (q0 < B0) q0 = B0;
        if (q1 > B1) q1 = B1;
        if (q0 >= q1) continue;
        const uint32_t n = (uint32_t)(q1 - q0);
        const uint8_t *p0 = pay + q0;
        const bb_pieces x = bb_pieces_split(p0, n);
        const bb_u4 *pmid = reinterpret_cast<const bb_u4 *>(p0 + x.nhead);
        bb_u4 v[BB_STATES_NL];
#pragma unroll
        for (int k = 0; k < BB_STATES_NL; ++k) bb_piece_load(v[k], pmid, x.nmid, (uint32_t)k * BB_WAVE + (uint32_t)lane);
        uint32_t off;
        if (bb_pieces_edge_byte(x, lane, off)) {
            const uint32_t b = p0[off];
            atomicAdd(&hist[(b << lP) + (((uint32_t)q0 + off) & pm)], 1u);
        }
        const uint32_t phA = ((uint32_t)q0 + x.nhead) & pm;     // phase of a piece's first byte: pieces are 16 bytes apart, P divides 16
#pragma unroll
        for (int k = 0; k < BB_STATES_NL; ++k) {
            const uint32_t k0 = (uint32_t)k * BB_WAVE;
            if (k0 >= x.nmid) break;
            const uint32_t W = (uint32_t)__builtin_amdgcn_readfirstlane((int)v[k].x);     // (lane 0 holds a piece: k0 < x.nmid)
            const uint32_t nv = x.nmid - k0 < BB_WAVE ? x.nmid - k0 : BB_WAVE;            // pieces of this load
            if (__all((uint32_t)lane >= nv || bb_piece_repeats(v[k], W))) {
                // nv pieces that repeat one dword: byte j of it 4 * nv times, dealt evenly over the phases it meets
                const uint32_t Q = lP > 2 ? 1u << (lP - 2) : 1u;
                if ((uint32_t)lane < 4u * Q) {
                    const uint32_t j = (uint32_t)lane & 3u, m = (uint32_t)lane >> 2;
                    atomicAdd(&hist[(((W >> (8 * j)) & 0xffu) << lP) + ((phA + 4u * m + j) & pm)], 4u * nv / Q);
                }
            } else if (k0 + (uint32_t)lane < x.nmid) {
                bb_states_add16(hist, v[k], lP, pm, phA);
            }
        }
    }
    __syncthreads();

    // byte counts -> code counts: bin (position, code) sums the byte values that carry
    // `code` in the field(s) of that position, over the four copies
    const uint32_t nbins = a.chunk << a.bps;
    const uint32_t fpb = 8u >> a.lbps, lfpb = 3u - a.lbps;    // fields per byte
    const uint32_t kstep = a.chunk < fpb ? a.chunk : fpb;
    for (uint32_t nb = threadIdx.x; nb < nbins; nb += BB_BLOCK) {
        const uint32_t pos = nb >> a.bps, c = nb & mask;
        const uint32_t p = a.chunk >= fpb ? pos >> lfpb : 0u;
        uint64_t sum = cb < 8 ? s_edge[nb] : 0u;
        for (uint32_t k = pos & (kstep - 1u); k < fpb; k += kstep) {
            const uint32_t kb = k << a.lbps;
            for (uint32_t i = 0; i < (256u >> a.bps); ++i) {
                const uint32_t bv = ((i >> kb) << (kb + a.bps)) | (c << kb) | (i & ((1u << kb) - 1u));
#pragma unroll
                for (uint32_t wv = 0; wv < BB_WAVES_PER_BLOCK; ++wv)
                    sum += s_states[(wv << (8 + lP)) + (bv << lP) + p];
            }
        }
        if (sum)
            __hip_atomic_fetch_add(a.counts + (uint64_t)slot * nbins + nb, (unsigned long long)sum,
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
