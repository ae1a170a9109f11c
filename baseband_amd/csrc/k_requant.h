// Conversion between sample widths on the packed bytes (bb_requant_frames): decode, one
// float32 gain, encode -- applied back to back that is an exact function from input code
// to output code, a table of at most 256 entries that the caller supplies.  No float is
// ever in HBM: N bytes in, N * bps_out / bps_in out.
//
// Both sides have the same slot structure (nslot payloads per frame, chunk codes per row),
// so a slot's payloads, frame after frame, are ONE stream of codes on either side: code n of
// the output stream is code n + D of the input stream, D = (row_lo - first_row) * chunk.
// Fields are LSB first.
//
// Shape (gfx950): a work item is a run of one OUTPUT frame and slot, 8 KiB of the wider
// side, and belongs to one wave.  A lane makes 16 output bytes at a time, which leave as one
// 16-byte store (payloads are multiples of 4: the destination is a dword boundary).  They
// draw from 16 * bps_in / bps_out input bytes, taken as 16-byte pieces: one 16-byte load
// from the address aligned down to a dword plus the dword behind it, the misalignment (whole
// bytes, and where the output is the wider side -- 1 -> 4, 1 -> 8, 2 -> 8, 4 -> 8 bits: a byte
// of output is less than a byte of input -- up to 7 bits more) shifted out in registers.
// A piece whose source counts nothing gives the fill pattern.  Pieces that meet a frame
// boundary of the input or the last bytes of the buffer, and the output bytes at the edge of
// the request, are walked code by code; bytes outside the rows of the request are never
// written and nothing outside the buffer is read.
//
// The lookup: tables of bps_in <= 4 (at most 16 entries of 8 bits) live in scalar registers
// and are a shift and a mask; the 256 entries of bps_in == 8 lie in LDS on a 256-byte
// boundary, one dword per bank, so two lanes on one bank always read the same dword: no
// conflicts, one LDS read per input byte.  The widths are wave-uniform run-time values: the
// kernel picks one of 16 unrolled loops per launch (ONE kernel in the code object).
#pragma once
#include "bb_common.h"

#define BB_REQUANT_ITEM_BYTES 8192u                          // bytes of a work item on its wider side
#define BB_REQUANT_MAX_SLOTS 32u
#define BB_REQUANT_MAX_ROW_BITS 256u

struct bb_requant_args {
    const uint8_t *buf;
    const int64_t *src;          // payload offsets, NULL: src0 + (f * nslot + slot) * src_stride
    uint8_t *out;
    uint64_t buf_n;              // bytes of buf
    uint64_t src_lim;            // bb_src_ok
    int64_t  src0, src_stride;
    uint64_t pay_in, pay_out;    // bytes per frame-slot
    uint64_t ya, yb;             // bytes [ya, yb) of a slot's output stream are written
    uint64_t xbit_a;             // bit of a slot's input stream that byte ya begins with
    uint64_t F0;                 // first output frame with a written byte
    uint64_t nseg;               // work items per output payload
    uint64_t nwork;
    uint32_t seg;                // output bytes per work item, a multiple of 16
    uint32_t nslot;
    uint32_t lbi, lbo;           // log2(bps), in and out
    uint32_t fillw;              // fill_code in every field of an output dword
    uint32_t map[64];            // uint8 map[256]
};

typedef uint32_t bb_u4d __attribute__((ext_vector_type(4), aligned(4)));     // 16 bytes on a dword boundary

// map[c]; s_map: the table in LDS (8-bit codes only).  Args: bb_requant_args, or k_recode's, which hold `map` alike.
template <int LBI, class Args>
__device__ __forceinline__ uint32_t bb_requant_map(const Args &a, const uint8_t *s_map, uint32_t c)
{
    if constexpr (LBI == 3) return s_map[c];
    else if constexpr (LBI == 2) {
        const uint32_t lo = (c & 4u) ? a.map[1] : a.map[0], hi = (c & 4u) ? a.map[3] : a.map[2];
        return (((c & 8u) ? hi : lo) >> ((c & 3u) << 3)) & 0xffu;
    }
    else return (a.map[0] >> (c << 3)) & 0xffu;
}

// (f, off) with off beyond the frame's bits -> the frame it lies in.  One step is the common
// case (an item is seldom longer than a frame); a 64-bit division costs some 200 operations.
__device__ __forceinline__ void bb_requant_frame_of(uint64_t &f, uint64_t &off, uint64_t paybits)
{
    if (off < paybits) return;
    off -= paybits; ++f;
    if (off < paybits) return;
    const uint64_t d = ((off | paybits) >> 32) == 0 ? (uint64_t)((uint32_t)off / (uint32_t)paybits) : off / paybits;
    f += d; off -= d * paybits;
}

// `nb` <= 16 output bytes from bit `off` of frame f of slot s's input on, code by code, across
// frame boundaries -> r0 (bytes 0..7), r1 (8..15).
template <int LBI>
__device__ __forceinline__ void bb_requant_walk(const bb_requant_args &a, const uint8_t *s_map, uint32_t s,
                                                uint64_t f, uint64_t off, uint32_t nb, uint64_t &r0, uint64_t &r1)
{
    const uint64_t paybits = a.pay_in << 3;
    bb_requant_frame_of(f, off, paybits);
    int64_t so = a.src ? a.src[f * a.nslot + s] : a.src0 + (int64_t)(f * a.nslot + s) * a.src_stride;
    bool ok = bb_src_ok(so, a.src_lim);
    const uint32_t cpo = 8u >> a.lbo, fill = a.fillw & ((1u << (1u << a.lbo)) - 1u);
    r0 = 0; r1 = 0;
#pragma unroll 1
    for (uint32_t b = 0; b < nb; ++b) {
        uint32_t ob = 0;
#pragma unroll 1
        for (uint32_t i = 0; i < cpo; ++i) {
            if (off >= paybits) {                                        // (codes never straddle a payload: exactly its end)
                off = 0; ++f;
                so = a.src ? a.src[f * a.nslot + s] : a.src0 + (int64_t)(f * a.nslot + s) * a.src_stride;
                ok = bb_src_ok(so, a.src_lim);
            }
            uint32_t m = fill;
            if (ok) {
                const uint32_t c = ((uint32_t)a.buf[(uint64_t)so + (off >> 3)] >> ((uint32_t)off & 7u)) & ((1u << (1u << LBI)) - 1u);
                m = bb_requant_map<LBI>(a, s_map, c);
            }
            ob |= m << (i << a.lbo);
            off += 1u << LBI;
        }
        if (b < 8u) r0 |= (uint64_t)ob << (8u * b);
        else        r1 |= (uint64_t)ob << (8u * (b - 8u));
    }
}

// The codes of NIN input bits in w[] -> their output bits in o[] (both from bit 0 on).
template <int LBI, int LBO, int NIN>
__device__ __forceinline__ void bb_requant_codes(const bb_requant_args &a, const uint8_t *s_map,
                                                 const uint32_t (&w)[4], uint32_t (&o)[4])
{
    constexpr uint32_t BI = 1u << LBI, BO = 1u << LBO, MI = (1u << BI) - 1u;
#pragma unroll
    for (int d = 0; d < 4; ++d) o[d] = 0;
#pragma unroll
    for (uint32_t n = 0; n < (uint32_t)NIN / BI; ++n) {
        const uint32_t c = (w[(n * BI) >> 5] >> ((n * BI) & 31u)) & MI;
        o[(n * BO) >> 5] |= bb_requant_map<LBI>(a, s_map, c) << ((n * BO) & 31u);
    }
}

// The output bytes [va, vb) of the item whose payload bytes from e_lo on lie at dst; the
// input bit of byte va is bit offu of frame fu.
template <int LBI, int LBO>
__device__ __forceinline__ void bb_requant_item(const bb_requant_args &a, const uint8_t *s_map, uint8_t *dst, uint32_t s,
                                                uint32_t va, uint32_t vb, uint64_t fu, uint64_t offu, uint32_t lane)
{
    constexpr int LS = LBI - LBO;
    constexpr int NSUB = LS > 0 ? 1 << LS : 1;                           // 16-byte input pieces per 16 output bytes
    constexpr int NIN = LS >= 0 ? 128 : 128 >> -LS;                      // input bits of a piece that are used
    constexpr uint32_t OUTB = LS > 0 ? 16u >> LS : 16u;                  // output bytes of a piece
    const uint64_t paybits = a.pay_in << 3;
    const uint32_t q1 = (vb + 15u) >> 4;
    for (uint32_t q = (va >> 4) + lane; q < q1; q += BB_WAVE) {
        const uint32_t e0 = q << 4;
        if (e0 >= va && e0 + 16u <= vb) {
            uint32_t v[4] = {0u, 0u, 0u, 0u};
            const uint64_t off0 = offu + ((((uint64_t)(e0 - va) << 3) >> LBO) << LBI);
#pragma unroll
            for (int j = 0; j < NSUB; ++j) {
                uint64_t f = fu, off = off0 + 128u * (uint32_t)j;
                bb_requant_frame_of(f, off, paybits);
                uint32_t o[4];
                bool done = false;
                if (off + (uint32_t)NIN <= paybits) {
                    const uint64_t fs = f * a.nslot + s;
                    const int64_t so = bb_src_at(a, fs);
                    if (!bb_src_ok(so, a.src_lim)) {
                        o[0] = o[1] = o[2] = o[3] = a.fillw;
                        done = true;
                    } else {
                        const uint64_t ob = (uint64_t)so + (off >> 3);
                        const uint64_t A = ob & ~3ull;
                        const uint32_t sh = (((uint32_t)ob & 3u) << 3) | ((uint32_t)off & 7u);
                        if (A + 20u <= a.buf_n) {
                            const bb_u4d l = __builtin_nontemporal_load(reinterpret_cast<const bb_u4d *>(a.buf + A));
                            uint32_t w[4] = {l.x, l.y, l.z, l.w};
                            if (sh) {
                                const uint32_t e = __builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(a.buf + A + 16u));
                                w[0] = (uint32_t)(((((uint64_t)l.y) << 32) | l.x) >> sh);
                                w[1] = (uint32_t)(((((uint64_t)l.z) << 32) | l.y) >> sh);
                                w[2] = (uint32_t)(((((uint64_t)l.w) << 32) | l.z) >> sh);
                                w[3] = (uint32_t)(((((uint64_t)e) << 32) | l.w) >> sh);
                            }
                            bb_requant_codes<LBI, LBO, NIN>(a, s_map, w, o);
                            done = true;
                        }
                    }
                }
                if (!done) {                                             // a frame boundary, the last bytes of the buffer
                    uint64_t r0, r1;
                    bb_requant_walk<LBI>(a, s_map, s, f, off, OUTB, r0, r1);
                    o[0] = (uint32_t)r0; o[1] = (uint32_t)(r0 >> 32); o[2] = (uint32_t)r1; o[3] = (uint32_t)(r1 >> 32);
                }
                if constexpr (LS <= 0)      { v[0] = o[0]; v[1] = o[1]; v[2] = o[2]; v[3] = o[3]; }
                else if constexpr (LS == 1) { v[2 * j] = o[0]; v[2 * j + 1] = o[1]; }
                else if constexpr (LS == 2) { v[j] = o[0]; }
                else                        { v[j >> 1] |= (o[0] & 0xffffu) << (16 * (j & 1)); }
            }
            bb_u4d t; t.x = v[0]; t.y = v[1]; t.z = v[2]; t.w = v[3];
            __builtin_nontemporal_store(t, reinterpret_cast<bb_u4d *>(dst + e0));
        } else {                                                         // the edge of the request
            const uint32_t lo = e0 > va ? e0 : va, hi = e0 + 16u < vb ? e0 + 16u : vb;
            uint64_t r0, r1;
            bb_requant_walk<LBI>(a, s_map, s, fu, offu + ((((uint64_t)(lo - va) << 3) >> LBO) << LBI), hi - lo, r0, r1);
#pragma unroll 1
            for (uint32_t b = 0; b < hi - lo; ++b)
                dst[lo + b] = (uint8_t)(b < 8u ? r0 >> (8u * b) : r1 >> (8u * (b - 8u)));
        }
    }
}

__global__ __launch_bounds__(BB_BLOCK, 4)
void k_requant(bb_requant_args a)
{
    __shared__ __attribute__((aligned(256))) uint32_t s_map32[64];
    const uint8_t *s_map = reinterpret_cast<const uint8_t *>(s_map32);
    if (a.lbi == 3u) {
        if (threadIdx.x < 64u) s_map32[threadIdx.x] = a.map[threadIdx.x];
        __syncthreads();
    }
    const uint32_t lane = (uint32_t)bb_lane();
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane(bb_wave());
    const uint64_t nwaves = (uint64_t)gridDim.x * BB_WAVES_PER_BLOCK;
    const uint64_t paybits = a.pay_in << 3;

    for (uint64_t w = (uint64_t)blockIdx.x * BB_WAVES_PER_BLOCK + wave; w < a.nwork; w += nwaves) {
        // the item: bytes [e_lo, e_hi) of output payload (F, s), of which [va, vb) belong to the request
        const uint64_t fs = a.nseg == 1 ? w : w / a.nseg;
        const uint64_t k = w - fs * a.nseg;
        const uint64_t Fr = fs / a.nslot;
        const uint32_t s = (uint32_t)(fs - Fr * a.nslot);
        const uint64_t F = a.F0 + Fr;
        const uint64_t Y0 = F * a.pay_out + k * a.seg;                   // the item's first byte in the slot's stream
        const uint64_t left = a.pay_out - k * a.seg;
        const uint64_t Y1 = Y0 + (left < a.seg ? left : a.seg);
        const uint64_t ya = Y0 > a.ya ? Y0 : a.ya, yb = Y1 < a.yb ? Y1 : a.yb;
        if (ya >= yb) continue;
        const uint32_t va = (uint32_t)(ya - Y0), vb = (uint32_t)(yb - Y0);
        // ... in the slot's input stream: byte ya begins with bit offu of frame fu
        const uint64_t xbit = a.xbit_a + ((((ya - a.ya) << 3) >> a.lbo) << a.lbi);
        const uint64_t fu = xbit / paybits;
        const uint64_t offu = xbit - fu * paybits;
        uint8_t *dst = a.out + (F * a.nslot + s) * a.pay_out + k * a.seg;
        switch ((a.lbi << 2) | a.lbo) {                                  // (wave-uniform: one kernel, sixteen loops)
#define BB_REQUANT_CASE(I, O) case ((I) << 2) | (O): bb_requant_item<I, O>(a, s_map, dst, s, va, vb, fu, offu, lane); break;
        BB_REQUANT_CASE(0, 0) BB_REQUANT_CASE(0, 1) BB_REQUANT_CASE(0, 2) BB_REQUANT_CASE(0, 3)
        BB_REQUANT_CASE(1, 0) BB_REQUANT_CASE(1, 1) BB_REQUANT_CASE(1, 2) BB_REQUANT_CASE(1, 3)
        BB_REQUANT_CASE(2, 0) BB_REQUANT_CASE(2, 1) BB_REQUANT_CASE(2, 2) BB_REQUANT_CASE(2, 3)
        BB_REQUANT_CASE(3, 0) BB_REQUANT_CASE(3, 1) BB_REQUANT_CASE(3, 2) BB_REQUANT_CASE(3, 3)
#undef BB_REQUANT_CASE
        default: break;
        }
    }
}
