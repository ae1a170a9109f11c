// Format conversion on the packed bytes (bb_repack_frames): the decode of one format and
// the encode of another, applied back to back, without the floats in between
// (base/payload.py:314-330 with vdif/payload.py:25-114 and mark5b/payload.py:27-106).
// Samples of the same size have the same scale in VDIF and Mark 5B, so decode-then-encode
// is an exact map from code to code (identity, ~x for 1 bit, the two bits of a field
// swapped for 2 bits) and a conversion is a permutation of bit fields: component k of a
// row is field p = k % chunk_in of input slot s = k / chunk_in and field q = k % chunk_out
// of output slot t = k / chunk_out.  Fields are LSB first; a slot's payloads, frame after
// frame, are one bit stream in which row r begins at bit r * chunk * bps.
//
// Shape (gfx950): a work item is a run of T rows of one OUTPUT frame across all slots,
// 8 KiB of packed bytes, and belongs to one wave.
//   1. Every input slot's piece of the item goes to LDS as it lies in its stream: 16-byte
//      pieces on the stream's own 16-byte grid, one per lane, lanes dealt over (slot,
//      piece).  The source is read as one 16-byte load from the address aligned down to a
//      dword plus the dword behind it, and the payload's byte misalignment is shifted out
//      in registers.  The code map is ALU work on those dwords; a source that counts
//      nothing leaves the fill pattern.  Pieces that meet the edge of the request, a frame
//      boundary or the last bytes of the buffer are moved byte by byte.
//   2. Every output slot's piece is put together from LDS, four dwords per lane, and
//      leaves as one 16-byte store (the destination is a dword boundary: payloads are
//      multiples of 4).  A dword is 32 / g chunks of g = min(chunk_in, chunk_out) * bps
//      bits: chunks are what stays together.  LG = log2(g) is a template argument of the
//      store loop (5: whole dwords, which is also the case of equal slot structures), so
//      the loop is unrolled and for rows of at most 32 bits everything but the row is
//      wave-uniform; the kernel picks the loop once per item (ONE kernel in the code object).
//      Groups at the edge of the request are stored byte by byte: bytes outside the rows
//      of the request are never written.
// Nothing outside the buffer is read.
// The item loop (bb_repack_items) and phase 1 (bb_stage_pieces<Stage>) are written here for this
// kernel and k_recode: what a kernel does to a piece on its way in is its Stage type.
// k_recode_tables does NOT use them: k_recode_tables.h holds its own copy of the item geometry and
// of the staging, so a fix to either must be made there as well.
#pragma once
#include "bb_common.h"

#define BB_REPACK_ITEM_BITS 65536u                           // packed bits of a work item over all slots (8 KiB)
#define BB_REPACK_MAX_SLOTS 32u
#define BB_REPACK_MAX_ROW_BITS 256u
#define BB_REPACK_SLACK 32u                                  // LDS bytes per slot beyond its piece: 16-byte grid + a partial byte
#define BB_REPACK_LDS_FLAT (BB_REPACK_ITEM_BITS / 8u + BB_REPACK_MAX_SLOTS * BB_REPACK_SLACK)    // bytes of a wave's input pieces
#define BB_REPACK_LDS_WAVE (BB_REPACK_LDS_FLAT + BB_REPACK_LDS_FLAT / 32u + 16u)                // ... with one spare dword per 32 (bb_repack_sw)

struct bb_repack_args {
    const uint8_t *buf;
    const int64_t *src;          // payload offsets, NULL: src0 + (f * nslot_in + slot) * src_stride
    uint8_t *out;
    uint64_t buf_n;              // bytes of buf
    uint64_t src_lim;            // bb_src_ok
    int64_t  src0, src_stride;
    uint64_t pay_in, pay_out;    // bytes per frame-slot
    uint64_t row_lo;             // first counted row of the request
    uint64_t first_row;          // its output row
    uint64_t nrows;              // counted rows
    uint64_t R_out;              // rows per output frame
    uint64_t F0;                 // first output frame with a written row
    uint64_t nseg;               // work items per output frame
    uint64_t nwork;
    uint32_t T;                  // rows per work item
    uint32_t nslot_in, nslot_out;
    uint32_t lbi, lbo;           // log2(chunk * bps) of a slot: bits per row, in and out
    uint32_t sstride;            // LDS bytes per input slot: T << lbi >> 3 plus BB_REPACK_SLACK
    uint32_t lg;                 // log2 of the bits that stay together, 5: whole dwords (bb_repack_dword)
    uint32_t map;                // 0: identity, 1: invert every bit, 2: swap the two bits of every 2-bit field
    uint32_t fillw;              // fill_code in every field of a dword
};

struct __attribute__((packed, aligned(4))) bb_u4p { uint32_t x, y, z, w; };   // 16 bytes on a dword boundary

__device__ __forceinline__ uint32_t bb_repack_map(uint32_t x, uint32_t map)
{
    return map == 0 ? x : map == 1 ? ~x : ((x & 0x55555555u) << 1) | ((x >> 1) & 0x55555555u);
}

// Where dword dw (byte b) of a wave's input pieces lies in LDS: one spare dword after every 32.
// In a thread split a lane's 16 output bytes draw from 16 * chunk_in / chunk_out input bytes, so
// the lanes of a wave read at strides of 8 .. 128 dwords: without the spare dwords 8 to 32 lanes
// met on one bank (the split row of tools/bench_convert.py took 7.2 ms that way).
__device__ __forceinline__ uint32_t bb_repack_sw(uint32_t dw) { return dw + (dw >> 5); }
__device__ __forceinline__ uint32_t bb_repack_swb(uint32_t b) { return (bb_repack_sw(b >> 2) << 2) | (b & 3u); }

// bytes sh.. of the dword pair (lo, hi)
__device__ __forceinline__ uint32_t bb_repack_shift(uint32_t lo, uint32_t hi, uint32_t sh)
{
    return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (8u * sh));
}

// ---- what k_repack and k_recode share: the item and phase 1.  Their arguments (bb_repack_args,
//      bb_recode_args) name the members used here alike.  (k_recode_tables.h has its own copy.) ----

// Work item w: rows [Gs, Gs + Ti) of output frame F, of which [ga, gb) belong to the request.
struct bb_repack_item {
    uint64_t F, k, Gs, ga, gb;
    uint64_t ia, ib, ibase;      // ... in every input slot's stream: bytes [ia, ib), kept in LDS from byte ibase on
    uint32_t phase;              // bit of grid row 0 relative to ibase (may be negative for rows in front of the request: wraps)
    uint32_t va, vb;             // ... of the bytes the item's grid has per output slot: bytes [va, vb)
    uint8_t *dst0;               // the grid's place in slot 0's payload
};

// The item loop of a wave: body(it) for every item of which a row belongs to the request.  (The loop and
// not a function of w that says "skip": inlined, that carries the item's members around the loop, the
// compiler forgets their ranges and the kernels' code gets slower)
template <class Args, class Body>
__device__ __forceinline__ void bb_repack_items(const Args &a, uint32_t wave, Body body)
{
    const uint64_t nwaves = (uint64_t)gridDim.x * BB_WAVES_PER_BLOCK;
    for (uint64_t w = (uint64_t)blockIdx.x * BB_WAVES_PER_BLOCK + wave; w < a.nwork; w += nwaves) {
        const uint64_t Fr = a.nseg == 1 ? w : w / a.nseg;
        const uint64_t k = w - Fr * a.nseg;
        const uint64_t F = a.F0 + Fr;
        const uint64_t Gs = F * a.R_out + k * a.T;
        const uint64_t left = a.R_out - k * a.T;
        const uint32_t Ti = left < a.T ? (uint32_t)left : a.T;
        const uint64_t ga = Gs > a.first_row ? Gs : a.first_row;
        const uint64_t gb = Gs + Ti < a.first_row + a.nrows ? Gs + Ti : a.first_row + a.nrows;
        if (ga >= gb) continue;
        const uint64_t ra = a.row_lo + (ga - a.first_row), rb = a.row_lo + (gb - a.first_row);
        const uint64_t ia = (ra << a.lbi) >> 3, ib = ((rb << a.lbi) + 7u) >> 3;
        const uint64_t ibase = ia & ~15ull;
        bb_repack_item it;
        it.F = F; it.k = k; it.Gs = Gs; it.ga = ga; it.gb = gb; it.ia = ia; it.ib = ib; it.ibase = ibase;
        // (ra - (ga - Gs)) * bits - ibase * 8, modulo 2^32
        it.phase = (uint32_t)((ra << a.lbi) - (ibase << 3)) - ((uint32_t)(ga - Gs) << a.lbi);
        it.va = (uint32_t)(((ga - Gs) << a.lbo) >> 3); it.vb = (uint32_t)(((gb - Gs) << a.lbo) >> 3);
        it.dst0 = a.out + F * a.nslot_out * a.pay_out + (((k * a.T) << a.lbo) >> 3);
        body(it);
    }
}

// 1. of the three kernels: input pieces -> LDS.  Every input slot's piece of the item goes to `in`
// as it lies in its stream, 16-byte pieces on the stream's own 16-byte grid, one per lane, lanes
// dealt over (slot, piece); pieces that meet the edge of the request, a frame boundary or the
// last bytes of the buffer go byte by byte.  `Stage` is what differs between the kernels:
//   code(x)        what a dword (a byte: its low 8 bits) of the source becomes on its way in;
//   absent(x)      no source: -> true with x the dword (low 8 bits: the byte) to leave, or false: leave nothing;
//   done(loff, m)  after the piece at LDS byte loff, m: a bit per dword of it that had a source.
template <class Stage, class Args>
__device__ __forceinline__ void bb_stage_pieces(const Args &a, const bb_repack_item &it, uint32_t *in, uint32_t lane, const Stage st)
{
    uint8_t *in8 = reinterpret_cast<uint8_t *>(in);
    const uint64_t ia = it.ia, ib = it.ib, ibase = it.ibase;
    const uint32_t pps = (uint32_t)((ib - ibase + 15u) >> 4);                // 16-byte pieces per slot
    const uint32_t total = pps * a.nslot_in;
    const uint64_t fu = ibase / a.pay_in;                                    // (wave-uniform) frame of ibase
    const uint64_t offu = ibase - fu * a.pay_in;
    for (uint32_t j = lane; j < total; j += BB_WAVE) {
        const uint32_t s = j / pps, q = j - s * pps;
        const uint32_t loff = s * a.sstride + (q << 4);
        const uint64_t x0 = ibase + ((uint64_t)q << 4);
        uint64_t f = fu, off = offu + ((uint64_t)q << 4);
        if (off >= a.pay_in) { const uint64_t d = off / a.pay_in; f += d; off -= d * a.pay_in; }
        uint32_t okm = 0u;                                                   // the piece's dwords that had a source
        bool fast = x0 >= ia && x0 + 16u <= ib && off + 16u <= a.pay_in;
        if (fast) {
            const int64_t so = bb_src_at(a, f * a.nslot_in + s);
            if (bb_src_ok(so, a.src_lim)) {
                const uint64_t o = (uint64_t)so + off;
                const uint64_t A = o & ~3ull;
                const uint32_t sh = (uint32_t)o & 3u;
                if (A + (sh ? 20u : 16u) <= a.buf_n) {
                    const bb_u4p l = *reinterpret_cast<const bb_u4p *>(a.buf + A);
                    bb_u4 v = bb_u4{l.x, l.y, l.z, l.w};
                    if (sh) {
                        const uint32_t e = *reinterpret_cast<const uint32_t *>(a.buf + A + 16u);
                        v = bb_u4{bb_repack_shift(l.x, l.y, sh), bb_repack_shift(l.y, l.z, sh),
                                  bb_repack_shift(l.z, l.w, sh), bb_repack_shift(l.w, e, sh)};
                    }
                    uint32_t *d = in + bb_repack_sw(loff >> 2);              // (a piece lies inside one run of 32 dwords)
                    d[0] = st.code(v.x); d[1] = st.code(v.y); d[2] = st.code(v.z); d[3] = st.code(v.w);
                    okm = 15u;
                } else {
                    fast = false;                                            // the last bytes of the buffer
                }
            } else {
                uint32_t x;
                uint32_t *d = in + bb_repack_sw(loff >> 2);
                if (st.absent(x)) { d[0] = x; d[1] = x; d[2] = x; d[3] = x; }
            }
        }
        if (!fast) {
            const uint64_t lo = x0 > ia ? x0 : ia, hi = x0 + 16u < ib ? x0 + 16u : ib;
#pragma unroll 1
            for (uint64_t x = lo; x < hi; ++x) {
                const uint64_t fx = x / a.pay_in;
                const int64_t so = bb_src_at(a, fx * a.nslot_in + s);
                uint32_t b;
                if (bb_src_ok(so, a.src_lim)) {
                    b = st.code(a.buf[(uint64_t)so + (x - fx * a.pay_in)]);
                    okm |= 1u << ((uint32_t)(x - x0) >> 2);
                } else if (!st.absent(b)) {
                    continue;
                }
                in8[bb_repack_swb(loff + (uint32_t)(x - x0))] = (uint8_t)b;
            }
        }
        st.done(loff, okm);
    }
}

// k_repack's: the code map is ALU work on the dwords; a source that counts nothing leaves the fill pattern.
struct bb_repack_stage {
    uint32_t map, fillw;
    __device__ __forceinline__ uint32_t code(uint32_t x) const { return bb_repack_map(x, map); }
    __device__ __forceinline__ bool absent(uint32_t &x) const { x = fillw; return true; }
    __device__ __forceinline__ void done(uint32_t, uint32_t) const {}
};

// What the store loop needs of the item and the arguments.
struct bb_repack_geo {
    uint32_t phase, lbi, lbo, sstride;
};

// Dword m of output slot t's piece.
template <int LG>
__device__ __forceinline__ uint32_t bb_repack_dword(const uint32_t *in, uint32_t m, uint32_t t, const bb_repack_geo &g)
{
    constexpr uint32_t GB = 1u << LG, NCH = 32u / GB, GM = LG >= 5 ? 0xffffffffu : (1u << (GB & 31u)) - 1u;
    const uint32_t bim = (1u << g.lbi) - 1u, bom = (1u << g.lbo) - 1u, sdw = g.sstride >> 2;
    uint32_t out = 0;
    if constexpr (LG >= 5) {
        // whole dwords; equal slot structures are a byte stream, which may sit at any byte of its dword
        const uint32_t P = m << 5;
        const uint32_t c = (t << g.lbo) + (P & bom);
        const uint32_t ibit = g.phase + ((P >> g.lbo) << g.lbi) + (c & bim);
        const uint32_t d = (c >> g.lbi) * sdw + (ibit >> 5);
        const uint32_t sh = ibit & 31u;
        out = in[bb_repack_sw(d)];
        if (sh) out = (uint32_t)(((((uint64_t)in[bb_repack_sw(d + 1u)]) << 32) | out) >> sh);
    } else if (g.lbo <= 5u) {
        // rows of at most a dword: slot and place in the row of chunk i are the same for every m
        const uint32_t ib0 = g.phase + ((m << (5u - g.lbo)) << g.lbi);
#pragma unroll
        for (uint32_t i = 0; i < NCH; ++i) {
            const uint32_t pb = i * GB;
            const uint32_t c = (t << g.lbo) + (pb & bom);
            const uint32_t ibit = ib0 + (((pb >> g.lbo) << g.lbi) + (c & bim));
            const uint32_t w = in[bb_repack_sw((c >> g.lbi) * sdw + (ibit >> 5))];
            out |= ((w >> (ibit & 31u)) & GM) << pb;
        }
    } else {
        const uint32_t ib0 = g.phase + ((m >> (g.lbo - 5u)) << g.lbi);
        const uint32_t c0 = (t << g.lbo) + ((m & ((1u << (g.lbo - 5u)) - 1u)) << 5);
#pragma unroll
        for (uint32_t i = 0; i < NCH; ++i) {
            const uint32_t pb = i * GB;
            const uint32_t c = c0 + pb;
            const uint32_t ibit = ib0 + (c & bim);
            const uint32_t w = in[bb_repack_sw((c >> g.lbi) * sdw + (ibit >> 5))];
            out |= ((w >> (ibit & 31u)) & GM) << pb;
        }
    }
    return out;
}

// Byte e of output slot t's piece, whatever the chunk (the edges of a request).
__device__ __forceinline__ uint32_t bb_repack_out_byte(const uint8_t *in, uint32_t e, uint32_t t, const bb_repack_geo &g)
{
    const uint32_t lg = g.lbi < g.lbo ? g.lbi : g.lbo;
    const uint32_t gb = lg >= 3u ? 8u : 1u << lg;
    const uint32_t bim = (1u << g.lbi) - 1u, bom = (1u << g.lbo) - 1u;
    uint32_t out = 0;
    for (uint32_t pb = 0; pb < 8u; pb += gb) {
        const uint32_t P = (e << 3) + pb;
        const uint32_t c = (t << g.lbo) + (P & bom);
        const uint32_t ibit = g.phase + ((P >> g.lbo) << g.lbi) + (c & bim);
        const uint32_t v = in[bb_repack_swb((c >> g.lbi) * g.sstride + (ibit >> 3))];
        out |= ((v >> (ibit & 7u)) & ((1u << gb) - 1u)) << pb;
    }
    return out;
}

// 2. of the kernel: LDS -> bytes [va, vb) of every output slot's piece at dst0 + t * tstride.
template <int LG>
__device__ __forceinline__ void bb_repack_store(const uint32_t *in, uint8_t *dst0, uint64_t tstride, uint32_t nslot_out,
                                                uint32_t va, uint32_t vb, uint32_t lane, const bb_repack_geo &g)
{
    const uint8_t *in8 = reinterpret_cast<const uint8_t *>(in);
    const uint32_t q0 = va >> 4, q1 = (vb + 15u) >> 4;
    for (uint32_t t = 0; t < nslot_out; ++t) {
        uint8_t *dst = dst0 + t * tstride;
        for (uint32_t q = q0 + lane; q < q1; q += BB_WAVE) {
            const uint32_t e0 = q << 4;
            if (e0 >= va && e0 + 16u <= vb) {
                bb_u4p v;
                v.x = bb_repack_dword<LG>(in, 4u * q, t, g);
                v.y = bb_repack_dword<LG>(in, 4u * q + 1u, t, g);
                v.z = bb_repack_dword<LG>(in, 4u * q + 2u, t, g);
                v.w = bb_repack_dword<LG>(in, 4u * q + 3u, t, g);
                *reinterpret_cast<bb_u4p *>(dst + e0) = v;
            } else {
                const uint32_t lo = e0 > va ? e0 : va, hi = e0 + 16u < vb ? e0 + 16u : vb;
#pragma unroll 1
                for (uint32_t e = lo; e < hi; ++e) dst[e] = (uint8_t)bb_repack_out_byte(in8, e, t, g);
            }
        }
    }
}

__global__ __launch_bounds__(BB_BLOCK, 4)
void k_repack(bb_repack_args a)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_in[BB_WAVES_PER_BLOCK * (BB_REPACK_LDS_WAVE / 4u)];
    const uint32_t lane = (uint32_t)bb_lane();
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane(bb_wave());
    uint32_t *in = s_in + wave * (BB_REPACK_LDS_WAVE / 4u);
    bb_repack_items(a, wave, [&](const bb_repack_item &it) __attribute__((always_inline)) {
        const bb_repack_geo g{it.phase, a.lbi, a.lbo, a.sstride};

        // 1. input pieces -> LDS
        bb_stage_pieces(a, it, in, lane, bb_repack_stage{a.map, a.fillw});
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();

        // 2. LDS -> output pieces
        switch (a.lg) {                                                      // (wave-uniform: one kernel, six loops)
        case 0:  bb_repack_store<0>(in, it.dst0, a.pay_out, a.nslot_out, it.va, it.vb, lane, g); break;
        case 1:  bb_repack_store<1>(in, it.dst0, a.pay_out, a.nslot_out, it.va, it.vb, lane, g); break;
        case 2:  bb_repack_store<2>(in, it.dst0, a.pay_out, a.nslot_out, it.va, it.vb, lane, g); break;
        case 3:  bb_repack_store<3>(in, it.dst0, a.pay_out, a.nslot_out, it.va, it.vb, lane, g); break;
        case 4:  bb_repack_store<4>(in, it.dst0, a.pay_out, a.nslot_out, it.va, it.vb, lane, g); break;
        default: bb_repack_store<5>(in, it.dst0, a.pay_out, a.nslot_out, it.va, it.vb, lane, g); break;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    });
}
