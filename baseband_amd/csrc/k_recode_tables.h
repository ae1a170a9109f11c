// Conversion between sample widths across thread layouts on the packed bytes with ONE TABLE PER
// COMPONENT of a row (bb_recode_frames_tables): k_recode's contract with map[k][code] in place
// of map[code] -- a gain per (thread, channel) in front of the requantizer.  Component k of a
// row is field p = k % chunk_in (bps_in bits) of input slot s = k / chunk_in and becomes field
// q = k % chunk_out (bps_out bits) of output slot t = k / chunk_out, with value tables[k][code];
// where the input payload counts nothing it is fill_code, not mapped.  Equal thread structures
// on both sides are one of the geometries.
//
// Shape (gfx950): k_recode's two phases, a wave per work item of 4 or 8 KiB on its wider side.  The
// item loop, the staging and the store loop are WRITTEN OUT here, a copy of what k_repack.h
// (bb_repack_items, bb_stage_pieces) and k_recode.h (bb_recode_codes, bb_recode_store) hold for
// k_repack and k_recode: built on those, this kernel is slower on 4-bit input.
// A fix to that code must be made here too.  What differs from k_recode is the table:
//   * The ncomp << bps_in table bytes (at most 8 KiB: 32 components of 8 bits) arrive in device
//     memory -- an argument block cannot hold them -- and every workgroup copies them to LDS
//     once, before its item loop, dword by dword (ncomp << bps_in is a power of two; the two
//     bytes of one 1-bit component go byte by byte).  Every byte is masked to bps_out bits on
//     the way: the host cannot see the values, and a bad table must not set bits of a
//     neighbouring field.
//   * For every input width the tables then lie in LDS as [k][code], an 8-bit table on a
//     256-byte boundary; a code costs one LDS byte read at (k << bps_in) + code.  Within a group
//     of gc adjacent codes the components are k0, k0 + 1, ...: k0 is found where the group's
//     input dword is.
//   * In phase 2 the lanes of a wave stand 16 output bytes apart.  Where an output slot's row
//     divides 16 bytes (chunk_out * bps_out <= 128) all lanes are at the same component at a
//     given step and read one table: the 64 dwords of an 8-bit table lie two to a bank of the
//     byte read's 32, at most a 2-way conflict, as in k_recode.  Where the row is 32 bytes
//     (chunk_out * bps_out == 256) even and odd lanes are at components half a row apart and
//     read two tables: up to 4-way.
// LDS: with 8 KiB of tables beside k_recode's 38,080 + 1,152 B a workgroup has 47,424 B and three
// of them share a CU where k_recode has four.  So the LDS is sized per launch (dynamic: the tables
// rounded up to 256 B, then per wave the pieces and the validity bits of the launch's item size),
// and the host halves the item to 4 KiB on the wider side where the input is the wider side
// (measured: DESIGN.md 3.12): 8 components of 8 bits then take 23,872 B, six workgroups on a CU,
// 32 components 30,016 B, five; where the output is wider (tables of at most 1 KiB) the item stays
// 8 KiB, 39,488 B or less, four.  The grid is capped accordingly (tables_grid in bb_packed.inc).
// Nothing outside the buffer and the tables is read.
#pragma once
#include "bb_common.h"
#include "k_recode.h"

struct bb_recode_tables_args {
    const uint8_t *buf;
    const int64_t *src;          // payload offsets, NULL: src0 + (f * nslot_in + slot) * src_stride
    uint8_t *out;
    const uint8_t *tables;       // [ncomp][1 << bps_in], device memory, a dword boundary
    uint64_t buf_n;              // bytes of buf
    uint64_t src_lim;            // bb_src_ok
    int64_t  src0, src_stride;
    uint64_t pay_in, pay_out;    // bytes per frame-slot
    uint64_t row_lo;             // first row of the request
    uint64_t first_row;          // its output row
    uint64_t nrows;              // rows of the request
    uint64_t R_out;              // rows per output frame
    uint64_t F0;                 // first output frame with a written row
    uint64_t nseg;               // work items per output frame
    uint64_t nwork;
    uint32_t T;                  // rows per work item
    uint32_t nslot_in, nslot_out;
    uint32_t lbi, lbo;           // log2(chunk * bps) of a slot: bits per row, in and out
    uint32_t lpi, lpo;           // log2(bps), in and out
    uint32_t lgc;                // log2 of the codes read with one LDS access
    uint32_t sstride;            // LDS bytes per input slot: T << lbi >> 3 plus BB_REPACK_SLACK
    uint32_t fill;               // fill_code
    uint32_t tab_n;              // bytes of the tables: ncomp << bps_in
    uint32_t tab_lds;            // ... of their place in LDS: a multiple of 256
    uint32_t in_lds;             // LDS bytes of a wave's input pieces (bb_recode_tables_lds), a multiple of 16
    uint32_t ok_words;           // ... and words of their validity bits, a multiple of 4
};

// LDS of a wave whose items have `item_bits` bits on their wider side: the input pieces with one spare dword
// per 32 (bb_repack_sw), as BB_REPACK_LDS_WAVE for k_repack's items, and a validity bit per staged dword.
__host__ __device__ inline uint32_t bb_recode_tables_flat(uint32_t item_bits) { return item_bits / 8u + BB_RECODE_MAX_SLOTS * BB_REPACK_SLACK; }
__host__ __device__ inline uint32_t bb_recode_tables_lds(uint32_t item_bits) { const uint32_t f = bb_recode_tables_flat(item_bits); return f + f / 32u + 16u; }

// As bb_recode_codes, with the table of the code's own component: s_tab[k][code].
template <int LPI, int LPO, int NC>
__device__ __forceinline__ uint32_t bb_recode_tables_codes(const uint32_t *in, const uint32_t *ok, const uint8_t *s_tab,
                                                           uint32_t P, uint32_t t, const bb_recode_geo &g)
{
    constexpr uint32_t BI = 1u << LPI, BO = 1u << LPO, MI = (1u << BI) - 1u;
    const uint32_t gcm = (1u << g.lgc) - 1u;
    const uint32_t bim = (1u << g.lbi) - 1u, bom = (1u << g.lbo) - 1u, sdw = g.sstride >> 2;
    uint32_t out = 0, w = 0;
    const uint8_t *tab = s_tab;
    bool valid = false;
#pragma unroll
    for (uint32_t n = 0; n < (uint32_t)NC; ++n) {
        if ((n & gcm) == 0u) {                                           // (wave-uniform)
            const uint32_t Pn = P + n * BO;
            const uint32_t k = ((t << g.lbo) + (Pn & bom)) >> LPO;       // the component
            const uint32_t kb = k << LPI;                                // ... as a bit of the input row over all slots
            const uint32_t ibit = g.phase + ((Pn >> g.lbo) << g.lbi) + (kb & bim);
            const uint32_t d = (kb >> g.lbi) * sdw + (ibit >> 5);
            w = in[bb_repack_sw(d)] >> (ibit & 31u);
            valid = (ok[d >> 5] >> (d & 31u)) & 1u;
            tab = s_tab + (k << BI);
        }
        const uint32_t m = tab[w & MI];
        out |= (valid ? m : g.fill) << (n * BO);
        w >>= BI;
        tab += 1u << BI;                                                 // the next code of the group: the next component
    }
    return out;
}

// 2. of the kernel: LDS -> bytes [va, vb) of every output slot's piece at dst0 + t * pay_out.
template <int LPI, int LPO>
__device__ __forceinline__ void bb_recode_tables_out(const bb_recode_tables_args &a, const uint32_t *in, const uint32_t *ok,
                                                     const uint8_t *s_tab, uint8_t *dst0, uint32_t va, uint32_t vb,
                                                     uint32_t lane, const bb_recode_geo &g)
{
    constexpr int NCD = 32 >> LPO, NCB = 8 >> LPO;                       // codes of an output dword, of a byte
    const uint32_t q0 = va >> 4, q1 = (vb + 15u) >> 4;
    for (uint32_t t = 0; t < a.nslot_out; ++t) {
        uint8_t *dst = dst0 + t * a.pay_out;
        for (uint32_t q = q0 + lane; q < q1; q += BB_WAVE) {
            const uint32_t e0 = q << 4;
            if (e0 >= va && e0 + 16u <= vb) {
                // blocks of at most 8 codes, their LDS reads in flight together
                constexpr uint32_t NB = NCD < 8 ? NCD : 8, BB = NB << LPO;
                bb_u4p v;
                v.x = v.y = v.z = v.w = 0;
#pragma unroll 1
                for (uint32_t bit = 0; bit < 128u; bit += BB) {
                    const uint32_t x = bb_recode_tables_codes<LPI, LPO, NB>(in, ok, s_tab, (e0 << 3) + bit, t, g) << (bit & 31u);
                    const uint32_t i = bit >> 5;
                    v.x |= i == 0u ? x : 0u; v.y |= i == 1u ? x : 0u; v.z |= i == 2u ? x : 0u; v.w |= i == 3u ? x : 0u;
                }
                *reinterpret_cast<bb_u4p *>(dst + e0) = v;
            } else {                                                     // the edge of the request
                const uint32_t lo = e0 > va ? e0 : va, hi = e0 + 16u < vb ? e0 + 16u : vb;
#pragma unroll 1
                for (uint32_t e = lo; e < hi; ++e)
                    dst[e] = (uint8_t)bb_recode_tables_codes<LPI, LPO, NCB>(in, ok, s_tab, e << 3, t, g);
            }
        }
    }
}

// The work items of one wave, at one pair of widths (the arguments by value, as in k_recode).
template <int LPI, int LPO>
__device__ __forceinline__ void bb_recode_tables_items(const bb_recode_tables_args a, uint32_t *in, uint32_t *ok,
                                                       const uint8_t *s_tab, uint32_t wave, uint32_t lane)
{
    uint8_t *in8 = reinterpret_cast<uint8_t *>(in);
    const uint64_t nwaves = (uint64_t)gridDim.x * BB_WAVES_PER_BLOCK;

    for (uint64_t w = (uint64_t)blockIdx.x * BB_WAVES_PER_BLOCK + wave; w < a.nwork; w += nwaves) {
        // the item: rows [Gs, Gs + Ti) of output frame F, of which [ga, gb) belong to the request
        const uint64_t Fr = a.nseg == 1 ? w : w / a.nseg;
        const uint64_t k = w - Fr * a.nseg;
        const uint64_t F = a.F0 + Fr;
        const uint64_t Gs = F * a.R_out + k * a.T;
        const uint64_t left = a.R_out - k * a.T;
        const uint32_t Ti = left < a.T ? (uint32_t)left : a.T;
        const uint64_t ga = Gs > a.first_row ? Gs : a.first_row;
        const uint64_t gb = Gs + Ti < a.first_row + a.nrows ? Gs + Ti : a.first_row + a.nrows;
        if (ga >= gb) continue;
        // ... in every input slot's stream: bytes [ia, ib), kept in LDS from byte ibase on
        const uint64_t ra = a.row_lo + (ga - a.first_row), rb = a.row_lo + (gb - a.first_row);
        const uint64_t ia = (ra << a.lbi) >> 3, ib = ((rb << a.lbi) + 7u) >> 3;
        const uint64_t ibase = ia & ~15ull;
        bb_recode_geo g;
        g.lbi = a.lbi; g.lbo = a.lbo; g.sstride = a.sstride; g.lgc = a.lgc; g.fill = a.fill;
        // bit of grid row 0 relative to ibase: (ra - (ga - Gs)) * bits - ibase * 8, modulo 2^32
        g.phase = (uint32_t)((ra << a.lbi) - (ibase << 3)) - ((uint32_t)(ga - Gs) << a.lbi);

        for (uint32_t i = lane; i < a.ok_words; i += BB_WAVE) ok[i] = 0u;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();

        // 1. input pieces -> LDS, and which of their dwords had a source
        {
            const uint32_t pps = (uint32_t)((ib - ibase + 15u) >> 4);        // 16-byte pieces per slot
            const uint32_t total = pps * a.nslot_in;
            const uint64_t fu = ibase / a.pay_in;                            // (wave-uniform) frame of ibase
            const uint64_t offu = ibase - fu * a.pay_in;
            for (uint32_t j = lane; j < total; j += BB_WAVE) {
                const uint32_t s = j / pps, q = j - s * pps;
                const uint32_t loff = s * a.sstride + (q << 4);
                const uint64_t x0 = ibase + ((uint64_t)q << 4);
                uint64_t f = fu, off = offu + ((uint64_t)q << 4);
                if (off >= a.pay_in) { const uint64_t d = off / a.pay_in; f += d; off -= d * a.pay_in; }
                uint32_t okm = 0u;                                           // the piece's dwords that had a source
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
                            uint32_t *d = in + bb_repack_sw(loff >> 2);      // (a piece lies inside one run of 32 dwords)
                            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
                            okm = 15u;
                        } else {
                            fast = false;                                    // the last bytes of the buffer
                        }
                    }
                }
                if (!fast) {
                    const uint64_t lo = x0 > ia ? x0 : ia, hi = x0 + 16u < ib ? x0 + 16u : ib;
#pragma unroll 1
                    for (uint64_t x = lo; x < hi; ++x) {
                        const uint64_t fx = x / a.pay_in;
                        const int64_t so = bb_src_at(a, fx * a.nslot_in + s);
                        if (!bb_src_ok(so, a.src_lim)) continue;
                        in8[bb_repack_swb(loff + (uint32_t)(x - x0))] = a.buf[(uint64_t)so + (x - fx * a.pay_in)];
                        okm |= 1u << ((uint32_t)(x - x0) >> 2);
                    }
                }
                if (okm) {
                    const uint32_t dw = loff >> 2;                           // (a multiple of 4: the four bits lie in one word)
                    __hip_atomic_fetch_or(ok + (dw >> 5), okm << (dw & 31u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();

        // 2. LDS -> output pieces: bytes [va, vb) of the bytes the item's grid has per slot
        {
            const uint32_t va = (uint32_t)(((ga - Gs) << a.lbo) >> 3), vb = (uint32_t)(((gb - Gs) << a.lbo) >> 3);
            uint8_t *dst0 = a.out + F * a.nslot_out * a.pay_out + (((k * a.T) << a.lbo) >> 3);   // the grid's place in slot 0's payload
            bb_recode_tables_out<LPI, LPO>(a, in, ok, s_tab, dst0, va, vb, lane, g);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

extern __shared__ __attribute__((aligned(256))) uint32_t s_recode_tables[];   // the tables | per wave: input pieces, validity bits

__global__ __launch_bounds__(BB_BLOCK, 4)
void k_recode_tables(bb_recode_tables_args a)
{
    uint32_t *s_tab32 = s_recode_tables;
    uint8_t *s_tab = reinterpret_cast<uint8_t *>(s_tab32);
    {
        // the tables -> LDS, every byte masked to bps_out bits (tab_n: a power of two, at most 8 KiB)
        const uint32_t keep = ((1u << (1u << a.lpo)) - 1u) * 0x01010101u;
        if (a.tab_n >= 4u) {
            const uint32_t *t32 = reinterpret_cast<const uint32_t *>(a.tables);
            for (uint32_t i = threadIdx.x; i < (a.tab_n >> 2); i += BB_BLOCK) s_tab32[i] = t32[i] & keep;
        } else if (threadIdx.x < a.tab_n) {
            s_tab[threadIdx.x] = (uint8_t)(a.tables[threadIdx.x] & keep);
        }
        __syncthreads();
    }
    const uint32_t lane = (uint32_t)bb_lane();
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane(bb_wave());
    uint32_t *in = s_recode_tables + (a.tab_lds >> 2) + wave * ((a.in_lds >> 2) + a.ok_words);
    uint32_t *ok = in + (a.in_lds >> 2);
    switch ((a.lpi << 2) | a.lpo) {                                          // (wave-uniform: one kernel, sixteen loops)
#define BB_RECODE_TABLES_CASE(I, O) case ((I) << 2) | (O): bb_recode_tables_items<I, O>(a, in, ok, s_tab, wave, lane); break;
    BB_RECODE_TABLES_CASE(0, 0) BB_RECODE_TABLES_CASE(0, 1) BB_RECODE_TABLES_CASE(0, 2) BB_RECODE_TABLES_CASE(0, 3)
    BB_RECODE_TABLES_CASE(1, 0) BB_RECODE_TABLES_CASE(1, 1) BB_RECODE_TABLES_CASE(1, 2) BB_RECODE_TABLES_CASE(1, 3)
    BB_RECODE_TABLES_CASE(2, 0) BB_RECODE_TABLES_CASE(2, 1) BB_RECODE_TABLES_CASE(2, 2) BB_RECODE_TABLES_CASE(2, 3)
    BB_RECODE_TABLES_CASE(3, 0) BB_RECODE_TABLES_CASE(3, 1) BB_RECODE_TABLES_CASE(3, 2) BB_RECODE_TABLES_CASE(3, 3)
#undef BB_RECODE_TABLES_CASE
    default: break;
    }
}
