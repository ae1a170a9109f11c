// Conversion between sample widths ACROSS thread layouts on the packed bytes (bb_recode_frames):
// k_repack's permutation of components with k_requant's table in place of the three-way code
// map, in one pass -- N bytes in, N * bps_out / bps_in out, no temporary between two launches.
// Component k of a row is field p = k % chunk_in (bps_in bits) of input slot s = k / chunk_in
// and becomes field q = k % chunk_out (bps_out bits) of output slot t = k / chunk_out, with
// value map[code]; where the input payload counts nothing it is fill_code, not mapped.  Fields
// are LSB first; a slot's payloads, frame after frame, are one bit stream in which row r begins
// at bit r * chunk * bps.
//
// Shape (gfx950), k_repack's two phases: a work item (k_repack's: bb_repack_items) is a run of T
// rows of one OUTPUT frame across all slots, 8 KiB on its wider side, and belongs to one wave.
//   1. The shared staging (bb_stage_pieces in k_repack.h, with bb_recode_stage).
//      Every input slot's piece of the item goes to LDS as it lies in its stream, UNMAPPED:
//      16-byte pieces on the stream's own 16-byte grid, one per lane, read as one 16-byte load
//      from the address aligned down to a dword plus the dword behind it, the misalignment
//      shifted out in registers; one spare dword per 32 (bb_repack_sw).  Pieces that meet the
//      edge of the request, a frame boundary or the last bytes of the buffer go byte by byte.
//      Whether a staged dword had a source is ONE BIT per dword beside the pieces (payloads are
//      whole dwords, so a dword never mixes frames): fill_code is a code of the output and has
//      no place among the unmapped input codes.  A lane sets the four bits of its piece with
//      one LDS atomic OR; the bits are cleared per item.
//   2. Every lane makes 16 output bytes: the codes are gathered from LDS and mapped one by one.
//      The gc = min(chunk_in, chunk_out) codes that stay adjacent on both sides (at most a
//      dword of either) are read with one LDS access.  The bytes leave as one 16-byte store
//      (payloads are whole dwords); groups at the edge of the request leave byte by byte:
//      bytes outside the rows of the request are never written.
// Tables of bps_in <= 4 are a shift and a mask on kernel arguments; the 256 entries of
// bps_in == 8 lie in LDS on a 256-byte boundary, one dword per bank, as in k_requant.  Widths
// and geometry are wave-uniform run-time values: the kernel picks one of 16 loops per launch
// (ONE kernel in the code object).  Nothing outside the buffer is read.
#pragma once
#include "bb_common.h"
#include "k_repack.h"

#define BB_RECODE_ITEM_BITS BB_REPACK_ITEM_BITS              // bits of a work item over all slots, on its wider side (8 KiB)
#define BB_RECODE_MAX_SLOTS 32u
#define BB_RECODE_MAX_ROW_BITS 256u
#define BB_RECODE_OK_WORDS (BB_REPACK_LDS_FLAT / 4u / 32u)   // a bit per staged dword: 72 words a wave

struct bb_recode_args {
    const uint8_t *buf;
    const int64_t *src;          // payload offsets, NULL: src0 + (f * nslot_in + slot) * src_stride
    uint8_t *out;
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
    uint32_t map[64];            // uint8 map[256]
};

struct bb_recode_geo {
    uint32_t phase, lbi, lbo, sstride, lgc, fill;
};

// bb_stage_pieces for k_recode: the pieces stay as they are, a piece or byte without a source
// leaves nothing, and a lane sets the validity bits of its piece with one LDS atomic OR.
struct bb_recode_stage {
    uint32_t *ok;
    __device__ __forceinline__ uint32_t code(uint32_t x) const { return x; }
    __device__ __forceinline__ bool absent(uint32_t &) const { return false; }
    __device__ __forceinline__ void done(uint32_t loff, uint32_t okm) const
    {
        if (okm) {
            const uint32_t dw = loff >> 2;                               // (a multiple of 4: the four bits lie in one word)
            __hip_atomic_fetch_or(ok + (dw >> 5), okm << (dw & 31u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        }
    }
};

// The NC output codes from bit P on of output slot t's piece (P counts from row 0 of the item's
// grid; NC codes never pass the end of a dword), mapped, from bit 0 of the result on.  A new
// LDS dword is read where a group of 1 << lgc codes begins and at the first code.
template <int LPI, int LPO, int NC>
__device__ __forceinline__ uint32_t bb_recode_codes(const bb_recode_args &a, const uint32_t *in, const uint32_t *ok,
                                                    const uint8_t *s_map, uint32_t P, uint32_t t, const bb_recode_geo &g)
{
    constexpr uint32_t BI = 1u << LPI, BO = 1u << LPO, MI = (1u << BI) - 1u;
    const uint32_t gcm = (1u << g.lgc) - 1u;
    const uint32_t bim = (1u << g.lbi) - 1u, bom = (1u << g.lbo) - 1u, sdw = g.sstride >> 2;
    uint32_t out = 0, w = 0;
    bool valid = false;
#pragma unroll
    for (uint32_t n = 0; n < (uint32_t)NC; ++n) {
        if ((n & gcm) == 0u) {                                           // (wave-uniform)
            const uint32_t Pn = P + n * BO;
            const uint32_t kb = (((t << g.lbo) + (Pn & bom)) >> LPO) << LPI;   // the component, as a bit of the input row over all slots
            const uint32_t ibit = g.phase + ((Pn >> g.lbo) << g.lbi) + (kb & bim);
            const uint32_t d = (kb >> g.lbi) * sdw + (ibit >> 5);
            w = in[bb_repack_sw(d)] >> (ibit & 31u);
            valid = (ok[d >> 5] >> (d & 31u)) & 1u;
        }
        const uint32_t m = bb_requant_map<LPI>(a, s_map, w & MI);
        out |= (valid ? m : g.fill) << (n * BO);
        w >>= BI;
    }
    return out;
}

// 2. of the kernel: LDS -> bytes [va, vb) of every output slot's piece at dst0 + t * pay_out.
template <int LPI, int LPO>
__device__ __forceinline__ void bb_recode_store(const bb_recode_args &a, const uint32_t *in, const uint32_t *ok, const uint8_t *s_map,
                                                uint8_t *dst0, uint32_t va, uint32_t vb, uint32_t lane, const bb_recode_geo &g)
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
                    const uint32_t x = bb_recode_codes<LPI, LPO, NB>(a, in, ok, s_map, (e0 << 3) + bit, t, g) << (bit & 31u);
                    const uint32_t i = bit >> 5;
                    v.x |= i == 0u ? x : 0u; v.y |= i == 1u ? x : 0u; v.z |= i == 2u ? x : 0u; v.w |= i == 3u ? x : 0u;
                }
                *reinterpret_cast<bb_u4p *>(dst + e0) = v;
            } else {                                                     // the edge of the request
                const uint32_t lo = e0 > va ? e0 : va, hi = e0 + 16u < vb ? e0 + 16u : vb;
#pragma unroll 1
                for (uint32_t e = lo; e < hi; ++e)
                    dst[e] = (uint8_t)bb_recode_codes<LPI, LPO, NCB>(a, in, ok, s_map, e << 3, t, g);
            }
        }
    }
}

// The work items of one wave, at one pair of widths.  (The arguments by value: a copy per pair of
// widths, which the compiler takes apart into registers; one block that all sixteen loops read has
// more uses than it takes apart, and stays in scratch.)
template <int LPI, int LPO>
__device__ __forceinline__ void bb_recode_items(const bb_recode_args a, uint32_t *in, uint32_t *ok, const uint8_t *s_map,
                                                uint32_t wave, uint32_t lane)
{
    bb_repack_items(a, wave, [&](const bb_repack_item &it) __attribute__((always_inline)) {
        const bb_recode_geo g{it.phase, a.lbi, a.lbo, a.sstride, a.lgc, a.fill};

        for (uint32_t i = lane; i < BB_RECODE_OK_WORDS; i += BB_WAVE) ok[i] = 0u;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();

        // 1. input pieces -> LDS, and which of their dwords had a source
        bb_stage_pieces(a, it, in, lane, bb_recode_stage{ok});
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();

        // 2. LDS -> output pieces
        bb_recode_store<LPI, LPO>(a, in, ok, s_map, it.dst0, it.va, it.vb, lane, g);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    });
}

__global__ __launch_bounds__(BB_BLOCK, 4)
void k_recode(bb_recode_args a)
{
    __shared__ __attribute__((aligned(256))) uint32_t s_map32[64];
    __shared__ __attribute__((aligned(16))) uint32_t s_in[BB_WAVES_PER_BLOCK * (BB_REPACK_LDS_WAVE / 4u)];
    __shared__ uint32_t s_ok[BB_WAVES_PER_BLOCK * BB_RECODE_OK_WORDS];
    const uint8_t *s_map = reinterpret_cast<const uint8_t *>(s_map32);
    if (a.lpi == 3u) {
        if (threadIdx.x < 64u) s_map32[threadIdx.x] = a.map[threadIdx.x];
        __syncthreads();
    }
    const uint32_t lane = (uint32_t)bb_lane();
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane(bb_wave());
    uint32_t *in = s_in + wave * (BB_REPACK_LDS_WAVE / 4u);
    uint32_t *ok = s_ok + wave * BB_RECODE_OK_WORDS;
    switch ((a.lpi << 2) | a.lpo) {                                          // (wave-uniform: one kernel, sixteen loops)
#define BB_RECODE_CASE(I, O) case ((I) << 2) | (O): bb_recode_items<I, O>(a, in, ok, s_map, wave, lane); break;
    BB_RECODE_CASE(0, 0) BB_RECODE_CASE(0, 1) BB_RECODE_CASE(0, 2) BB_RECODE_CASE(0, 3)
    BB_RECODE_CASE(1, 0) BB_RECODE_CASE(1, 1) BB_RECODE_CASE(1, 2) BB_RECODE_CASE(1, 3)
    BB_RECODE_CASE(2, 0) BB_RECODE_CASE(2, 1) BB_RECODE_CASE(2, 2) BB_RECODE_CASE(2, 3)
    BB_RECODE_CASE(3, 0) BB_RECODE_CASE(3, 1) BB_RECODE_CASE(3, 2) BB_RECODE_CASE(3, 3)
#undef BB_RECODE_CASE
    default: break;
    }
}
