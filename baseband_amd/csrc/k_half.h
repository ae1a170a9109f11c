// Decode to 16-BIT output elements (bb_decode_params.out_type = BB_OUT_F16 /
// BB_OUT_BF16): packed 1/2/4/8-bit codes -> float16 or bfloat16, whole frames.
// Same reference lines as k_flat.h (vdif/payload.py:69-103, mark5b/payload.py:
// 78-94, base/encoding.py:131-144, base/payload.py:314-330, vdif/frame.py:402-434,
// base/frame.py:191-199), the result being the float32 value rounded once to
// nearest even.
//
// The kernels do NOT know which of the two types they write: every sample value
// is a table entry, the host converts the level tables and the fill value once
// (bb_half_host.h) and hands the kernel 2^bps 16-bit patterns; the kernel builds
// its byte table from them in LDS and moves patterns.  One family, eight
// instantiations (the product code object is capped below 150 kernels).
//
// k_decode_half_flat<BPS>: contiguous output (nslot == 1), modelled on
// k_decode_flat_lds (k_lds.h): a wave stages up to 8 tiles of 256 payload bytes
// with direct-to-LDS 16-byte loads (global_load_lds_dwordx4), then every store
// pass writes 1 KiB contiguous: lane l stores the 8 elements (16 bytes)
// 512 p + 8 l .. + 8 of the wave's range, which are the codes of
//     1-bit: byte  64 p + l         one 16-byte table row
//     2-bit: bytes 128 p + 2 l, +1  two 8-byte rows (as 4-bit float32 does with s_lut2)
//     4-bit: bytes 256 p + 4 l ..   one staged dword, four 4-byte rows
//     8-bit: bytes 512 p + 8 l ..   two staged dwords, eight 2-byte entries
// Work dealing (bb_perm), bounds rule (bb_src_ok), edge pieces loaded dword by
// dword and the byte-wise staging of payloads at odd addresses are those of
// k_decode_flat_lds.  Non-temporal stores always.
//
// k_decode_half_rows<BPS>: thread interleave (nslot > 1), one general kernel:
// a workgroup stages `seg_bytes` of every thread slot's payload of one frame
// set in LDS and writes the rows they hold in OUTPUT order, 16 bytes per lane
// whatever the chunk (a lane's 8 elements come from 8 / chunk thread slots when
// the chunk is narrower than 8).
#pragma once
#include "bb_common.h"

typedef uint32_t bb_u2 __attribute__((ext_vector_type(2)));

struct bb_half_args {
    const uint8_t  *buf;
    const int64_t  *src;    // [nfs] payload offsets, -1 = fill; may be null
    uint16_t       *out;
    const uint16_t *tab;    // 2^bps level patterns in the output type
    uint64_t nfs;           // nframes * nslot
    uint64_t ndw;           // payload dwords per frame-slot
    uint64_t nseg;          // work items per frame-slot (flat) / frame set (rows)
    uint32_t seg_tiles;     // flat: tiles per work item
    uint32_t tpw;           // flat: tiles per wave within a work item (<= 8)
    uint32_t seg_bytes;     // rows: payload bytes of every slot per work item (power of two >= 8)
    uint32_t nslot, chunk, lchunk;
    uint32_t fill;          // fill pattern of an (even, odd) element pair: re | im << 16
    int64_t  src0, src_stride;
    uint64_t src_lim;       // bb_src_ok
    bb_perm_t perm;
};

// byte -> the 8 / BPS elements it holds, low field first
template <int BPS>
__device__ __forceinline__ void bb_half_byte_table(uint16_t *s_tab, const uint16_t *tab, int nthreads)
{
    constexpr int EPB = 8 / BPS;
    constexpr uint32_t CMASK = (1u << BPS) - 1;
    for (int i = threadIdx.x; i < 256 * EPB; i += nthreads) {
        const uint32_t b = (uint32_t)i / EPB, k = (uint32_t)i % EPB;
        s_tab[i] = tab[(b >> (k * BPS)) & CMASK];
    }
}

// the 8 elements whose codes start at byte `b` of a staged image (b a multiple of BPS;
// for 8-bit samples `both` = the second dword is wanted too)
template <int BPS>
__device__ __forceinline__ bb_u4 bb_half_expand(const uint16_t *s_tab, const uint8_t *stage, uint32_t b, bool both = true)
{
    if (BPS == 1) {
        return reinterpret_cast<const bb_u4 *>(s_tab)[stage[b]];
    } else if (BPS == 2) {
        const uint32_t h = *reinterpret_cast<const uint16_t *>(stage + b);
        const bb_u2 lo = reinterpret_cast<const bb_u2 *>(s_tab)[h & 0xff];
        const bb_u2 hi = reinterpret_cast<const bb_u2 *>(s_tab)[h >> 8];
        return bb_u4{lo.x, lo.y, hi.x, hi.y};
    } else if (BPS == 4) {
        const uint32_t w = *reinterpret_cast<const uint32_t *>(stage + b);
        const uint32_t *t = reinterpret_cast<const uint32_t *>(s_tab);
        return bb_u4{t[w & 0xff], t[(w >> 8) & 0xff], t[(w >> 16) & 0xff], t[w >> 24]};
    } else {
        const uint32_t w0 = *reinterpret_cast<const uint32_t *>(stage + b);
        const uint32_t w1 = both ? *reinterpret_cast<const uint32_t *>(stage + b + 4) : 0u;
        return bb_u4{(uint32_t)s_tab[w0 & 0xff] | ((uint32_t)s_tab[(w0 >> 8) & 0xff] << 16),
                     (uint32_t)s_tab[(w0 >> 16) & 0xff] | ((uint32_t)s_tab[w0 >> 24] << 16),
                     (uint32_t)s_tab[w1 & 0xff] | ((uint32_t)s_tab[(w1 >> 8) & 0xff] << 16),
                     (uint32_t)s_tab[(w1 >> 16) & 0xff] | ((uint32_t)s_tab[w1 >> 24] << 16)};
    }
}

// 8 elements (or the first 4: `both` false) to p; one 16-byte store when p is 16-byte aligned
__device__ __forceinline__ void bb_half_store(uint16_t *p, bb_u4 v, bool aligned16, bool both)
{
    if (aligned16 && both) {
        __builtin_nontemporal_store(v, reinterpret_cast<bb_u4 *>(p));
    } else {
        __builtin_nontemporal_store(bb_u2{v.x, v.y}, reinterpret_cast<bb_u2 *>(p));
        if (both) __builtin_nontemporal_store(bb_u2{v.z, v.w}, reinterpret_cast<bb_u2 *>(p + 4));
    }
}

template <int BPS, int NW, int MAXT>
__global__ __launch_bounds__(NW * BB_WAVE)
void k_decode_half_flat(bb_half_args a)
{
    static_assert(BPS == 1 || BPS == 2 || BPS == 4 || BPS == 8, "1-, 2-, 4- or 8-bit samples");
    constexpr int EPB = 8 / BPS;                            // elements per payload byte
    constexpr int NPASS = MAXT * 256 * EPB / 512;           // 1 KiB store passes a wave makes at most
    constexpr int NPIECE = (MAXT + 1) * 16;                 // 16-byte pieces a wave stages at most
    constexpr int NLOAD = (NPIECE + BB_WAVE - 1) / BB_WAVE;
    __shared__ __attribute__((aligned(16))) uint16_t s_tab[256 * EPB];
    __shared__ bb_u4 s_stage[NW][NPIECE];
    bb_half_byte_table<BPS>(s_tab, a.tab, NW * BB_WAVE);
    __syncthreads();
    const int lane = bb_lane();
    const int wave = __builtin_amdgcn_readfirstlane(bb_wave());
    const uint64_t E = a.ndw * (32 / BPS);
    const uint64_t nwork = a.nfs * a.nseg;
    const uint64_t pbytes = a.ndw * 4;
    const bb_u4 fillv = bb_u4{a.fill, a.fill, a.fill, a.fill};
    // 8-bit samples: a frame is 8 * ndw bytes of output, 16-byte aligned only when ndw is even
    const bool al16 = BPS != 8 || !(a.ndw & 1);
    const uint8_t *stage8 = reinterpret_cast<const uint8_t *>(&s_stage[wave][0]);
    uint32_t *stage32 = reinterpret_cast<uint32_t *>(&s_stage[wave][0]);

    for (uint64_t step = blockIdx.x; step < nwork; step += gridDim.x) {
        const uint64_t work = bb_perm(a.perm, step);
        uint64_t fs, seg;
        if (a.nseg == 1) { fs = work; seg = 0; }
        else { fs = work / a.nseg; seg = work - fs * a.nseg; }
        const int64_t so = bb_src_at(a, fs);
        const bool valid = bb_src_ok(so, a.src_lim);
        const uint64_t tile0 = seg * a.seg_tiles + (uint64_t)wave * a.tpw;
        const uint64_t seg_b_end = (seg + 1) * a.seg_tiles * 256 < pbytes ? (seg + 1) * a.seg_tiles * 256 : pbytes;
        const uint64_t b0 = tile0 * 256;                                  // first payload byte of this wave
        uint64_t nb = 0;                                                  // bytes this wave decodes
        if (b0 < seg_b_end) { nb = seg_b_end - b0; if (nb > (uint64_t)a.tpw * 256) nb = (uint64_t)a.tpw * 256; }
        uint16_t *obase = a.out + fs * E + b0 * EPB;
        uint32_t s = 0;
        if (valid && nb && (reinterpret_cast<uintptr_t>(a.buf + (uint64_t)so) & 3)) {
            // a payload at an odd address: byte loads, staged from offset 0
            const uint8_t *pp = a.buf + (uint64_t)so + b0;
            uint8_t *st8 = reinterpret_cast<uint8_t *>(&s_stage[wave][0]);
#pragma nounroll
            for (uint32_t i = (uint32_t)lane; i < (uint32_t)nb; i += BB_WAVE) st8[i] = pp[i];
        } else if (valid && nb) {
            const uint8_t *pp = a.buf + (uint64_t)so + b0;                // 4-byte aligned
            s = (uint32_t)(reinterpret_cast<uintptr_t>(pp) & 255);
            const uint8_t *base = pp - s;                                 // 256-byte aligned address
            const uint32_t lo = s, hi = s + (uint32_t)nb;                 // wanted bytes of the staged image
#pragma unroll
            for (int k = 0; k < NLOAD; ++k) {
                const uint32_t piece = (uint32_t)k * BB_WAVE + (uint32_t)lane;
                const uint32_t p0 = piece * 16;
                if (piece >= (uint32_t)NPIECE || p0 + 16 <= lo || p0 >= hi) continue;
                if (p0 >= lo && p0 + 16 <= hi) {
                    __builtin_amdgcn_global_load_lds(
                        (const __attribute__((address_space(1))) void *)(base + p0),
                        (__attribute__((address_space(3))) void *)(&s_stage[wave][k * BB_WAVE]), 16, 0, 0);
                } else {
#pragma unroll
                    for (int d = 0; d < 4; ++d) {
                        const uint32_t q = p0 + 4 * d;
                        if (q >= lo && q + 4 <= hi) stage32[piece * 4 + d] = *reinterpret_cast<const uint32_t *>(base + q);
                    }
                }
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                 // the direct-to-LDS loads have landed
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const uint32_t e_end = (uint32_t)nb * EPB;                        // elements of this wave
#pragma unroll
        for (int p = 0; p < NPASS; ++p) {
            if ((uint32_t)p * 512 >= e_end) break;
            const uint32_t e = (uint32_t)p * 512 + 8 * (uint32_t)lane;
            if (e >= e_end) continue;
            const bool both = BPS != 8 || e + 8 <= e_end;                 // (8-bit: nb is a multiple of 4 only)
            bb_u4 v = fillv;
            if (valid) v = bb_half_expand<BPS>(s_tab, stage8, s + e / EPB, both);
            bb_half_store(obase + e, v, al16, both);
        }
        __builtin_amdgcn_wave_barrier();          // the next step overwrites the staging area
    }
}

template <int BPS>
__global__ __launch_bounds__(BB_BLOCK)
void k_decode_half_rows(bb_half_args a)
{
    static_assert(BPS == 1 || BPS == 2 || BPS == 4 || BPS == 8, "1-, 2-, 4- or 8-bit samples");
    constexpr int EPB = 8 / BPS;
    __shared__ __attribute__((aligned(16))) uint16_t s_tab[256 * EPB];
    // [nslot] payload offsets of the frame set (-1 = fill), then nslot * seg_bytes staged bytes
    extern __shared__ __attribute__((aligned(16))) uint8_t s_dyn[];
    int64_t *s_so = reinterpret_cast<int64_t *>(s_dyn);
    uint8_t *stage = s_dyn + (size_t)a.nslot * 8;
    bb_half_byte_table<BPS>(s_tab, a.tab, BB_BLOCK);
    const uint32_t nslot = a.nslot, chunk = a.chunk, lchunk = a.lchunk, segb = a.seg_bytes;
    const uint64_t E = a.ndw * (32 / BPS);
    const uint64_t pbytes = a.ndw * 4;
    const uint64_t nframes = a.nfs / nslot;
    const uint64_t nwork = nframes * a.nseg;
    const bb_u4 fillv = bb_u4{a.fill, a.fill, a.fill, a.fill};

    for (uint64_t step = blockIdx.x; step < nwork; step += gridDim.x) {
        const uint64_t work = bb_perm(a.perm, step);
        uint64_t f, seg;
        if (a.nseg == 1) { f = work; seg = 0; }
        else { f = work / a.nseg; seg = work - f * a.nseg; }
        const uint64_t b0 = seg * segb;                                   // first payload byte of this item
        const uint32_t nb = pbytes - b0 < segb ? (uint32_t)(pbytes - b0) : segb;
        __syncthreads();                          // the table is built / the last item has been written
        for (uint32_t sl = threadIdx.x; sl < nslot; sl += BB_BLOCK) {
            const uint64_t fs = f * nslot + sl;
            const int64_t so = bb_src_at(a, fs);
            s_so[sl] = bb_src_ok(so, a.src_lim) ? so : -1;
        }
        __syncthreads();
        const uint32_t ndws = nb / 4;
        for (uint32_t i = threadIdx.x; i < nslot * ndws; i += BB_BLOCK) {
            const uint32_t sl = i / ndws, j = i - sl * ndws;
            const int64_t so = s_so[sl];
            if (so < 0) continue;
            const uint8_t *pp = a.buf + (uint64_t)so + b0 + 4 * (uint64_t)j;
            uint32_t w;
            if (reinterpret_cast<uintptr_t>(pp) & 3)
                w = (uint32_t)pp[0] | ((uint32_t)pp[1] << 8) | ((uint32_t)pp[2] << 16) | ((uint32_t)pp[3] << 24);
            else
                w = *reinterpret_cast<const uint32_t *>(pp);
            reinterpret_cast<uint32_t *>(stage + (size_t)sl * segb)[j] = w;
        }
        __syncthreads();
        const uint32_t ser = nb * EPB;                                    // elements per slot in this item
        const uint64_t e0 = b0 * EPB;                                     // first element per slot
        uint16_t *oframe = a.out + f * nslot * E;
        if (chunk >= 8) {
            // a lane's 8 elements lie inside one thread sample: units in output order are
            // (row, slot, 8-element group of the chunk); an item narrower than a chunk
            // (chunk > seg_bytes' elements) holds one piece of one row per slot
            const uint32_t cw = chunk < ser ? chunk : ser;
            const uint32_t gpc = cw / 8;
            const uint32_t nunit = nslot * (ser / 8);
            for (uint32_t u = threadIdx.x; u < nunit; u += BB_BLOCK) {
                const uint32_t t = u / gpc, cg = u - t * gpc;
                const uint32_t rl = t / nslot, sl = t - rl * nslot;
                const uint32_t el = rl * cw + cg * 8;
                const uint64_t e = e0 + el;
                bb_u4 v = fillv;
                if (s_so[sl] >= 0) v = bb_half_expand<BPS>(s_tab, stage + (size_t)sl * segb, el / EPB);
                uint16_t *o = oframe + (((e >> lchunk) * nslot + sl) << lchunk) + (e & (chunk - 1));
                bb_half_store(o, v, true, true);          // (E is a multiple of the chunk: 16-byte aligned)
            }
        } else {
            // narrow chunks: whole rows are staged (chunk <= 8 <= elements per item), the item's
            // output is one run of nslot * ser elements; element by element through the byte table
            const uint32_t ntot = nslot * ser;                            // a multiple of 4
            uint16_t *orun = oframe + e0 * nslot;
            const bool al16 = (reinterpret_cast<uintptr_t>(orun) & 15) == 0;
            for (uint32_t u = threadIdx.x; u * 8 < ntot; u += BB_BLOCK) {
                const bool both = u * 8 + 8 <= ntot;
                uint32_t t = (u * 8) >> lchunk;
                uint32_t rl = t / nslot, sl = t - rl * nslot;
                uint32_t pk[4] = {0, 0, 0, 0};
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const uint32_t c = (u * 8 + k) & (chunk - 1);
                    if (k && c == 0 && ++sl == nslot) { sl = 0; ++rl; }
                    uint32_t val = (k & 1) ? a.fill >> 16 : a.fill & 0xffffu;
                    if ((both || k < 4) && s_so[sl] >= 0) {
                        const uint32_t el = (rl << lchunk) + c;
                        val = s_tab[(uint32_t)stage[(size_t)sl * segb + el / EPB] * EPB + (el & (EPB - 1))];
                    }
                    pk[k >> 1] |= val << (16 * (k & 1));
                }
                bb_half_store(orun + (size_t)u * 8, bb_u4{pk[0], pk[1], pk[2], pk[3]}, al16, both);
            }
        }
    }
}
