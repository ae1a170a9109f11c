// Time-resolved sampler statistics: how often each raw code occurs per (thread slot,
// time bin, position in the row), counted from the packed bytes (bb_count_states_bins).
// EXTENSION -- the reference has no counterpart; codes are fields taken LSB first, as in
// k_states.h.
//
// Shape (gfx950): a read-only stream like k_count_states, but the answer is a series, so
// the byte histogram of that kernel (expanded once per workgroup) does not carry over:
// per bin the expansion would cost more than a short bin's bytes.  Here every wave owns
// a WINDOW of BB_BINS_WIN output counters in LDS: the counters of win_bins consecutive
// bins of one slot, chunk << bps per bin, laid out as d_counts is.  Codes are added
// straight to window[((bin - base) * chunk + pos) << bps | code].
//
// Work items are at most BB_STATES_SEG bytes of one frame-slot (four 16-byte loads per
// lane, all issued before the first add), cut shorter by the host where bins are so short
// that an item would meet more bins than a window holds.  Items are numbered slot-major
// and in time order inside a slot, and a wave walks a CONTIGUOUS run of them: the bins
// it meets only grow.  It writes its window out (skipping zeros, one 32-bit integer
// atomic per counter, contiguous lanes on contiguous counters) only when the next item
// does not fit behind the window's first bin, when the slot changes, and at its end: a
// bin of many frames costs each wave one flush, a short bin what its output costs.
// Integer adds commute: the result is the same bit for bit whatever the order.
//
// Bins are whole bytes of a slot's stream (the host checks), a row range begins and ends
// on a byte: there is no field-by-field edge.  Payloads may lie at any byte address: the
// bytes in front of and behind the 16-byte aligned middle of an item are read one by one,
// nothing outside the payload is read.  A wave load that repeats one dword throughout (a
// fill pattern, a dead channel) is added per bin by 16 lanes, one per byte phase: 64
// lanes on one LDS address would serialise.  For the same reason rows that divide a byte
// (chunk * bps <= 8 with 1- and 2-bit codes: 16 counters a bin at most, which every lane
// meets) are counted per (position, code) with masks and popcounts in registers and added
// once per 16-byte piece (bb_bins_add16_rows): with one LDS add per code the long-bin rows
// of tools/bench_state_bins.py took 4.7-4.8 ms a GiB, with this 0.9 (profiles/state_bins.log).
#pragma once
#include "bb_common.h"
#include "k_states.h"

#define BB_BINS_WIN 2048u                                    // counters of a wave's window (8 KiB)
#define BB_BINS_MAX_PER_BIN 1024u                            // chunk << bps at most: two bins fit a window

struct bb_state_bins_args {
    const uint8_t *buf;
    const int64_t *src;          // payload offsets, NULL: src0 + (f * nslot + slot) * src_stride
    uint32_t *counts;
    uint64_t src_lim;            // bb_src_ok
    int64_t  src0, src_stride;
    uint64_t payload;            // bytes per frame-slot
    uint64_t lo_byte, hi_byte;   // bytes of a slot's request (frame after frame) that count
    uint64_t first_byte;         // place of lo_byte in the slot's series
    uint64_t bin_bytes;          // bytes of a slot per bin
    uint64_t nbins;
    uint64_t f_lo, nfr;          // first frame with a counted byte, frames with one
    uint64_t nseg;               // work items per frame-slot
    uint64_t nwork;              // nslot * nfr * nseg
    uint64_t per;                // work items of a wave's run
    uint32_t seg_bytes;          // bytes of a work item
    uint32_t nslot, chunk, bps;
    uint32_t lnc;                // log2(chunk << bps): counters per bin
    uint32_t win_bins;           // bins of a window: BB_BINS_WIN >> lnc
};

// Bin (relative to the item's first) of byte t of an item, and the bytes left in that bin
// from t on (at least 1, cut to 32 bits: an item has 4096 bytes at most).  left0: bytes
// of the item's first bin from its byte 0 on; bbc: bytes per bin, cut to 32 bits.
__device__ __forceinline__ void bb_bins_at(uint32_t t, uint64_t left0, uint32_t bbc, uint32_t &lb, uint32_t &left)
{
    if ((uint64_t)t < left0) {
        const uint64_t d = left0 - t;
        lb = 0;
        left = d > 0xffffffffull ? 0xffffffffu : (uint32_t)d;
    } else {
        const uint32_t x = t - (uint32_t)left0;
        const uint32_t q = x / bbc;
        lb = 1u + q;
        left = bbc - (x - q * bbc);
    }
}

// One byte, whatever the width (the bytes around the aligned middle).  ph: payload offset
// of the byte (its low bits); wb: window index of its bin.
__device__ __forceinline__ void bb_bins_add_byte(uint32_t *win, uint32_t v, uint32_t ph, uint32_t wb,
                                                 uint32_t bps, uint32_t lbps, uint32_t cm, uint32_t lnc, uint32_t n)
{
    const uint32_t mask = (1u << bps) - 1u;
    const uint32_t e0 = ph << (3u - lbps);                   // index of the byte's first field in the payload
    for (uint32_t b = 0, k = 0; b < 8u; b += bps, ++k)
        atomicAdd(&win[(wb << lnc) + ((((e0 + k) & cm) << bps) | ((v >> b) & mask))], n);
}

// The 16 bytes of a piece that lie in one bin, for rows that divide a byte (chunk * bps <= 8,
// bps <= 2): position p of a row is the fields k = p (mod chunk) of every byte, so the codes
// of a dword are counted per (position, code) with masks and popcounts in registers and added
// once per piece, zeros skipped: chunk << bps adds instead of 128 / bps, on the few counters
// that every lane of the wave meets.  rep: a one at the lowest bit of every row of a dword.
template <int BPS>
__device__ __forceinline__ void bb_bins_add16_rows(uint32_t *bin, const bb_u4 &v, uint32_t chunk, uint32_t rep)
{
    constexpr uint32_t NLEV = 1u << BPS;
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t m[NLEV][4];                                     // fields that hold code c, marked at their lowest bit
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        if constexpr (BPS == 1) {
            m[0][d] = ~w[d];
            m[1][d] = w[d];
        } else {
            const uint32_t lo = w[d] & 0x55555555u, hi = (w[d] >> 1) & 0x55555555u;
            m[0][d] = ~(lo | hi) & 0x55555555u;
            m[1][d] = lo & ~hi;
            m[2][d] = hi & ~lo;
            m[3][d] = lo & hi;
        }
    }
    for (uint32_t p = 0; p < chunk; ++p) {
        const uint32_t pm = rep << (p * BPS);
#pragma unroll
        for (uint32_t c = 0; c < NLEV; ++c) {
            const uint32_t cnt = (uint32_t)(__popc(m[c][0] & pm) + __popc(m[c][1] & pm) + __popc(m[c][2] & pm)
                                            + __popc(m[c][3] & pm));
            if (cnt) atomicAdd(&bin[(p << BPS) | c], cnt);
        }
    }
}

// The 16 bytes of a piece.  ph: payload offset of its first byte; wb / left: window index
// of that byte's bin, bytes left in it.
template <int BPS>
__device__ __forceinline__ void bb_bins_add16(uint32_t *win, const bb_u4 &v, uint32_t ph, uint32_t wb, uint32_t left,
                                              uint32_t bbc, uint32_t cm, uint32_t lnc, uint32_t rep)
{
    constexpr uint32_t FPB = 8u / BPS, M = (1u << BPS) - 1u;
    if (left >= 16u) {
        uint32_t *bin = win + (wb << lnc);
        if constexpr (BPS <= 2) {
            if (rep) { bb_bins_add16_rows<BPS>(bin, v, cm + 1u, rep); return; }   // (wave-uniform)
        }
#pragma unroll 1
        for (int i = 0; i < 4; ++i) {
            const uint32_t wi = i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w;   // (no indexed registers)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t byte = (wi >> (8 * j)) & 0xffu;
                const uint32_t e0 = (ph + (uint32_t)(4 * i + j)) * FPB;
#pragma unroll
                for (uint32_t k = 0; k < FPB; ++k)
                    atomicAdd(&bin[(((e0 + k) & cm) << BPS) | ((byte >> (k * BPS)) & M)], 1u);
            }
        }
        return;
    }
#pragma unroll 1
    for (int i = 0; i < 4; ++i) {
        const uint32_t wi = i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (left == 0) { ++wb; left = bbc; }
            --left;
            const uint32_t byte = (wi >> (8 * j)) & 0xffu;
            const uint32_t e0 = (ph + (uint32_t)(4 * i + j)) * FPB;
#pragma unroll
            for (uint32_t k = 0; k < FPB; ++k)
                atomicAdd(&win[(wb << lnc) + ((((e0 + k) & cm) << BPS) | ((byte >> (k * BPS)) & M))], 1u);
        }
    }
}

// The window's counters that are in use -> d_counts; the window is zero afterwards.
__device__ __forceinline__ void bb_bins_flush(uint32_t *win, const bb_state_bins_args &a, uint32_t slot, uint64_t base,
                                              uint32_t used, int lane)
{
    if (base >= a.nbins) used = 0;                           // (the host lets no counted byte past nbins)
    else if ((uint64_t)used > a.nbins - base) used = (uint32_t)(a.nbins - base);
    const uint32_t n = used << a.lnc;
    uint32_t *out = a.counts + (((uint64_t)slot * a.nbins + base) << a.lnc);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (uint32_t i = (uint32_t)lane; i < n; i += BB_WAVE) {
        const uint32_t c = win[i];
        if (c) {
            __hip_atomic_fetch_add(out + i, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            win[i] = 0;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__global__ __launch_bounds__(BB_BLOCK, 4)                    // 4 waves per SIMD: 128 VGPRs, as many as the LDS windows allow
void k_count_state_bins(bb_state_bins_args a)
{
    __shared__ uint32_t s_bins[BB_WAVES_PER_BLOCK * BB_BINS_WIN];
    const int lane = bb_lane();
    const int wave = __builtin_amdgcn_readfirstlane(bb_wave());
    uint32_t *win = s_bins + (uint32_t)wave * BB_BINS_WIN;
    for (uint32_t i = (uint32_t)lane; i < BB_BINS_WIN; i += BB_WAVE) win[i] = 0;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();

    // this wave's run of work items: item w is (slot, frame, piece), slot-major
    uint64_t w = ((uint64_t)blockIdx.x * BB_WAVES_PER_BLOCK + (uint64_t)wave) * a.per;
    if (w >= a.nwork) return;
    const uint64_t wend = a.nwork - w < a.per ? a.nwork : w + a.per;
    const uint64_t per_slot = a.nfr * a.nseg;
    uint32_t slot_next = (uint32_t)(w / per_slot);
    uint64_t fr = (w - (uint64_t)slot_next * per_slot) / a.nseg;
    uint64_t seg_next = w - (uint64_t)slot_next * per_slot - fr * a.nseg;

    const uint32_t lbps = a.bps == 8 ? 3u : a.bps == 4 ? 2u : a.bps == 2 ? 1u : 0u;
    const uint32_t cm = a.chunk - 1u, lnc = a.lnc;
    const uint32_t bbc = a.bin_bytes > 0xffffffffull ? 0xffffffffu : (uint32_t)a.bin_bytes;
    const uint32_t cb = a.chunk * a.bps;                     // bits per row
    const uint32_t rep = (a.bps <= 2 && cb <= 8) ? 0xffffffffu / ((1u << cb) - 1u) : 0u;   // bb_bins_add16_rows
    uint32_t wslot = 0, wused = 0;                           // the window: slot, first bin, bins in use
    uint64_t wbase = 0;

    for (; w < wend; ++w) {
        const uint64_t f = a.f_lo + fr;
        const uint32_t slot = slot_next;
        const uint64_t seg = seg_next;
        if (++seg_next == a.nseg) { seg_next = 0; if (++fr == a.nfr) { fr = 0; ++slot_next; } }   // (the item after this one)
        const uint64_t fs = f * a.nslot + slot;
        const int64_t so = bb_src_at(a, fs);
        if (!bb_src_ok(so, a.src_lim)) continue;             // missing, invalid or outside the buffer: counts nothing
        // bytes [q0, q1) of this frame-slot
        const uint64_t fbyte = f * a.payload;
        const uint64_t lo = a.lo_byte > fbyte ? a.lo_byte - fbyte : 0;
        const uint64_t hi = a.hi_byte - fbyte < a.payload ? a.hi_byte - fbyte : a.payload;
        uint64_t q0 = seg * a.seg_bytes, q1 = q0 + a.seg_bytes;
        if (q0 < lo) q0 = lo;
        if (q1 > hi) q1 = hi;
        if (q0 >= q1) continue;
        const uint32_t n = (uint32_t)(q1 - q0);
        // where they lie in the series
        const uint64_t G0 = a.first_byte + (fbyte + q0 - a.lo_byte);
        const uint64_t b0 = G0 / a.bin_bytes;
        const uint64_t left0 = a.bin_bytes - (G0 - b0 * a.bin_bytes);
        const uint32_t nb = (uint64_t)(n - 1u) < left0 ? 1u : 2u + ((n - 1u) - (uint32_t)left0) / bbc;
        if (wused == 0 || slot != wslot || b0 + nb > wbase + a.win_bins) {
            if (wused) bb_bins_flush(win, a, wslot, wbase, wused, lane);
            wslot = slot; wbase = b0; wused = 0;
        }
        const uint32_t lbase = (uint32_t)(b0 - wbase);
        if (lbase + nb > wused) wused = lbase + nb;          // (<= win_bins: the host cuts items to fit a window)

        const uint8_t *p0 = a.buf + (uint64_t)so + q0;
        const uint32_t qlow = (uint32_t)q0;
        const bb_pieces x = bb_pieces_split(p0, n);
        const bb_u4 *pmid = reinterpret_cast<const bb_u4 *>(p0 + x.nhead);
        bb_u4 v[BB_STATES_NL];
#pragma unroll
        for (int k = 0; k < BB_STATES_NL; ++k) bb_piece_load(v[k], pmid, x.nmid, (uint32_t)k * BB_WAVE + (uint32_t)lane);
        uint32_t off;
        if (bb_pieces_edge_byte(x, lane, off)) {
            uint32_t lb, left;
            bb_bins_at(off, left0, bbc, lb, left);
            bb_bins_add_byte(win, p0[off], qlow + off, lbase + lb, a.bps, lbps, cm, lnc, 1u);
        }
#pragma unroll
        for (int k = 0; k < BB_STATES_NL; ++k) {
            const uint32_t k0 = (uint32_t)k * BB_WAVE;
            if (k0 >= x.nmid) break;
            const uint32_t W = (uint32_t)__builtin_amdgcn_readfirstlane((int)v[k].x);     // (lane 0 holds a piece: k0 < x.nmid)
            const uint32_t nv = x.nmid - k0 < BB_WAVE ? x.nmid - k0 : BB_WAVE;            // pieces of this load
            const uint32_t ta = x.nhead + (k0 << 4);                                        // its first byte
            if (bbc >= 64u && __all((uint32_t)lane >= nv || bb_piece_repeats(v[k], W))) {
                // nv pieces that repeat one dword: bin after bin, lane o < 16 adds the bytes at ta + o + 16 m
                const uint32_t tb = ta + (nv << 4);
                uint32_t lb, left;
                bb_bins_at(ta, left0, bbc, lb, left);
                for (uint32_t t = ta; t < tb; ++lb) {
                    const uint32_t e = tb - t < left ? tb : t + left;
                    if (lane < 16) {
                        const uint32_t o = (uint32_t)lane;
                        const uint32_t cnt = ((e - ta + 15u - o) >> 4) - ((t - ta + 15u - o) >> 4);
                        if (cnt)
                            bb_bins_add_byte(win, (W >> (8u * (o & 3u))) & 0xffu, qlow + ta + o, lbase + lb,
                                             a.bps, lbps, cm, lnc, cnt);
                    }
                    t = e;
                    left = bbc;
                }
            } else if (k0 + (uint32_t)lane < x.nmid) {
                const uint32_t t0 = ta + ((uint32_t)lane << 4);
                uint32_t lb, left;
                bb_bins_at(t0, left0, bbc, lb, left);
                switch (a.bps) {
                case 1:  bb_bins_add16<1>(win, v[k], qlow + t0, lbase + lb, left, bbc, cm, lnc, rep); break;
                case 2:  bb_bins_add16<2>(win, v[k], qlow + t0, lbase + lb, left, bbc, cm, lnc, rep); break;
                case 4:  bb_bins_add16<4>(win, v[k], qlow + t0, lbase + lb, left, bbc, cm, lnc, rep); break;
                default: bb_bins_add16<8>(win, v[k], qlow + t0, lbase + lb, left, bbc, cm, lnc, rep); break;
                }
            }
        }
    }
    if (wused) bb_bins_flush(win, a, wslot, wbase, wused, lane);
}
