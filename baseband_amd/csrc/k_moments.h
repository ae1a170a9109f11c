// Sums per time bin straight from the stored bytes of int8 block streams: the two walks over the
// bytes that every such statistic shares (bb_binned_run, bb_binned_rows), and the first of them,
// power and moments: the sums of x and of x * x of every real component (bb_i8_moments).  The
// second, the cross-polarisation products, is k_coherence.h.  EXTENSION -- the reference has no
// counterpart: there the numbers come from a read followed by a reduction.
//
// Shape (gfx950): a read-only stream, 16 bytes per lane and BB_MOM_U wave loads issued before
// the first use, nontemporal, int32 lane partials, int64 totals that leave as 64-bit atomics, no
// LDS.  A walk knows addresses, ranges, bins and when partials must leave; WHAT is added is an
// accumulator type's business (bb_mom_run_acc, bb_mom_rows_acc<V> below).  Two walks, picked by
// a.mode (wave-uniform):
//
//   RUN  (bb_binned_run): a contiguous run along time per unit (a channel), P bytes per time.
//        Pieces are the 16-byte aligned ones of memory that meet the run, whatever the run's own
//        alignment; a piece that is not wholly inside it is loaded dword by dword, the dwords
//        that hold a counted byte only.  A group of wave loads that lies in one bin is added
//        whole; one that meets several bins or a range edge is walked once per bin, edge dwords
//        handed to the accumulator with their place, over the loads that bin meets: bins shorter
//        than a wave load cost a pass each.  The accumulator folds its lanes' partials into wave
//        totals after FOLD passes, and the totals leave when the (run, bin) changes and at the
//        wave's end.
//   ROWS (bb_binned_rows): rows of a multiple of 4 bytes, time along the rows.  A lane owns V
//        dwords of fixed columns of the row (V = 4 where rows, offsets and the buffer are
//        multiples of 16 bytes, else 1) and walks down the rows; rows narrower than a wave load
//        take several rows per load.  Groups of loads end at bin edges, so a wave's partials
//        belong to one bin; they leave as atomics (lanes on the same columns added up first where
//        their number is a power of two) when the (column block, bin) changes, after FOLD rows
//        over all lanes, and at the wave's end.
//
// Work items are numbered unit-major (run or column block), frames and pieces in time order
// inside, and a wave walks a CONTIGUOUS range of them, as k_count_state_bins does: the bins
// it meets only grow, and a bin of many items costs a wave one flush, not one per item.
// Integer adds commute: the result is the same bit for bit whatever the order.
//
// Moments.  A dword w adds to four byte-phase sums with v_dot4c_i32_i8: sdot4(w, 1 << 8 j) is
// byte j, sdot4(w, w & (0xff << 8 j)) its square; a byte mask on w serves range and bin edges
// that fall inside a dword.  RUN (GUPPI channels first; rows of 1, 2 or 4 bytes as one run): a
// component repeats every P = 1, 2 or 4 bytes, so the byte phase of a dword IS the component;
// lanes keep eight int32 partials, a fold adds them up (shuffles) into eight int64 totals, one in
// each of the wave's first eight lanes.  ROWS (GUPPI time first; rows of a multiple of 4 bytes):
// eight partials per dword of the lane.  Everything that lives longer than a fold is int64.
#pragma once
#include "bb_common.h"

#define BB_MOM_RUN  0u
#define BB_MOM_ROW1 1u
#define BB_MOM_ROW4 2u
#define BB_MOM_U 4                                           // wave loads in flight
#define BB_MOM_STEP 1024u                                    // RUN: bytes of a wave load
#define BB_MOM_RUN_STEPS 16u                                 // RUN: wave loads of a work item (16 KiB)
#define BB_MOM_ROW_STEPS 32u                                 // ROWS: wave loads of a work item
// A dot4 adds at most 4 * 128 * 128 = 2^16, 2^14 of it to one byte phase.  RUN: a lane adds at most
// 16 dwords a pass, so 64 passes give a byte phase at most 64 * 16 * 2^14 = 2^24 a lane, 2^30
// over the 64 lanes that the fold adds up in int32.
#define BB_MOM_RUN_FOLD 64u
// ROWS: rows over ALL lanes; a column gets at most 2^16 * 2^14 = 2^30, also after the lanes are added.
#define BB_MOM_ROW_FOLD 65536u

struct bb_moments_args {
    const uint8_t *buf;
    const int64_t *src;          // payload offsets (multiples of 4), NULL: src0 + f * src_stride
    long long *sums;
    uint64_t src_lim;            // bb_src_ok
    int64_t  src0, src_stride;
    uint64_t pay_bytes;          // bytes of a payload: nothing behind them is read
    uint64_t nframes;
    uint64_t t_lo, nt;           // times [t_lo, t_lo + nt) of every payload count
    uint64_t first_row, bin_rows, nbins;
    uint64_t pitch;              // RUN: bytes from one run of a payload to the next
    uint64_t nseg;               // work items per (run or column block, frame)
    uint64_t nwork, per;         // work items; those of a wave's range
    uint32_t mode;
    uint32_t P;                  // RUN: bytes per time of a run
    uint32_t nrun;               // RUN: runs of a payload; ROWS: column blocks of 64 lane columns
    uint32_t Rb;                 // ROWS: bytes of a row
    uint32_t NV;                 // ROWS: lane columns of a row, Rb / (4 V)
    uint32_t rpl;                // ROWS: rows of a wave load
    uint32_t chunk_rows;         // ROWS: rows of a work item
    uint32_t tf, nchan;          // ROWS: columns are (chan, pol, re/im) and leave as (pol, chan, re/im)
    uint32_t bin_elems;          // components of a bin
    uint32_t c_stride;           // RUN: components from one run to the next
    uint32_t ph_off[4];          // RUN: component of byte phase j
};

typedef long long bb_i64;

// A wave-uniform value back in scalar registers (64-bit divisions leave theirs in vector ones).
__device__ __forceinline__ uint64_t bb_mom_uniform(uint64_t x)
{
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(x >> 32)) << 32)
           | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)x);
}

__device__ __forceinline__ void bb_mom_dot(uint32_t w, int32_t (&sx)[4], int32_t (&sq)[4])
{
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        sx[j] = __builtin_amdgcn_sdot4((int)w, (int)(1u << (8 * j)), sx[j], false);
        sq[j] = __builtin_amdgcn_sdot4((int)w, (int)(w & (0xffu << (8 * j))), sq[j], false);
    }
}

__device__ __forceinline__ void bb_mom_atomic(bb_i64 *p, bb_i64 v)
{
    if (v) __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Bytes [lo, hi) of the dword at `rel`, all three relative to a step: the mask that keeps them.
__device__ __forceinline__ uint32_t bb_mom_mask(uint32_t rel, uint32_t lo, uint32_t hi)
{
    const uint32_t a = lo > rel ? lo - rel : 0u;             // first byte kept
    const uint32_t b = hi > rel ? (hi - rel < 4u ? hi - rel : 4u) : 0u;   // one past the last
    if (a >= b) return 0u;
    return (0xffffffffu >> (8u * (4u - b))) & (0xffffffffu << (8u * a));
}

// The piece at byte `rel` of a group of wave loads that begins at g (16-byte aligned in memory)
// against the group's counted bytes [lo, hi): whole inside, one load; else its dwords that hold a
// counted byte (the last dword of a payload that does not end on a dword -- pe: the payload's end
// in the group -- is put together from its bytes).
__device__ __forceinline__ bb_u4 bb_mom_piece(const uint8_t *g, uint32_t rel, uint32_t lo, uint32_t hi, uint32_t pe)
{
    if (rel >= lo && rel + 16u <= hi) return __builtin_nontemporal_load(reinterpret_cast<const bb_u4 *>(g + rel));
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const uint32_t q = rel + 4u * (uint32_t)d;
        if (q + 4u <= lo || q >= hi) continue;
        if (q + 4u <= pe) {
            w[d] = *reinterpret_cast<const uint32_t *>(g + q);
        } else {
#pragma unroll 1
            for (uint32_t k = 0; k < 4u && q + k < pe; ++k) w[d] |= (uint32_t)g[q + k] << (8u * k);
        }
    }
    return bb_u4{w[0], w[1], w[2], w[3]};
}

// The run walk over the work items [w, wend).  Acc holds a lane's partials and the wave's totals
// of the current (run, bin) and says:
//   FOLD                      passes after which the partials must be folded
//   bytes_per_time(a)         of a run
//   payload_end(a, so, gb, hi)  the end, relative to the group at gb, of the payload at so: the
//                             dwords of a piece behind it are put together from bytes
//   add(w)                    a dword that counts whole
//   add(w, rel, lo, n)        the dword at rel of a group of which bytes [lo, lo + n) count
//   fold(lane)                partials -> totals
//   flush(a, lane, run, bin)  fold, and the totals leave
template <class Acc>
__device__ __forceinline__ void bb_binned_run(const bb_moments_args &a, const int lane, uint64_t w, const uint64_t wend)
{
    Acc acc;
    uint32_t nacc = 0;                                       // passes since the last fold
    bool have = false;
    uint64_t cur_c = 0, cur_bin = 0;
    const uint32_t P = Acc::bytes_per_time(a);
    const uint64_t bin_bytes = a.bin_rows * P;
    const uint64_t per_c = a.nframes * a.nseg;

    auto enter = [&](uint64_t c, uint64_t bin) {             // a pass adds to (c, bin): what was of another leaves first
        if (!have || c != cur_c || bin != cur_bin) {
            if (have) { acc.flush(a, lane, cur_c, cur_bin); nacc = 0; }
            have = true; cur_c = c; cur_bin = bin;
        }
    };
    auto leave = [&]() { if (++nacc >= Acc::FOLD) { acc.fold(lane); nacc = 0; } };

    uint64_t c = bb_mom_uniform(w / per_c);
    uint64_t fi = bb_mom_uniform((w - c * per_c) / a.nseg);
    uint64_t seg = w - c * per_c - fi * a.nseg;
    for (; w < wend; ++w) {
        const uint64_t c_ = c, fi_ = fi, seg_ = seg;
        if (++seg == a.nseg) { seg = 0; if (++fi == a.nframes) { fi = 0; ++c; } }   // (the item after this one)
        const int64_t so = bb_src_at(a, fi_);
        if (!bb_src_ok(so, a.src_lim) || (so & 3)) continue; // missing, outside the buffer or not on a dword: adds nothing
        // offsets into the buffer: the run's counted bytes [A0, A1), the 16-byte boundary of memory at or below A0
        const int64_t A0 = so + (int64_t)(c_ * a.pitch + a.t_lo * P), A1 = A0 + (int64_t)(a.nt * P);
        const int64_t base = A0 - (int64_t)((reinterpret_cast<uintptr_t>(a.buf) + (uint64_t)A0) & 15u);
        const uint64_t nst = ((uint64_t)(A1 - base) + BB_MOM_STEP - 1) / BB_MOM_STEP;   // (a shift)
        uint64_t st = seg_ * BB_MOM_RUN_STEPS;
        if (st >= nst) continue;
        const uint64_t st_end = st + BB_MOM_RUN_STEPS < nst ? st + BB_MOM_RUN_STEPS : nst;
        // where the item's first counted byte lies in the run's series
        const int64_t x0 = base + (int64_t)(st * BB_MOM_STEP) > A0 ? base + (int64_t)(st * BB_MOM_STEP) : A0;
        const uint64_t g = (a.first_row + fi_ * a.nt) * P + (uint64_t)(x0 - A0);
        uint64_t bin = bb_mom_uniform(g / bin_bytes);
        uint64_t left = bin_bytes - (g - bin * bin_bytes);
#pragma nounroll
        for (; st < st_end; st += BB_MOM_U) {                // a group of BB_MOM_U wave loads
            const int64_t gb = base + (int64_t)(st * BB_MOM_STEP);
            const uint8_t *gp = a.buf + gb;                  // (nothing in front of the payload is read)
            // the group's counted bytes [lo, hi), relative to the group
            uint32_t lo = gb < A0 ? (uint32_t)(A0 - gb) : 0u;
            const uint64_t gend = (st_end - st < BB_MOM_U ? st_end - st : BB_MOM_U) * BB_MOM_STEP;
            const uint32_t hi = (uint64_t)(A1 - gb) < gend ? (uint32_t)(A1 - gb) : (uint32_t)gend;
            const uint32_t pe = Acc::payload_end(a, so, gb, hi);
            bb_u4 v[BB_MOM_U];
#pragma unroll
            for (int u = 0; u < BB_MOM_U; ++u)
                v[u] = bb_mom_piece(gp, (uint32_t)u * BB_MOM_STEP + 16u * (uint32_t)lane, lo, hi, pe);
            if (lo == 0u && hi == BB_MOM_U * BB_MOM_STEP && left >= hi) {
                // the whole group lies in one bin: every dword counts whole
                enter(c_, bin);
#pragma unroll
                for (int u = 0; u < BB_MOM_U; ++u) { acc.add(v[u].x); acc.add(v[u].y); acc.add(v[u].z); acc.add(v[u].w); }
                leave();
                left -= hi;
                if (left == 0) { ++bin; left = bin_bytes; }
                continue;
            }
#pragma nounroll
            while (lo < hi) {                                // bin after bin: bytes [lo, lo + n)
                const uint32_t n = (uint64_t)(hi - lo) < left ? hi - lo : (uint32_t)left;
                enter(c_, bin);
#pragma unroll
                for (int u = 0; u < BB_MOM_U; ++u) {
                    const uint32_t s0 = (uint32_t)u * BB_MOM_STEP;
                    if (lo + n <= s0 || lo >= s0 + BB_MOM_STEP) continue;    // (wave-uniform: a load that this bin does not meet)
                    const uint32_t rel = s0 + 16u * (uint32_t)lane;
                    acc.add(v[u].x, rel, lo, n);       acc.add(v[u].y, rel + 4u, lo, n);
                    acc.add(v[u].z, rel + 8u, lo, n);  acc.add(v[u].w, rel + 12u, lo, n);
                }
                leave();
                lo += n;
                left -= n;
                if (left == 0) { ++bin; left = bin_bytes; }
            }
        }
    }
    if (have) acc.flush(a, lane, cur_c, cur_bin);
}

template <int V> struct bb_mom_vec;
template <> struct bb_mom_vec<1> { typedef uint32_t type; };
template <> struct bb_mom_vec<4> { typedef bb_u4 type; };
__device__ __forceinline__ uint32_t bb_mom_word(const uint32_t &v, int) { return v; }
__device__ __forceinline__ uint32_t bb_mom_word(const bb_u4 &v, int d) { return d == 0 ? v.x : d == 1 ? v.y : d == 2 ? v.z : v.w; }

// The row walk over the work items [w, wend).  Acc holds a lane's partials of the current (column
// block, bin) and says:
//   V, FOLD            dwords of a row that a lane owns; rows, over all lanes, after which the
//                      partials must leave
//   U                  groups of rpl rows in flight (BB_MOM_U wave loads)
//   row_t, load(a, p)  what a lane loads of the row whose lane columns begin at p (row_t{}: nothing)
//   add(row)           what it adds
//   flush(a, bin, vc, off0, mine)  lanes off0, 2 off0, .. < 64 apart are added up, those with
//                      `mine` add the partials of lane column vc to the sums, and all are zero again
template <class Acc>
__device__ __forceinline__ void bb_binned_rows(const bb_moments_args &a, const int lane, uint64_t w, const uint64_t wend)
{
    constexpr int V = Acc::V, U = Acc::U;
    Acc acc;
    uint32_t nacc = 0;                                       // rows since the last flush, over all lanes
    bool have = false;
    uint64_t cur_cb = 0, cur_bin = 0;
    const uint32_t NV = a.NV;
    const uint32_t dr = NV < BB_WAVE ? (uint32_t)lane / NV : 0u;                        // row of a wave load that this lane reads
    const uint32_t lc = NV < BB_WAVE ? (uint32_t)lane - dr * NV : (uint32_t)lane;      // ... and its lane column in the block
    const bool pow2 = NV < BB_WAVE && (NV & (NV - 1u)) == 0; // lanes NV apart share columns, all 64 read: add them up by shuffles
    const uint64_t per_cb = a.nframes * a.nseg;

    auto flush = [&]() {
        const uint32_t vc = (uint32_t)cur_cb * BB_WAVE + lc;
        acc.flush(a, cur_bin, vc, pow2 ? NV : BB_WAVE, pow2 ? dr == 0 : (vc < NV && dr < a.rpl));
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
            if (!have || cb_ != cur_cb || bin != cur_bin || nacc + m > Acc::FOLD) {
                if (have) flush();
                have = true; cur_cb = cb_; cur_bin = bin;
            }
            typename Acc::row_t v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t row = (uint32_t)u * a.rpl + dr;
                v[u] = typename Acc::row_t{};
                if (col_ok && row < m) v[u] = Acc::load(a, pl + (r + row) * a.Rb);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) acc.add(v[u]);
            nacc += m;
            r += m;
            left -= m;
            if (left == 0) { ++bin; left = a.bin_rows; }
        }
    }
    if (have) flush();
}

struct bb_mom_run_acc {
    static constexpr uint32_t FOLD = BB_MOM_RUN_FOLD;
    int32_t sx[4] = {0, 0, 0, 0}, sq[4] = {0, 0, 0, 0};      // this lane's partials, by byte phase
    bb_i64 tot = 0;                                          // lane i < 8: the wave's total i (2 j: x, 2 j + 1: x * x of byte phase j)

    static __device__ __forceinline__ uint32_t bytes_per_time(const bb_moments_args &a) { return a.P; }
    static __device__ __forceinline__ uint32_t payload_end(const bb_moments_args &a, int64_t so, int64_t gb, uint32_t)
    {
        const uint64_t pe = (uint64_t)(so + (int64_t)a.pay_bytes - gb);
        return pe < 2u * BB_MOM_U * BB_MOM_STEP ? (uint32_t)pe : 2u * BB_MOM_U * BB_MOM_STEP;
    }
    __device__ __forceinline__ void add(uint32_t w) { bb_mom_dot(w, sx, sq); }
    __device__ __forceinline__ void add(uint32_t w, uint32_t rel, uint32_t lo, uint32_t n) { bb_mom_dot(w & bb_mom_mask(rel, lo, lo + n), sx, sq); }
    __device__ __forceinline__ void fold(const int lane)
    {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int32_t x = sx[j], q = sq[j];
#pragma unroll
            for (int off = 32; off; off >>= 1) { x += __shfl_xor(x, off); q += __shfl_xor(q, off); }
            if (lane == 2 * j) tot += x;
            if (lane == 2 * j + 1) tot += q;
            sx[j] = 0; sq[j] = 0;
        }
    }
    __device__ __forceinline__ void flush(const bb_moments_args &a, const int lane, uint64_t c, uint64_t bin)
    {
        fold(lane);
        if (lane < 8 && bin < a.nbins) {                     // (the host lets no counted row past nbins)
            const uint32_t ph = lane < 2 ? a.ph_off[0] : lane < 4 ? a.ph_off[1] : lane < 6 ? a.ph_off[2] : a.ph_off[3];
            bb_mom_atomic(a.sums + 2 * (bin * a.bin_elems + c * a.c_stride) + 2u * ph + ((uint32_t)lane & 1u), tot);
        }
        tot = 0;
    }
};

template <int V_>
struct bb_mom_rows_acc {
    static constexpr int V = V_, U = BB_MOM_U;
    static constexpr uint32_t FOLD = BB_MOM_ROW_FOLD;
    typedef typename bb_mom_vec<V>::type row_t;
    int32_t sx[V][4] = {}, sq[V][4] = {};                    // this lane's partials, by dword and byte of it

    static __device__ __forceinline__ row_t load(const bb_moments_args &, const uint8_t *p)
    {
        return __builtin_nontemporal_load(reinterpret_cast<const row_t *>(p));
    }
    __device__ __forceinline__ void add(const row_t &v)
    {
#pragma unroll
        for (int d = 0; d < V; ++d) bb_mom_dot(bb_mom_word(v, d), sx[d], sq[d]);
    }
    __device__ __forceinline__ void flush(const bb_moments_args &a, uint64_t bin, uint32_t vc, uint32_t off0, bool mine)
    {
        for (uint32_t off = off0; off < BB_WAVE; off <<= 1) {
#pragma unroll
            for (int d = 0; d < V; ++d)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    sx[d][j] += __shfl_xor(sx[d][j], (int)off);
                    sq[d][j] += __shfl_xor(sq[d][j], (int)off);
                }
        }
        if (mine && bin < a.nbins) {                         // (the host lets no counted row past nbins)
            bb_i64 *out = a.sums + 2 * bin * a.bin_elems;
#pragma unroll
            for (int d = 0; d < V; ++d)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (sq[d][j] == 0) continue;             // (no square, no sum)
                    const uint32_t q = vc * (4u * V) + 4u * (uint32_t)d + (uint32_t)j;   // byte of the row
                    const uint32_t e = a.tf ? (((q >> 1) & 1u) * a.nchan + (q >> 2)) * 2u + (q & 1u) : q;
                    bb_mom_atomic(out + 2 * e, (bb_i64)sx[d][j]);
                    bb_mom_atomic(out + 2 * e + 1, (bb_i64)sq[d][j]);
                }
        }
#pragma unroll
        for (int d = 0; d < V; ++d)
#pragma unroll
            for (int j = 0; j < 4; ++j) { sx[d][j] = 0; sq[d][j] = 0; }
    }
};

__global__ __launch_bounds__(BB_BLOCK, 4)                    // at least 4 waves per SIMD: 128 VGPRs at most
void k_i8_moments(bb_moments_args a)
{
    const int lane = bb_lane();
    const int wave = __builtin_amdgcn_readfirstlane(bb_wave());
    // this wave's contiguous range of work items
    const uint64_t w = ((uint64_t)blockIdx.x * BB_WAVES_PER_BLOCK + (uint64_t)wave) * a.per;
    if (w >= a.nwork) return;
    const uint64_t wend = a.nwork - w < a.per ? a.nwork : w + a.per;
    switch (a.mode) {                                        // (wave-uniform)
    case BB_MOM_RUN:  bb_binned_run<bb_mom_run_acc>(a, lane, w, wend); break;
    case BB_MOM_ROW1: bb_binned_rows<bb_mom_rows_acc<1>>(a, lane, w, wend); break;
    default:          bb_binned_rows<bb_mom_rows_acc<4>>(a, lane, w, wend); break;
    }
}
