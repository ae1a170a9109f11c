// Experiment build only (make EXPERIMENTS=1): the dispatcher of rounds 1-2 with
// every measurement variant, kept as the record of those A/B runs
// (BB_TUNE_FLAT_VARIANT and friends, include/bbdecode_exp.h).  The product
// dispatch in bbdecode.hip is what variant 5 with default knobs used to pick.
namespace expd {

template <int BPS, int LV>
void launch_gather(bool nt, dim3 grid, size_t lds, hipStream_t st, const bb_gather_args &a)
{
    const bool wide = a.lchunk >= 2;
#define BB_G(NT, W) hipLaunchKernelGGL((k_decode_gather<BPS, LV, NT, W>), grid, dim3(BB_BLOCK), lds, st, a)
    if (nt) { if (wide) BB_G(true, true); else BB_G(true, false); }
    else    { if (wide) BB_G(false, true); else BB_G(false, false); }
#undef BB_G
}

template <int BPS, int LV, int NW, int TPW>
void launch_flat_pipe(int om, bool nt, dim3 grid, hipStream_t st, const bb_flat_args &a)
{
#define BB_L(OM, NT) hipLaunchKernelGGL((k_decode_flat_pipe<BPS, LV, OM, NT, NW, TPW>), grid, dim3(NW * BB_WAVE), 0, st, a)
    if (om == BB_OUT_FLAT)       { if (nt) BB_L(BB_OUT_FLAT, true);    else BB_L(BB_OUT_FLAT, false); }
    else if (om == BB_OUT_ROWS4) { if (nt) BB_L(BB_OUT_ROWS4, true);   else BB_L(BB_OUT_ROWS4, false); }
    else                         { if (nt) BB_L(BB_OUT_SCATTER, true); else BB_L(BB_OUT_SCATTER, false); }
#undef BB_L
}

template <int BPS>
void launch_flat_lut(bool nt, dim3 grid, hipStream_t st, const bb_flat_args &a)
{
    // (an instantiation sized for the default short items, 2 x 5 instead of
    // 2 x 17 block registers per lane, is SLOWER -- more workgroups per CU, more
    // write streams at a time: profiles/r02ap_exp_lut_small.log; kept behind
    // BB_TUNE_LUT_SMALL.  BB_TUNE_LDS_PAD asks for unused LDS to bound the
    // workgroups per CU from above, for the same experiment.)
    const unsigned pad = (unsigned)g_tune_lds_pad.load();
    if (a.tpw <= 4 && g_tune_lut_small.load() != 0) {
        if (nt) hipLaunchKernelGGL((k_decode_flat_lut<BPS, true, 2, 4>), grid, dim3(2 * BB_WAVE), pad, st, a);
        else    hipLaunchKernelGGL((k_decode_flat_lut<BPS, false, 2, 4>), grid, dim3(2 * BB_WAVE), pad, st, a);
        return;
    }
    if (nt) hipLaunchKernelGGL((k_decode_flat_lut<BPS, true, 2, 16>), grid, dim3(2 * BB_WAVE), pad, st, a);
    else    hipLaunchKernelGGL((k_decode_flat_lut<BPS, false, 2, 16>), grid, dim3(2 * BB_WAVE), pad, st, a);
}

template <int BPS, int LV>
void launch_flat_aln(bool nt, dim3 grid, hipStream_t st, const bb_flat_args &a)
{
    // experiment knob: unused dynamic LDS caps the workgroups per CU (160 KiB / pad)
    const size_t pad = (size_t)g_tune_lds_pad.load();
    if (nt) hipLaunchKernelGGL((k_decode_flat_aln<BPS, LV, true, 2, 16>), grid, dim3(2 * BB_WAVE), pad, st, a);
    else    hipLaunchKernelGGL((k_decode_flat_aln<BPS, LV, false, 2, 16>), grid, dim3(2 * BB_WAVE), pad, st, a);
}

// 8-bit data: one dword is only four samples, so a wave needs 32 tiles for a
// 32 KiB output run (k_decode_flat_aln<.., 2, 32>)
template <int BPS, int LV>
void launch_flat_aln32(bool nt, dim3 grid, hipStream_t st, const bb_flat_args &a)
{
    if (nt) hipLaunchKernelGGL((k_decode_flat_aln<BPS, LV, true, 2, 32>), grid, dim3(2 * BB_WAVE), 0, st, a);
    else    hipLaunchKernelGGL((k_decode_flat_aln<BPS, LV, false, 2, 32>), grid, dim3(2 * BB_WAVE), 0, st, a);
}

// k_decode_flat_front: geometry + launch.  Returns the grid size used.
template <int BPS, int LV, int NW, int TPW>
unsigned launch_flat_front(bool nt, hipStream_t st, const bb_flat_args &a)
{
    const uint64_t ntiles = (a.ndw + 63) / 64;
    bb_front_geom g;
    g.ipf = (uint32_t)((ntiles + TPW - 1) / TPW);
    g.nitems = a.nfs * g.ipf;
    uint64_t G = (uint64_t)g_tune_front_g.load(), K = (uint64_t)g_tune_front_k.load();
    const uint64_t wgs = (g.nitems + NW - 1) / NW;              // workgroup-steps in all
    if (G > wgs) G = wgs;                                       // small launch: one short group
    if (K * G > wgs) K = (wgs + G - 1) / G;
    const uint64_t ngroups = (wgs + G * K - 1) / (G * K);
    g.G = (uint32_t)G; g.K = (uint32_t)K;
    g.step_fs = (uint32_t)((G * NW) / g.ipf);
    g.step_j = (uint32_t)((G * NW) % g.ipf);
    const dim3 grid((unsigned)(ngroups * G));
    if (nt) hipLaunchKernelGGL((k_decode_flat_front<BPS, LV, true, NW, TPW>), grid, dim3(NW * BB_WAVE), 0, st, a, g);
    else    hipLaunchKernelGGL((k_decode_flat_front<BPS, LV, false, NW, TPW>), grid, dim3(NW * BB_WAVE), 0, st, a, g);
    return grid.x;
}

template <int NW, int TPW>
unsigned launch_flat_front_any(int bps, int coder, bool nt, hipStream_t st, const bb_flat_args &a)
{
    switch (bps) {
        case 1: return launch_flat_front<1, BB_LV_REG, NW, TPW>(nt, st, a);
        case 2: return launch_flat_front<2, BB_LV_REG, NW, TPW>(nt, st, a);
        case 4: return launch_flat_front<4, BB_LV_LDS, NW, TPW>(nt, st, a);
        default:
            if (coder == BB_CODER_INT) return launch_flat_front<8, BB_LV_INT8, NW, TPW>(nt, st, a);
            return launch_flat_front<8, BB_LV_LDS, NW, TPW>(nt, st, a);
    }
}

// k_decode_flat_es: one pass, U stripes
template <int BPS, int LV, int U>
unsigned launch_flat_es(bool nt, hipStream_t st, const bb_flat_args &a)
{
    const uint64_t ntiles = (a.ndw + 63) / 64;
    const uint64_t total = a.nfs * ntiles;
    const uint64_t per = (total + U - 1) / U;
    const uint64_t blocks = (per + BB_WAVES_PER_BLOCK - 1) / BB_WAVES_PER_BLOCK;
    const dim3 grid((unsigned)(blocks > 0x7fffffffull ? 0x7fffffffull : blocks));
    if (nt) hipLaunchKernelGGL((k_decode_flat_es<BPS, LV, true, U>), grid, dim3(BB_BLOCK), 0, st, a, total, per);
    else    hipLaunchKernelGGL((k_decode_flat_es<BPS, LV, false, U>), grid, dim3(BB_BLOCK), 0, st, a, total, per);
    return grid.x;
}

template <int U>
unsigned launch_flat_es_any(int bps, int coder, bool nt, hipStream_t st, const bb_flat_args &a)
{
    switch (bps) {
        case 1: return launch_flat_es<1, BB_LV_REG, U>(nt, st, a);
        case 2: return launch_flat_es<2, BB_LV_REG, U>(nt, st, a);
        case 4: return launch_flat_es<4, BB_LV_LDS, U>(nt, st, a);
        default:
            if (coder == BB_CODER_INT) return launch_flat_es<8, BB_LV_INT8, U>(nt, st, a);
            return launch_flat_es<8, BB_LV_LDS, U>(nt, st, a);
    }
}

// k_decode_flat_elem: one pass, 16 stripes of whole frames, one float4 per thread and stripe
template <int BPS, int LV>
unsigned launch_flat_elem(bool nt, hipStream_t st, const bb_flat_args &a)
{
    const uint64_t fps = (a.nfs + BB_ELEM_STRIPES - 1) / BB_ELEM_STRIPES;
    const uint64_t E4 = a.ndw * (32 / BPS) / 4;
    const uint64_t blocks = (fps * E4 + BB_BLOCK - 1) / BB_BLOCK;
    const dim3 grid((unsigned)(blocks > 0x7fffffffull ? 0x7fffffffull : blocks));
    if (nt) hipLaunchKernelGGL((k_decode_flat_elem<BPS, LV, true>), grid, dim3(BB_BLOCK), 0, st, a, fps);
    else    hipLaunchKernelGGL((k_decode_flat_elem<BPS, LV, false>), grid, dim3(BB_BLOCK), 0, st, a, fps);
    return grid.x;
}

template <int BPS, int LV>
void launch_flat_span(bool nt, dim3 grid, hipStream_t st, const bb_flat_args &a)
{
    if (nt) hipLaunchKernelGGL((k_decode_flat_span<BPS, LV, true, 2, 16>), grid, dim3(2 * BB_WAVE), 0, st, a);
    else    hipLaunchKernelGGL((k_decode_flat_span<BPS, LV, false, 2, 16>), grid, dim3(2 * BB_WAVE), 0, st, a);
}

template <int BPS, int LV>
void launch_rows_pipe(bool nt, bool aln, int nw, dim3 grid, hipStream_t st, const bb_flat_args &a)
{
#define BB_R2(NW, NT, ALN) hipLaunchKernelGGL((k_decode_rows_pipe<BPS, LV, NT, NW, 8, ALN>), grid, dim3(NW * BB_WAVE), 0, st, a)
#define BB_R(NW) do { if (aln) { if (nt) BB_R2(NW, true, true); else BB_R2(NW, false, true); } \
                      else     { if (nt) BB_R2(NW, true, false); else BB_R2(NW, false, false); } } while (0)
    if (nw == 8) BB_R(8); else if (nw == 4) BB_R(4); else BB_R(2);
#undef BB_R
#undef BB_R2
}

template <int BPS, int LV>
void launch_flat(int om, bool nt, dim3 grid, hipStream_t st, const bb_flat_args &a)
{
#define BB_L(OM, NT) hipLaunchKernelGGL((k_decode_flat<BPS, LV, OM, NT>), grid, dim3(BB_BLOCK), 0, st, a)
    if (om == BB_OUT_FLAT)       { if (nt) BB_L(BB_OUT_FLAT, true);    else BB_L(BB_OUT_FLAT, false); }
    else if (om == BB_OUT_ROWS4) { if (nt) BB_L(BB_OUT_ROWS4, true);   else BB_L(BB_OUT_ROWS4, false); }
    else                         { if (nt) BB_L(BB_OUT_SCATTER, true); else BB_L(BB_OUT_SCATTER, false); }
#undef BB_L
}


// 1 = not an experiment launch (the product dispatch runs), else a BB_* code
int decode_frames(const bb_decode_params *p, const int64_t *d_src, size_t nframes,
                  bb_flat_args a, int om, float *d_out, hipStream_t st)
{
    int variant = g_tune_variant.load();
    if (variant == 15 || variant == 16 || (variant >= 19 && variant <= 25)) variant = 5;        // (which byte-table kernel: decided by the product dispatch)
    if (variant == 5 && g_tune_byte_lut.load() != 0 && g_tune_lut_small.load() == 0
            && g_tune_lds_pad.load() == 0 && g_tune_tpw8.load() <= 16 && g_tune_tpw.load() == 12)
        return 1;
    const uint64_t nfs = a.nfs;
    const uint64_t E = p->payload_nbytes * 8 / (uint64_t)p->bps;
    const uint64_t ntiles = (a.ndw + 63) / 64;
    // plain kernel: tiles per workgroup.  8-bit samples: 16 (4 KiB in, 16 KiB
    // out per workgroup) instead of 32: +7 % at 8 GiB, +0-3.5 % at 31 GiB
    // (profiles/r02ba_exp_int8_seg.log)
    const int seg_knob = g_tune_seg_tiles.load();
    const uint64_t seg_plain = seg_knob ? (uint64_t)seg_knob : (p->bps == 8 ? 16u : (uint64_t)BB_SEG_TILES);
    split_tiles(a, ntiles, seg_plain, BB_WAVES_PER_BLOCK);
    const uint64_t nwork = nfs * a.nseg;
    const uint64_t out_bytes = nfs * E * 4;
    a.perm = make_perm(nwork, out_bytes);   // (branches that cut the work differently set their own)
    const dim3 grid = capped_grid(nwork, BB_GRID_MAX);
    const bool nt = g_tune_nt.load() != 0;

    // Kernel choice.  The default (5) is the persistent pipelined family with
    // aligned block loads -- except for 8-bit samples with contiguous output:
    // they read 20 % of their traffic instead of 6 %, and the plain
    // one-workgroup-per-32-tiles kernel with an uncapped grid is 3-6 % faster
    // there for every payload size tried (profiles/r01i_exp_int8_v0.log:
    // 5.34-5.37 -> 5.55-5.67 TB/s int8, 5.10-5.37 -> 5.44-5.58 VDIF 8-bit).
    // BB_TUNE_TILES_PER_WAVE_8BIT > 16 selects the long pipelined form again.
    if (variant == 5 && p->bps == 8 && om == BB_OUT_FLAT && g_tune_tpw8.load() <= 16)
        variant = 0;
    // 4-bit samples (11 % of the traffic is reads): the plain kernel is 3-6 %
    // ahead as well (profiles/r02t_exp_es.log, r02u_exp_es_elem.log: 5.72-5.82
    // against 5.43-5.55 TB/s at 4 and 34 GB of output)
    // -- against the register-select kernel; the byte table kernel with short
    // work items (k_lut.h) takes 4-bit samples too and is ahead of both
    if (variant == 5 && p->bps == 4 && om == BB_OUT_FLAT && g_tune_byte_lut.load() == 0) variant = 0;
    // Mid-size launches: with one or two work items per workgroup the
    // persistent pipelined kernel (5.1-5.3 TB/s) loses to the plain one
    // (5.4-5.5); from four items per workgroup on it is at least as fast on
    // freshly allocated outputs (5.8-5.9 at 2^18 frames, 6.2-6.6 beyond) --
    // how fast depends on the allocation, the plain kernel does 5.4-5.7
    // everywhere (profiles/r01i_exp_launch_size.log, r01i_exp_launch_fresh.log).
    // An explicit BB_TUNE_BLOCKS keeps the pipelined kernel (experiments).
    // (round 2: with the striped work order the two are equal there --
    // 5.60 / 5.61 TB/s at 2^16 frames, profiles/r02e_exp_order.log -- and the
    // fallback is gone)

    if (variant == 14 && om == BB_OUT_FLAT) {
        // the fill-shaped decode (k_front.h)
        unsigned gx;
        switch (p->bps) {
            case 1: gx = launch_flat_elem<1, BB_LV_REG>(nt, st, a); break;
            case 2: gx = launch_flat_elem<2, BB_LV_REG>(nt, st, a); break;
            case 4: gx = launch_flat_elem<4, BB_LV_LDS>(nt, st, a); break;
            default:
                if (p->coder == BB_CODER_INT) gx = launch_flat_elem<8, BB_LV_INT8>(nt, st, a);
                else                          gx = launch_flat_elem<8, BB_LV_LDS>(nt, st, a);
                break;
        }
        BB_NOTE("k_decode_flat_elem<%d,%s,%s> grid %u", p->bps, lv_name(p->bps, p->coder), nt ? "nt" : "plain", gx);
        BB_HIP(hipGetLastError());
        return BB_OK;
    }

    if (variant >= 10 && variant <= 12 && om == BB_OUT_FLAT) {
        // one pass, striped (k_front.h): 10 = 2 tiles per wave, 11 = 4, 12 = 8
        // (16 ran at 3.5-4 TB/s, profiles/r02t_exp_es.log, and is gone)
        unsigned gx;
        switch (variant) {
            case 10: gx = launch_flat_es_any<2>(p->bps, p->coder, nt, st, a); break;
            case 11: gx = launch_flat_es_any<4>(p->bps, p->coder, nt, st, a); break;
            default: gx = launch_flat_es_any<8>(p->bps, p->coder, nt, st, a); break;
        }
        BB_NOTE("k_decode_flat_es<%d,%s,%s,%d> grid %u", p->bps, lv_name(p->bps, p->coder), nt ? "nt" : "plain",
                variant == 10 ? 2 : variant == 11 ? 4 : 8, gx);
        BB_HIP(hipGetLastError());
        return BB_OK;
    }

    if (variant >= 6 && variant <= 9 && om == BB_OUT_FLAT) {
        // explicit write front (k_front.h): 6 = 4 waves x 1 tile, 7 = 4 x 2, 8 = 2 x 4, 9 = 4 x 4
        unsigned gx;
        switch (variant) {
            case 6:  gx = launch_flat_front_any<4, 1>(p->bps, p->coder, nt, st, a); break;
            case 7:  gx = launch_flat_front_any<4, 2>(p->bps, p->coder, nt, st, a); break;
            case 8:  gx = launch_flat_front_any<2, 4>(p->bps, p->coder, nt, st, a); break;
            default: gx = launch_flat_front_any<4, 4>(p->bps, p->coder, nt, st, a); break;
        }
        BB_NOTE("k_decode_flat_front<%d,%s,%s,%s> grid %u G %d K %d", p->bps, lv_name(p->bps, p->coder),
                nt ? "nt" : "plain", variant == 6 ? "4,1" : variant == 7 ? "4,2" : variant == 8 ? "2,4" : "4,4",
                gx, g_tune_front_g.load(), g_tune_front_k.load());
        BB_HIP(hipGetLastError());
        return BB_OK;
    }

    if (variant == 1 && p->bps == 2 && om == BB_OUT_FLAT) {
        const dim3 g2 = capped_grid(nfs, BB_GRID_MAX);
        if (nt) hipLaunchKernelGGL(k_decode_flat2_bytes<true>, g2, dim3(BB_BLOCK), 0, st, a);
        else    hipLaunchKernelGGL(k_decode_flat2_bytes<false>, g2, dim3(BB_BLOCK), 0, st, a);
        BB_NOTE("k_decode_flat2_bytes<%s> grid %u", nt ? "nt" : "plain", g2.x);
        BB_HIP(hipGetLastError());
        return BB_OK;
    }

    // rows kernel or LDS gather for chunks of at least four floats: with the
    // default knob (32) up to four thread slots always gather (one wave per
    // slot leaves the rows kernel with 2-4 waves per workgroup: 5.6 / 6.1 TB/s
    // against 6.4 / 6.3), eight or more only below 32 floats
    // (profiles/r01i_exp_interleave_thr.log)
    // -- and, since the staging rewrite of round 2, 2-bit launches of 64 GiB of
    // output and more whatever the chunk: +1-3.5 % in every cell of 8-64 slots x
    // 32-256 floats at 8 GiB of input (profiles/r02at_exp_rows_vs_gather_2bit_8GiB.log);
    // smaller launches and other sample widths show no clear winner and stay
    const int gchunks = g_tune_gather_chunks.load();
    const bool big2 = p->bps == 2 && p->chunk <= 256 && out_bytes >= (64ull << 30);
    const bool gather_wide = om == BB_OUT_ROWS4
        && (gchunks == 32 ? (p->nslot <= 4 || p->chunk < 32 || big2) : p->chunk < gchunks);
    if ((om == BB_OUT_SCATTER || gather_wide)
        && d_src && variant >= 2
        && (size_t)p->nslot * 528 + 1024 + 64 <= 48 * 1024) {
        // narrow chunks (a thread's sample is less than 128 bytes of output):
        // assemble output rows in LDS (k_gather.h).  Through the rows kernel,
        // whose waves each write their own 16..64-byte pieces of every row,
        // chunks of 4 / 8 / 16 floats ran at 0.55 / 1.15 / 3.45 TB/s
        // (profiles/r01i_exp_interleave.log)
        bb_gather_args ga;
        ga.within = nullptr; ga.nsel = 0; ga.mag_row = ga.mag_sel = 0;
        ga.buf = a.buf; ga.src = d_src; ga.out = d_out; ga.tab = a.tab;
        ga.nframes = nframes; ga.ndw = a.ndw;
        ga.nslot = a.nslot; ga.chunk = a.chunk; ga.lchunk = a.lchunk;
        // bytes staged per work item: 16 KiB, 4 KiB for 1-bit data whose items
        // expand 32-fold (profiles/r01i_exp_interleave_gb.log); knob value 8192 = this default
        size_t gbytes = (size_t)g_tune_gather_bytes.load();
        if (gbytes == 8192) gbytes = p->bps == 1 ? 4096 : 16384;
        uint32_t gt = (uint32_t)(gbytes / ((size_t)p->nslot * 256));
        if (gt < 1) gt = 1;
        if (gt > 32) gt = 32;
        if ((uint64_t)gt > ntiles) gt = (uint32_t)ntiles;
        ga.gtiles = gt;
        ga.ngroup = (uint32_t)((ntiles + gt - 1) / gt);
        ga.fill_re = a.fill_re; ga.fill_im = a.fill_im; ga.complex_data = a.complex_data;
        {
            const uint32_t rl = (uint32_t)p->nslot * (uint32_t)p->chunk;
            ga.lrow = -1;
            if ((rl & (rl - 1)) == 0) ga.lrow = (int32_t)ceil_log2(rl);
        }
        ga.aligned = variant >= 5 ? 1 : 0;
        ga.glds = 0;
        const size_t lds = ((size_t)p->nslot * (gt * 64 + 65) + 2 * p->nslot + 1) * 4 + 1024;
        // persistent grid: a workgroup walks about five work items (8 KiB of
        // payload each); one workgroup per item costs 15 %, a few thousand
        // long-running ones 5-10 % (profiles/r01f_exp_gather*.log)
        ga.perm = make_perm((uint64_t)nframes * ga.ngroup, out_bytes);
        const dim3 gg = capped_grid((uint64_t)nframes * ga.ngroup, BB_GRID_CAP);
        switch (p->bps) {
            case 1: launch_gather<1, BB_LV_REG>(nt, gg, lds, st, ga); break;
            case 2: launch_gather<2, BB_LV_REG>(nt, gg, lds, st, ga); break;
            case 4: launch_gather<4, BB_LV_LDS>(nt, gg, lds, st, ga); break;
            default:
                if (p->coder == BB_CODER_INT) launch_gather<8, BB_LV_INT8>(nt, gg, lds, st, ga);
                else                          launch_gather<8, BB_LV_LDS>(nt, gg, lds, st, ga);
                break;
        }
        BB_NOTE("k_decode_gather<%d,%s,%s,%s> grid %u gtiles %u lds %zu", p->bps, lv_name(p->bps, p->coder),
                nt ? "nt" : "plain", ga.lchunk >= 2 ? "wide" : "narrow", gg.x, ga.gtiles, lds);
        BB_HIP(hipGetLastError());
        return BB_OK;
    }

    if (om == BB_OUT_ROWS4 && variant >= 3) {
        // thread interleave with wide chunks: one wave per thread slot, all
        // waves on the same 8 tiles (k_decode_rows_pipe)
        const int nw = p->nslot >= 8 ? 8 : (p->nslot >= 4 ? 4 : 2);
        const bool aln = variant >= 5;
        const uint64_t seg_max = g_tune_tpw.load() < 8 ? (uint64_t)g_tune_tpw.load() : 8;
        split_tiles(a, ntiles, seg_max, 1);
        const uint64_t sgroups = ((uint64_t)p->nslot + nw - 1) / nw;
        a.perm = make_perm((uint64_t)nframes * a.nseg * sgroups, out_bytes);
        const dim3 g2 = capped_grid((uint64_t)nframes * a.nseg * sgroups, BB_GRID_CAP);
        switch (p->bps) {
            case 1: launch_rows_pipe<1, BB_LV_REG>(nt, aln, nw, g2, st, a); break;
            case 2: launch_rows_pipe<2, BB_LV_REG>(nt, aln, nw, g2, st, a); break;
            case 4: launch_rows_pipe<4, BB_LV_LDS>(nt, aln, nw, g2, st, a); break;
            default:
                if (p->coder == BB_CODER_INT) launch_rows_pipe<8, BB_LV_INT8>(nt, aln, nw, g2, st, a);
                else                          launch_rows_pipe<8, BB_LV_LDS>(nt, aln, nw, g2, st, a);
                break;
        }
        BB_NOTE("k_decode_rows_pipe<%d,%s,%s,%d,8,%s> grid %u", p->bps, lv_name(p->bps, p->coder),
                nt ? "nt" : "plain", nw, aln ? "aligned" : "plain-loads", g2.x);
        BB_HIP(hipGetLastError());
        return BB_OK;
    }

    if (om == BB_OUT_FLAT && variant == 4 && a.ndw >= 64 * 16) {
        // contiguous output: cut the work in output space (k_decode_flat_span),
        // 2 waves x 16 tiles per item whatever the frame size
        const uint64_t tiles_all = (nfs * a.ndw + 63) / 64;
        const dim3 g2 = capped_grid((tiles_all + 31) / 32, BB_GRID_CAP);
        switch (p->bps) {
            case 1: launch_flat_span<1, BB_LV_REG>(nt, g2, st, a); break;
            case 2: launch_flat_span<2, BB_LV_REG>(nt, g2, st, a); break;
            case 4: launch_flat_span<4, BB_LV_LDS>(nt, g2, st, a); break;
            default:
                if (p->coder == BB_CODER_INT) launch_flat_span<8, BB_LV_INT8>(nt, g2, st, a);
                else                          launch_flat_span<8, BB_LV_LDS>(nt, g2, st, a);
                break;
        }
        BB_NOTE("k_decode_flat_span<%d,%s,%s,2,16> grid %u", p->bps, lv_name(p->bps, p->coder),
                nt ? "nt" : "plain", g2.x);
        BB_HIP(hipGetLastError());
        return BB_OK;
    }

    if (variant >= 2) {
        // persistent pipelined form.  Geometry (waves per workgroup x tiles
        // per wave) is chosen so that a wave writes a long contiguous run:
        // 2 waves x up to 12 tiles (an 8000-byte payload becomes two items of
        // 2 x 8 tiles = 32 KiB runs; with the large grid that beats 2 x 16 by
        // 1.5 %, profiles/r01g_exp_tpw.log).  Variant 2 keeps the
        // 4 x 8 geometry; 2 x 32 tiles was tried for 8-bit data and lost 27 %.
        const bool wide = variant >= 3;
        const int nw = wide ? 2 : 4;
        const bool aln = wide && om == BB_OUT_FLAT && variant == 5;
        const int tpw8 = g_tune_tpw8.load();
        const bool long8 = aln && p->bps == 8 && tpw8 > 16;
        // the byte table kernel (1-, 2- and 4-bit contiguous output) is at its best
        // with SHORT work items, one per workgroup: 2 waves x 4 tiles (2 KiB
        // in, 32 KiB out) on an uncapped grid, +2-4 % over 2 x 8-12 tiles on
        // 131072 persistent workgroups at every size from 2 to 8 GiB, for
        // 8000-, 8192- and 10000-byte payloads (profiles/r02ao_exp_tpw_grid*.log)
        // -- many small workgroups in flight again overlap loads and stores
        // better than a register pipeline, as for the 8-bit kernels
        const bool lut = aln && p->bps <= 4 && g_tune_byte_lut.load() != 0;
        // (what counts is the OUTPUT of a work item, 32 KiB: 2 / 4 / 8 tiles per
        // wave for 1- / 2- / 4-bit samples -- 1-bit 6.58 -> 6.86 TB/s against 4
        // tiles, 4-bit 5.28 -> 6.62 and +7 % over the plain kernel it used before,
        // profiles/r02ar_exp_1bit_items.log, r02ar_exp_4bit_lut.log)
        int lut_tiles = (g_tune_lut_tpw.load() ? g_tune_lut_tpw.load() : 4) * p->bps / 2;
        lut_tiles = lut_tiles < 1 ? 1 : lut_tiles > 16 ? 16 : lut_tiles;
        const int tpw_max = long8 ? (tpw8 > 32 ? 32 : tpw8) : lut ? lut_tiles
                            : wide ? g_tune_tpw.load() : 8;
        const uint64_t seg_max = (uint64_t)nw * tpw_max;
        split_tiles(a, ntiles, seg_max, nw);
        a.perm = make_perm(nfs * a.nseg, out_bytes);
        const dim3 g2 = capped_grid(nfs * a.nseg, lut ? BB_GRID_SHORT_ITEMS : (uint64_t)(wide ? BB_GRID_CAP : 4096));
        if (!wide) {
            switch (p->bps) {
                case 1: launch_flat_pipe<1, BB_LV_REG, 4, 8>(om, nt, g2, st, a); break;
                case 2: launch_flat_pipe<2, BB_LV_REG, 4, 8>(om, nt, g2, st, a); break;
                case 4: launch_flat_pipe<4, BB_LV_LDS, 4, 8>(om, nt, g2, st, a); break;
                default:
                    if (p->coder == BB_CODER_INT) launch_flat_pipe<8, BB_LV_INT8, 4, 8>(om, nt, g2, st, a);
                    else                          launch_flat_pipe<8, BB_LV_LDS, 4, 8>(om, nt, g2, st, a);
                    break;
            }
        } else if (long8) {
            if (p->coder == BB_CODER_INT) launch_flat_aln32<8, BB_LV_INT8>(nt, g2, st, a);
            else                          launch_flat_aln32<8, BB_LV_LDS>(nt, g2, st, a);
        } else if (lut) {
            // byte table in LDS instead of the register level select (k_lut.h)
            if (p->bps == 1) launch_flat_lut<1>(nt, g2, st, a);
            else if (p->bps == 2) launch_flat_lut<2>(nt, g2, st, a);
            else launch_flat_lut<4>(nt, g2, st, a);
            BB_NOTE("k_decode_flat_lut<%d,%s,2,%d> grid %u tiles/wave %u", p->bps, nt ? "nt" : "plain",
                    (a.tpw <= 4 && g_tune_lut_small.load() != 0) ? 4 : 16, g2.x, a.tpw);
            BB_HIP(hipGetLastError());
            return BB_OK;
        } else if (aln) {
            // aligned 256-byte block loads (k_decode_flat_aln)
            switch (p->bps) {
                case 1: launch_flat_aln<1, BB_LV_REG>(nt, g2, st, a); break;
                case 2: launch_flat_aln<2, BB_LV_REG>(nt, g2, st, a); break;
                case 4: launch_flat_aln<4, BB_LV_LDS>(nt, g2, st, a); break;
                default:
                    if (p->coder == BB_CODER_INT) launch_flat_aln<8, BB_LV_INT8>(nt, g2, st, a);
                    else                          launch_flat_aln<8, BB_LV_LDS>(nt, g2, st, a);
                    break;
            }
        } else {
            switch (p->bps) {
                case 1: launch_flat_pipe<1, BB_LV_REG, 2, 16>(om, nt, g2, st, a); break;
                case 2: launch_flat_pipe<2, BB_LV_REG, 2, 16>(om, nt, g2, st, a); break;
                case 4: launch_flat_pipe<4, BB_LV_LDS, 2, 16>(om, nt, g2, st, a); break;
                default:
                    if (p->coder == BB_CODER_INT) launch_flat_pipe<8, BB_LV_INT8, 2, 16>(om, nt, g2, st, a);
                    else                          launch_flat_pipe<8, BB_LV_LDS, 2, 16>(om, nt, g2, st, a);
                    break;
            }
        }
        BB_NOTE("%s<%d,%s,%s,%d,%d> out-mode %d grid %u tiles/wave %u",
                !wide ? "k_decode_flat_pipe" : (long8 || aln) ? "k_decode_flat_aln" : "k_decode_flat_pipe",
                p->bps, lv_name(p->bps, p->coder), nt ? "nt" : "plain", nw, long8 ? 32 : wide ? 16 : 8,
                om, g2.x, a.tpw);
        BB_HIP(hipGetLastError());
        return BB_OK;
    }

    switch (p->bps) {
        case 1: launch_flat<1, BB_LV_REG>(om, nt, grid, st, a); break;
        case 2: launch_flat<2, BB_LV_REG>(om, nt, grid, st, a); break;
        case 4: launch_flat<4, BB_LV_LDS>(om, nt, grid, st, a); break;
        case 8:
            if (p->coder == BB_CODER_INT) launch_flat<8, BB_LV_INT8>(om, nt, grid, st, a);
            else                          launch_flat<8, BB_LV_LDS>(om, nt, grid, st, a);
            break;
        default: return BB_ENOTSUP;
    }
    BB_NOTE("k_decode_flat<%d,%s,%d,%s> grid %u", p->bps, lv_name(p->bps, p->coder), om,
            nt ? "nt" : "plain", grid.x);
    BB_HIP(hipGetLastError());
    return BB_OK;
}

} // namespace expd
