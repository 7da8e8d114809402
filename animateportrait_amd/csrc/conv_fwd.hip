// conv_fwd.hip -- the forward launch of the convolution operator: one launcher per kernel family and the ap_conv2d_fwd* entry
// points.  Every entry point plans the layer (conv_plan.h), refuses what the plan or the arguments rule out, then launches.
// The APAMD_VARIANTS (`make variants`) and APAMD_ABLATION (`make ablate`) hooks of the forward side live here.
#include "conv_plan.h"
#include "conv_direct.h"
#include "conv_tapgemm.h"   // TapGemmCfg / TapGemmParams; the kernel itself is instantiated in conv_tapgemm_inst.hip
#include "conv_small.h"
#include "conv_head.h"      // conv_head_fwd_kernel (its weight gradient: wgrad_edge_host.hip; kHeadMaxW: conv_plan.hip)
#include "conv_tsmall.h"

#include <cstdlib>
#include <cstring>
#include <string>

namespace apamd {

#ifdef APAMD_VARIANTS
const void* bf3_sb_kernel(size_t* lds_bytes);     // tools/variants/conv_bf3_sb.hip
#endif

static const int kDirectCops[] = {1, 4};     // the instantiations of conv_direct_f32<DirectCfg<7, cop>>
static const void* direct_fn(int K, int cop) {
    if (K == 7 && cop == 1) return reinterpret_cast<const void*>(&conv_direct_f32<DirectCfg<7, 1>>);
    if (K == 7 && cop == 4) return reinterpret_cast<const void*>(&conv_direct_f32<DirectCfg<7, 4>>);
    return nullptr;
}
static size_t direct_lds_bytes(int K, int cop, int nbuf, int cin_pad) {
    if (cop == 1) return 4 * DirectCfg<7, 1>::lds_floats(nbuf, cin_pad);
    return 4 * DirectCfg<7, 4>::lds_floats(nbuf, cin_pad);
}

// ------------------------------------------------------------------ the forward launch
// How the result is stored; the default is the whole NCHW fp32 tensor.
struct OutForm {
    const ap_out_view* view = nullptr;   // a window of the output, with the caller's strides
    bool octet = false;                  // channel-octet layout y[n][Cout/8][OH*OW][8]
    bool bf16 = false;                   // bf16 values
};

struct FwdArgs {
    const float *packed, *bias;
    float *y, *stats;    // stats: per-tile partial sums for the consumer's InstanceNorm, or null
    hipStream_t stream;
};

// Every refusal that depends on the arguments, before anything is launched; callers tell the refusals apart, so the order stays.
// a == null (ap_conv2d_fwd_route): the data pointers are taken as given, everything else is checked as for a launch
static int check_fwd_args(const ap_conv_desc* d, const Plan& pl, const OutForm& o, const FwdArgs* a) {
    if (o.bf16 && (!ob16_plan_ok(d, pl) || o.octet))
        return fail(AP_ERR_UNSUPPORTED, "conv2d_fwd_bf16out: only the plain-bf16 dense 3x3 stride-1 layers store bf16 (ap_conv2d_bf16out_ok)");
    if (a && (!a->packed || !a->y)) return fail(AP_ERR_INVALID, "null packed/y pointer");
    if (o.octet && !octet_plan_ok(d, pl))
        return fail(AP_ERR_UNSUPPORTED, "conv2d_fwd_octet: only single-launch split-bf16 layers of the run-time-tap / row kernel "
                                        "families with Cout %% 8 == 0 write the channel-octet layout (ap_conv2d_octet_ok)");
    if (o.view) {
        if (!pl.bf3 || pl.fused_phases || pl.launches.size() != 1)
            return fail(AP_ERR_UNSUPPORTED, "conv2d_fwd_view: only single-launch split-bf16 plans take an output window");
        if (o.view->OH < 1 || o.view->OW < 1 || o.view->OH > pl.Hout || o.view->OW > pl.Wout)
            return fail(AP_ERR_INVALID, "conv2d_fwd_view: window %dx%d outside the %dx%d output", o.view->OH, o.view->OW, pl.Hout, pl.Wout);
    }
    if (d->presplit && !pl.bf3) return fail(AP_ERR_INVALID, "desc.presplit set for a layer that does not take split sources");
    for (int s = 0; s < d->nsrc; ++s) {
        if (a && !d->src[s].data) return fail(AP_ERR_INVALID, "segment %d: null data", s);
        if ((d->src[s].mean == nullptr) != (d->src[s].rstd == nullptr))
            return fail(AP_ERR_INVALID, "segment %d: mean and rstd must be given together", s);
        if (d->src[s].act < 0 || d->src[s].act > 2) return fail(AP_ERR_INVALID, "segment %d: act %d", s, d->src[s].act);
    }
    return AP_OK;
}

// conv_tsmall_f32<CO> is instantiated for these output widths; a layer runs on the narrowest one that holds its channels
static const int kTSmallCouts[] = {1, 2, 4};
static int tsmall_inst(int Cout) {
    for (int c : kTSmallCouts)
        if (Cout <= c) return c;
    return 0;
}

static int tsmall_grid_ok(const ap_conv_desc* d) {
    if (d->N > 65535 || (d->H + 7) / 8 > 65535) return fail(AP_ERR_UNSUPPORTED, "conv_tsmall: grid too large");
    return AP_OK;
}

static int launch_tsmall(const ap_conv_desc* d, const Plan& pl, const FwdArgs& a) {
    TSmallParams p;
    memset(&p, 0, sizeof(p));
    fill_seg(p.src, d->src[0], 0);
    p.N = d->N; p.C = pl.Cin; p.H = d->H; p.W = d->W; p.Cout = d->Cout;
    p.w = a.packed + pl.head_w_off; p.bias = a.bias; p.act = d->act; p.y = a.y;
    if (int rc = tsmall_grid_ok(d)) return rc;
    const dim3 grid((d->W + 31) / 32, (d->H + 7) / 8, d->N);
    switch (tsmall_inst(d->Cout)) {
        case 1: hipLaunchKernelGGL((conv_tsmall_f32<1>), grid, dim3(256), 0, a.stream, p); break;
        case 2: hipLaunchKernelGGL((conv_tsmall_f32<2>), grid, dim3(256), 0, a.stream, p); break;
        default: hipLaunchKernelGGL((conv_tsmall_f32<4>), grid, dim3(256), 0, a.stream, p); break;
    }
    return check_launch("conv_tsmall_f32");
}

// Rows per workgroup of the head kernel.  The kernel is bound by its vector ALUs (normalisation, activation, three wave shifts and
// 16 FMAs per staged row element, on RB + 3 rows for RB outputs) and a launch is a few hundred 1024-thread workgroups: what counts
// is the number of workgroup ROUNDS on the CUs times the rows a workgroup stages.  (Round 6; before: 3-row bands unless taller
// ones still gave >= 200 workgroups -- 320 workgroups = two rounds at 2B = 32, 160 = 5/8 of the chip at B = 16.)
static const int kHeadRows[] = {2, 3, 4, 5, 6, 10};      // the instantiations of conv_head_fwd_kernel<RB>
static int head_rows(int N, int Hout) {
    const int cus = num_cus();
    int rb = 3;
    long long best_cost = -1;
    for (int cand : kHeadRows) {
        const long long wgs = (long long)N * ((Hout + cand - 1) / cand);
        const long long cost = ((wgs + cus - 1) / cus) * (cand + 3);
        if (best_cost < 0 || cost < best_cost) { rb = cand; best_cost = cost; }
    }
    return rb;
}

static int launch_head(const ap_conv_desc* d, const Plan& pl, const FwdArgs& a) {
    const int rb = head_rows(d->N, pl.Hout);
    HeadParams p;
    memset(&p, 0, sizeof(p));
    fill_seg(p.src, d->src[0], 0);
    p.N = d->N; p.C = pl.Cin; p.H = d->H; p.W = d->W; p.OH = pl.Hout; p.OW = pl.Wout;
    p.w = a.packed + pl.head_w_off; p.bias = a.bias; p.act = d->act; p.y = a.y;
    const dim3 hg(d->N, (pl.Hout + rb - 1) / rb);
    switch (rb) {
        case 2: hipLaunchKernelGGL(conv_head_fwd_kernel<2>, hg, dim3(1024), 0, a.stream, p); break;
        case 4: hipLaunchKernelGGL(conv_head_fwd_kernel<4>, hg, dim3(1024), 0, a.stream, p); break;
        case 5: hipLaunchKernelGGL(conv_head_fwd_kernel<5>, hg, dim3(1024), 0, a.stream, p); break;
        case 6: hipLaunchKernelGGL(conv_head_fwd_kernel<6>, hg, dim3(1024), 0, a.stream, p); break;
        case 10: hipLaunchKernelGGL(conv_head_fwd_kernel<10>, hg, dim3(1024), 0, a.stream, p); break;
        default: hipLaunchKernelGGL(conv_head_fwd_kernel<3>, hg, dim3(1024), 0, a.stream, p); break;
    }
    return check_launch("conv_head_fwd_kernel");
}

// the instantiations of the narrow 3x3 kernels: {stride, Cout}; stride 1 stages its tile in LDS (conv_small_f32), stride 2 gathers
// (conv_small_gather_f32)
static const int kSmallCfgs[][2] = {{1, 8}, {1, 16}, {2, 8}, {2, 16}};
static bool small_gathers(int stride) { return stride != 1; }

static int launch_small(const ap_conv_desc* d, const Plan& pl, const FwdArgs& a) {
    SmallKParams p;
    memset(&p, 0, sizeof(p));
    fill_seg(p.src, d->src[0], 0);
    p.N = d->N; p.H = d->H; p.W = d->W; p.Cin = pl.Cin; p.Cout = d->Cout; p.OH = pl.Hout; p.OW = pl.Wout;
    p.pad = d->pad; p.pad_mode = d->pad_mode;
    p.y = a.y; p.w = a.packed; p.bias = a.bias; p.act = d->act;
    p.stats = a.stats; p.stat_tiles = pl.stat_tiles;
    p.tiles_x = (pl.Wout + 31) / 32; p.tiles_y = (pl.Hout + 7) / 8;
    const dim3 grid((unsigned)((long long)d->N * p.tiles_y * p.tiles_x));
    if (!small_gathers(d->stride) && d->Cout == 8) hipLaunchKernelGGL((conv_small_f32<SmallCfg<1, 8>>), grid, dim3(256), 0, a.stream, p);
    else if (!small_gathers(d->stride)) hipLaunchKernelGGL((conv_small_f32<SmallCfg<1, 16>>), grid, dim3(256), 0, a.stream, p);
    else if (d->Cout == 8) hipLaunchKernelGGL((conv_small_gather_f32<SmallCfg<2, 8>>), grid, dim3(256), 0, a.stream, p);
    else hipLaunchKernelGGL((conv_small_gather_f32<SmallCfg<2, 16>>), grid, dim3(256), 0, a.stream, p);
    return check_launch("conv_small_f32");
}

// The generator's output layer in split-bf16 arithmetic -- one reflection-padded 64-channel source, one output channel, no
// statistics epilogue -- multiplies on the matrix pipe (conv_tapgemm.h).  Same plan, same packed image: chosen here, at launch.
static bool tapgemm_serves(const ap_conv_desc* d, const Plan& pl, bool with_stats) {
    return d->precision == AP_PRECISION_BF16X3 && d->Cout == 1 && d->KH == 7 && d->nsrc == 1 && d->src[0].C == TapGemmCfg::C &&
           d->pad_mode == AP_PAD_REFLECT && !with_stats && pl.cin_pad == TapGemmCfg::C;
}

// Tile height: the workgroups (two per CU) run in rounds, and a workgroup stages th + 6 rows for th output rows
static int tapgemm_tiles_x(const Plan& pl) { return (pl.Wout + TapGemmCfg::TW - 1) / TapGemmCfg::TW; }
static int tapgemm_band(int N, int Hout, int tiles_x) {
    const long long slots = 2LL * num_cus();
    long long best_cost = -1;
    int best = Hout;
    for (int ty = 1; ty <= (Hout + 7) / 8; ++ty) {
        const int th = (Hout + ty - 1) / ty;
        const long long wgs = (long long)N * tiles_x * ((Hout + th - 1) / th);
        const long long cost = ((wgs + slots - 1) / slots) * (th + 6);
        if (best_cost < 0 || cost < best_cost) { best = th; best_cost = cost; }
    }
    return best;
}

static int launch_tapgemm(const ap_conv_desc* d, const Plan& pl, const FwdArgs& a) {
    const void* kfn = tapgemm_kernel();
    int rc = ensure_dyn_lds(kfn, 160 * 1024);
    if (rc) return rc;
    TapGemmParams p;
    memset(&p, 0, sizeof(p));
    fill_seg(p.seg, d->src[0], 0);
    p.N = d->N; p.H = d->H; p.W = d->W;
    p.y = a.y; p.wp = a.packed; p.bias = a.bias; p.act = d->act;
    p.tiles_x = tapgemm_tiles_x(pl);
    p.th = tapgemm_band(d->N, pl.Hout, p.tiles_x);
    p.tiles_y = (pl.Hout + p.th - 1) / p.th;
    void* args[] = {&p};
    hipError_t e = hipLaunchKernel(kfn, dim3((unsigned)(d->N * p.tiles_y * p.tiles_x)), dim3(256), args, TapGemmCfg::lds_bytes(), a.stream);
    if (e != hipSuccess) return fail(AP_ERR_LAUNCH, "conv_tapgemm_bf16x3 launch: %s", hipGetErrorString(e));
    return AP_OK;
}

static int launch_direct(const ap_conv_desc* d, const Plan& pl, const FwdArgs& a) {
    const void* kfn = direct_fn(d->KH, pl.direct_cop);
    int rc = ensure_dyn_lds(kfn, 160 * 1024);
    if (rc) return rc;
    DirectKParams p;
    memset(&p, 0, sizeof(p));
    p.nseg = d->nsrc;
    for (int s = 0; s < d->nsrc; ++s) fill_seg(p.seg[s], d->src[s], pl.chunk_begin[s]);
    p.N = d->N; p.H = d->H; p.W = d->W; p.Cout = d->Cout; p.OH = pl.Hout; p.OW = pl.Wout;
    p.pad = d->pad; p.pad_mode = d->pad_mode;
    p.y = a.y; p.wp = a.packed; p.bias = a.bias; p.act = d->act;
    p.stats = a.stats; p.stat_tiles = pl.stat_tiles;
    p.nchunks = pl.nchunks; p.cin_pad = pl.cin_pad;
    p.tiles_x = (pl.Wout + 63) / 64; p.tiles_y = (pl.Hout + 15) / 16;
    const size_t lds = direct_lds_bytes(d->KH, pl.direct_cop, p.nchunks > 1 ? 2 : 1, p.cin_pad);
    void* args[] = {&p};
    hipError_t e = hipLaunchKernel(kfn, dim3((unsigned)(d->N * p.tiles_y * p.tiles_x)), dim3(256), args, lds, a.stream);
    if (e != hipSuccess) return fail(AP_ERR_LAUNCH, "conv_direct_f32 launch: %s", hipGetErrorString(e));
    return AP_OK;
}

// what the fp32 implicit-GEMM and the split-bf16 kernel take alike for launch L (with_norm = false: sources are split copies)
static ConvKParams conv_params(const ap_conv_desc* d, const Plan& pl, const Launch& L, const FwdArgs& a, bool with_norm) {
    ConvKParams p;
    memset(&p, 0, sizeof(p));
    p.nseg = d->nsrc;
    for (int s = 0; s < d->nsrc; ++s) fill_seg(p.seg[s], d->src[s], pl.chunk_begin[s], with_norm);
    p.N = d->N; p.H = d->H; p.W = d->W; p.Cout = d->Cout;
    p.OH = L.OH; p.OW = L.OW; p.dy0 = L.dy0; p.dx0 = L.dx0;
    p.pad_mode = d->pad_mode; p.y = a.y;
    p.o_nstride = (long long)d->Cout * pl.Hout * pl.Wout; p.o_cstride = (long long)pl.Hout * pl.Wout; p.o_rstride = pl.Wout;
    p.osy = L.osy; p.osx = L.osx; p.oy_off = L.oy_off; p.ox_off = L.ox_off;
    p.wp = a.packed + L.wp_off; p.bias = a.bias; p.act = d->act;
    p.stats = a.stats; p.stat_tiles = pl.stat_tiles; p.stat_tile_off = L.stat_tile_off;
    p.ntaps = (int)L.taps.size(); p.nchunks = pl.nchunks;
    p.tiles_x = L.tiles_x; p.tiles_y = L.tiles_y; p.co_tiles = pl.co_tiles;
    p.cin_pad = pl.cin_pad;
#ifdef APAMD_ABLATION
    p.ablate = sw(SW_ABLATE);
#endif
    return p;
}

// ConvKParams.tap_bits of a run-time-tap kernel (K == 0, at most 4 taps in a 2 x 2 window): bit 2t = ly, bit 2t+1 = lx of tap t
static int tap_bits(const Launch& L, unsigned& bits) {
    const int ntaps = (int)L.taps.size();
    if (ntaps > 4) return fail(AP_ERR_UNSUPPORTED, "phase with %d taps", ntaps);
    bits = 0;
    for (int t = 0; t < ntaps; ++t) bits |= (unsigned)((L.taps[t].ly & 1) | ((L.taps[t].lx & 1) << 1)) << (2 * t);
    return AP_OK;
}

// what launch L of an implicit-GEMM plan cannot be; bits: ConvKParams.tap_bits of a run-time-tap kernel
static int igemm_launch_ok(const ap_conv_desc* d, const Plan& pl, const Launch& L, unsigned& bits) {
    int rc;
    bits = 0;
    if (pl.k->K == 0 && (rc = tap_bits(L, bits))) return rc;
    if ((long long)d->N * L.tiles_y * L.tiles_x * pl.co_tiles > 0x7fffffffLL) return fail(AP_ERR_UNSUPPORTED, "grid too large");
    return AP_OK;
}

static int launch_igemm(const ap_conv_desc* d, const Plan& pl, const FwdArgs& a) {
    int rc = ensure_dyn_lds(pl.k->fn, 160 * 1024);
    if (rc) return rc;
    for (const auto& L : pl.launches) {
        ConvKParams p = conv_params(d, pl, L, a, true);
        p.wfloats = pl.k->wfloats(p.ntaps);
        if ((rc = igemm_launch_ok(d, pl, L, p.tap_bits))) return rc;
        const size_t lds = 4 * pl.k->lds_floats(p.ntaps, p.nchunks > 1 ? 2 : 1, p.cin_pad);
        const long long nblk = (long long)d->N * L.tiles_y * L.tiles_x * pl.co_tiles;
        void* args[] = {&p};
        hipError_t e = hipLaunchKernel(pl.k->fn, dim3((unsigned)nblk), dim3(256), args, lds, a.stream);
        if (e != hipSuccess) return fail(AP_ERR_LAUNCH, "conv_igemm_f32 launch: %s", hipGetErrorString(e));
    }
    return AP_OK;
}

// ---- split-bf16 launches
// bit t of the result: tap t of the 2 x 2 window exists in this phase of a fused launch
static unsigned phase_tapmask(const Launch& L) {
    unsigned m = 0;
    for (size_t t = 0; t < L.taps.size() && t < 4; ++t)
        if (L.taps[t].ky >= 0) m |= 1u << t;
    return m;
}

// conv_ph4 walks cout tiles only and derives the phase geometry from K: check the plan agrees
static int check_ph4_plan(const Plan& pl, const ap_out_view* view) {
    if (view) return fail(AP_ERR_UNSUPPORTED, "conv_ph4: output views are not supported");
    // (the kernel folds the phase into 32-bit per-lane byte offsets of the packed weights)
    const int wfloats = pl.bk->wfloats((int)pl.launches[0].taps.size());
    if (3LL * pl.co_tiles * pl.nchunks * wfloats * 4 >= (1LL << 31))
        return fail(AP_ERR_UNSUPPORTED, "conv_ph4: packed phase blocks of %d cout tiles x %d chunks are too large", pl.co_tiles, pl.nchunks);
    const int base = pl.ph4 == 3 ? 0 : -1;
    for (int ph = 0; ph < 4; ++ph) {
        const Launch& Lp = pl.launches[ph];
        const unsigned want = (pl.ph4 == 3 && !(ph >> 1)) ? 1u : 3u;          // taps along y
        const unsigned wanx = (pl.ph4 == 3 && !(ph & 1)) ? 1u : 3u;
        unsigned m = 0;
        for (int t = 0; t < 4; ++t) if (((want >> (t >> 1)) & 1u) && ((wanx >> (t & 1)) & 1u)) m |= 1u << t;
        const int oy = pl.ph4 == 3 ? 0 : (ph >> 1), ox = pl.ph4 == 3 ? 0 : (ph & 1);
        const unsigned have = phase_tapmask(Lp);
        if (have != m || Lp.dy0 != base + oy || Lp.dx0 != base + ox || Lp.oy_off != (ph >> 1) || Lp.ox_off != (ph & 1) ||
            Lp.osy != 2 || Lp.osx != 2 || Lp.OH != pl.launches[0].OH || Lp.OW != pl.launches[0].OW)
            return fail(AP_ERR_UNSUPPORTED, "conv_ph4: phase %d geometry (taps %x/%x, origin %d,%d)", ph, have, m, Lp.dy0, Lp.dx0);
    }
    return AP_OK;
}

// one launch (phase 0's geometry) covers the four phases: their weight blocks follow each other in the packed image, so the
// virtual cout tile indexes them directly (conv_ph4 walks the real cout tiles)
static int launch_co_tiles(const Plan& pl) { return pl.fused_phases && !pl.ph4 ? 4 * pl.co_tiles : pl.co_tiles; }
static void fused_phase_params(ConvKParams& p, const Plan& pl) {
    p.nphase = 4;
    p.co_tiles_phase = pl.co_tiles;
    p.co_tiles = launch_co_tiles(pl);
    for (int ph = 0; ph < 4; ++ph) {
        const Launch& Lp = pl.launches[ph];
        p.ph_dy0[ph] = Lp.dy0; p.ph_dx0[ph] = Lp.dx0; p.ph_oy[ph] = Lp.oy_off; p.ph_ox[ph] = Lp.ox_off;
        p.ph_stat[ph] = Lp.stat_tile_off;
        p.ph_tapmask[ph] = phase_tapmask(Lp);
    }
}

// space-to-depth form of a 3x3 stride-2 layer: input phase (ry, rx) = 16-channel chunks [r C/16, (r+1) C/16)
static int s2d3_div(const ap_conv_desc* d, const Plan& pl) {
    if (d->s2d_k != 3 || d->transposed || pl.bk->K != 0 || d->KW != 2 || d->nsrc != 1 || d->src[0].C % 64 != 0) return 0;
    return d->src[0].C / 64;
}
static void s2d3_params(ConvKParams& p, int div) {
    if (div <= 0) return;
    p.s2d_div = div;
    for (int r = 0; r < 4; ++r) {
        p.s2d_mask[r] = 0;
        for (int t = 0; t < 4; ++t)
            if (2 * (t >> 1) + (r >> 1) <= 2 && 2 * (t & 1) + (r & 1) <= 2) p.s2d_mask[r] |= 1u << t;
    }
}

// persistent workgroups, each walks its share of the tiles: one per CU, two when two stage sets fit its 160 KB of LDS
static unsigned bf3_workgroups(long long tiles, size_t lds, bool two_per_cu) {
    int cus = num_cus() * ((2 * lds <= 160 * 1024 || two_per_cu) ? 2 : 1);
    if (const int forced = sw(SW_BF3_BLOCKS)) {      // tuning / test knob: never silent
        static bool told = false;
        if (!told) fprintf(stderr, "libapamd: APAMD_BF3_BLOCKS=%d overrides the persistent workgroup count\n", forced);
        told = true;
        cus = forced;
    }
    return (unsigned)(tiles > cus ? cus : tiles);
}

// What one split-bf16 launch runs: decided here for the launcher and for ap_conv2d_fwd_route alike
struct Bf3Launch {
    const Bf3Kernel* kern;
    const void* kfn;
    bool s2d3_ct;          // kfn is the instantiation with the compile-time tap sets of a space-to-depth 3x3 layer
    int s2d_div;           // > 0: space-to-depth 3x3 layer, C / 64 chunks per input phase
    unsigned tap_bits;
    int tiles_x, tiles_y, co_tiles;
    size_t lds;
};

static int bf3_choose(const ap_conv_desc* d, const Plan& pl, const OutForm& o, const Launch& L, Bf3Launch& c) {
    const int ntaps = (int)L.taps.size();
    c.kern = pl.ph4 ? pl.bk : bf3_for_taps(pl.bk, ntaps);
    if (!c.kern) return fail(AP_ERR_UNSUPPORTED, "no split-bf16 kernel for a phase with %d taps", ntaps);
    c.tiles_x = L.tiles_x; c.tiles_y = L.tiles_y;
    if (const ap_out_view* v = o.view) {
        c.tiles_x = (v->OW + 31) / 32;
        c.tiles_y = (v->OH + pl.bk->TH - 1) / pl.bk->TH;
    }
    c.co_tiles = launch_co_tiles(pl);
    c.s2d_div = s2d3_div(d, pl);
    c.tap_bits = 0;
    int rc;
    if (pl.bk->K == 0 && (rc = tap_bits(L, c.tap_bits))) return rc;
    c.kfn = o.bf16 ? c.kern->fn1_ob16 : c.kern->kernel(d->precision);
    // even chunk count per input phase: the instantiation with compile-time tap sets (no fragment reads for absent taps)
    c.s2d3_ct = c.s2d_div > 0 && (c.s2d_div & 1) == 0 && pl.nchunks == 4 * c.s2d_div && c.kern->kernel_s2d3(d->precision);
    if (c.s2d3_ct) c.kfn = c.kern->kernel_s2d3(d->precision);
    c.lds = c.kern->lds(d->precision, ntaps);
    return AP_OK;
}

// what the split-bf16 pipeline cannot take, whatever the kernel (lds: with whatever a hook added)
static int bf3_fits(const ap_conv_desc* d, const Plan& pl, size_t lds) {
    if (lds > 160 * 1024) return fail(AP_ERR_UNSUPPORTED, "bf16x3 LDS tile of %zu bytes does not fit", lds);
    if (pl.nchunks < 2) return fail(AP_ERR_UNSUPPORTED, "bf16x3 pipeline needs >= 32 input channels");
    if (((long long)d->H * d->W + 1) * 32 >= (1LL << 31))   // per-lane DMA offsets span two channel-group planes
        return fail(AP_ERR_UNSUPPORTED, "split-bf16 path: %d x %d planes are too large", d->H, d->W);
    return AP_OK;
}

// the launches of a split-bf16 plan, in order: each(L, c) launches or describes one; a fused plan has one for its four phases
template <class Each>
static int bf3_launches(const ap_conv_desc* d, const Plan& pl, const OutForm& o, Each&& each) {
    if (!d->presplit)
        return fail(AP_ERR_INVALID, "this layer runs on the split-bf16 path: pass sources prepared by "
                                    "ap_split_prepass and set desc.presplit (see ap_conv2d_wants_presplit)");
    int rc = pl.ph4 ? check_ph4_plan(pl, o.view) : AP_OK;
    if (rc) return rc;
    for (const auto& L : pl.launches) {
        Bf3Launch c;
        if ((rc = bf3_choose(d, pl, o, L, c)) || (rc = each(L, c))) return rc;
        if (pl.fused_phases) break;
    }
    return AP_OK;
}

static int launch_bf3(const ap_conv_desc* d, const Plan& pl, const OutForm& o, const FwdArgs& a) {
    return bf3_launches(d, pl, o, [&](const Launch& L, const Bf3Launch& c) -> int {
        ConvKParams p = conv_params(d, pl, L, a, false);
        p.wfloats = pl.bk->wfloats(p.ntaps);
        p.o_octet = o.octet ? 1 : 0;
        if (const ap_out_view* v = o.view) {
            // output window: a sub-grid of the output, stored with the caller's strides (ap_out_view)
            p.OH = v->OH; p.OW = v->OW;
            p.o_nstride = v->nstride; p.o_cstride = v->cstride; p.o_rstride = v->rstride;
            p.osy = 1; p.oy_off = v->y_off;
            p.osx = v->xstride; p.ox_off = v->x_off * v->xstride;
        }
        p.tiles_x = c.tiles_x; p.tiles_y = c.tiles_y;
        if (pl.fused_phases) fused_phase_params(p, pl);
        s2d3_params(p, c.s2d_div);
        p.tap_bits = c.tap_bits;
        const void* kfn = c.kfn;
        int rc = ensure_dyn_lds(kfn, 160 * 1024);
        if (rc) return rc;
        size_t lds = c.lds;
        bool sb = false;
#ifdef APAMD_VARIANTS
        if (!o.view && !o.octet && c.kern->K == 3 && c.kern->S == 1 && c.kern->TH == 16 && !c.kern->ROW && d->precision != AP_PRECISION_BF16 &&
            p.osx == 1 && p.osy == 1 && p.oy_off == 0 && p.ox_off == 0 && sw(SW_CONV_SB)) {
            // rejected experiment kept for A/B (tools/variants/conv_bf16x3_sb.h, `make variants`): one LDS stage per
            // workgroup, two workgroups per CU
            kfn = bf3_sb_kernel(&lds);
            rc = ensure_dyn_lds(kfn, 160 * 1024);
            if (rc) return rc;
            p.sb_skew = sw(SW_CONV_SB_SKEW);
            sb = true;
        }
#endif
#ifdef APAMD_ABLATION
        // cycle account (tools/cycle_account.py): APAMD_STAMP_BUF = device address of the stamp buffer, APAMD_STAMP_WORDS =
        // dwords per wave; the stamps live in LDS behind the stage buffers, so only kernels that leave that room take them
        if (const char* sb_ = sw_text(SW_STAMP_BUF)) {
            const int words = sw(SW_STAMP_WORDS);
            if (!pl.ph4 && lds + (size_t)16 * words <= 160 * 1024) {
                p.stamps = reinterpret_cast<unsigned*>(strtoull(sb_, nullptr, 0));
                p.stamp_lds_off = (int)lds;
                p.stamp_words = words;
                lds += (size_t)16 * words;
            }
        }
#endif
        if ((rc = bf3_fits(d, pl, lds))) return rc;
        const unsigned nblk = bf3_workgroups((long long)d->N * c.tiles_y * c.tiles_x * c.co_tiles, lds, sb);
        void* args[] = {&p};
        hipError_t e = hipLaunchKernel(kfn, dim3(nblk), dim3(256), args, lds, a.stream);
        if (e != hipSuccess) return fail(AP_ERR_LAUNCH, "conv_bf16x3 launch: %s", hipGetErrorString(e));
        return AP_OK;
    });
}

// Which launcher serves a plan.  With a statistics epilogue wanted the two narrow-output layers stay on the general kernel, and
// the last 7x7 layer on the vector ALUs
enum class FwdFamily { TSmall, Head, Small, Bf3, TapGemm, Direct, Igemm };
static FwdFamily fwd_family(const ap_conv_desc* d, const Plan& pl, bool with_stats) {
    if (pl.tsmall && !with_stats) return FwdFamily::TSmall;
    if (pl.head && !with_stats) return FwdFamily::Head;
    if (pl.small) return FwdFamily::Small;
    if (pl.bf3) return FwdFamily::Bf3;
    if (pl.direct_cop) return tapgemm_serves(d, pl, with_stats) ? FwdFamily::TapGemm : FwdFamily::Direct;
    return FwdFamily::Igemm;
}

// Every forward entry point: plan, refuse what the plan or the arguments rule out, then the family's launcher
static int conv2d_fwd_impl(const ap_conv_desc* d, const OutForm& o, const FwdArgs& a) {
    Plan pl;
    int rc = make_plan(d, pl);
    if (rc) return rc;
    rc = check_fwd_args(d, pl, o, &a);
    if (rc) return rc;
    switch (fwd_family(d, pl, a.stats != nullptr)) {
        case FwdFamily::TSmall: return launch_tsmall(d, pl, a);
        case FwdFamily::Head: return launch_head(d, pl, a);
        case FwdFamily::Small: return launch_small(d, pl, a);
        case FwdFamily::Bf3: return launch_bf3(d, pl, o, a);
        case FwdFamily::TapGemm: return launch_tapgemm(d, pl, a);
        case FwdFamily::Direct: return launch_direct(d, pl, a);
        default: return launch_igemm(d, pl, a);
    }
}

// ------------------------------------------------------------------ the launch as text (ap_conv2d_fwd_route)
// A kernel's word: the registries' names without their blanks
static std::string word_of(const char* name) {
    std::string w;
    for (const char* c = name; *c; ++c)
        if (*c != ' ') w += *c;
    return w;
}
static std::string igemm_word(const ConvKernelInfo& k) {
    char name[64];
    snprintf(name, sizeof(name), "ConvCfg<%d,%d,%d,%d,%d,%d,%d>", k.CI, k.S, k.K, k.WCO, k.MT, k.WPX, k.NT);
    return name;
}
static std::string num(long long v) { return std::to_string(v); }
// name<a> / name<a,b>
static std::string inst(const char* name, int a) { return std::string(name) + "<" + num(a) + ">"; }
static std::string inst(const char* name, int a, int b) { return std::string(name) + "<" + num(a) + "," + num(b) + ">"; }

// what conv2d_fwd_impl would launch for this descriptor and output form, from the launchers' own decisions: nothing is launched
// and no pointer is followed
static int fwd_route_text(const ap_conv_desc* d, int with_stats, int out_form, char* buf, int n) {
    Plan pl;
    int rc = make_plan(d, pl);
    if (rc) return rc;
    if (!buf || n < 1) return fail(AP_ERR_INVALID, "fwd_route: bad buffer");
    if (out_form < 0 || out_form > 4) return fail(AP_ERR_INVALID, "fwd_route: out_form %d", out_form);
    if (out_form >= 3 && with_stats) return fail(AP_ERR_INVALID, "fwd_route: the view forms take no statistics buffer");
    // a window's size does not change the kernel: the whole output stands for every window
    ap_out_view whole;
    memset(&whole, 0, sizeof(whole));
    whole.OH = pl.Hout; whole.OW = pl.Wout; whole.xstride = 1;
    OutForm o;
    o.view = out_form >= 3 ? &whole : nullptr;
    o.octet = out_form == 1;
    o.bf16 = out_form == 2 || out_form == 4;
    if ((rc = check_fwd_args(d, pl, o, nullptr))) return rc;
    std::string text;
    switch (fwd_family(d, pl, with_stats != 0)) {
        case FwdFamily::TSmall:
            if ((rc = tsmall_grid_ok(d))) return rc;
            text = inst("tsmall", tsmall_inst(d->Cout));
            break;
        case FwdFamily::Head: text = inst("head", head_rows(d->N, pl.Hout)); break;
        case FwdFamily::Small: text = inst("small", d->stride, d->Cout) + (small_gathers(d->stride) ? " gather" : " staged"); break;
        case FwdFamily::TapGemm: text = "tapgemm th=" + num(tapgemm_band(d->N, pl.Hout, tapgemm_tiles_x(pl))); break;
        case FwdFamily::Direct: text = inst("direct", d->KH, pl.direct_cop); break;
        case FwdFamily::Bf3:
            rc = bf3_launches(d, pl, o, [&](const Launch& L, const Bf3Launch& c) -> int {
                int r = bf3_fits(d, pl, c.lds);
                if (r) return r;
                if (!text.empty()) text += "; ";
                text += "bf3 " + word_of(c.kern->name) + " taps=" + num((long long)L.taps.size()) +
                        (d->precision == AP_PRECISION_BF16 ? " b16" : " x3") + (o.bf16 ? " ob16" : "");
                if (c.s2d_div > 0) text += c.s2d3_ct ? " s2d3=ct" : " s2d3=mask";
                if (pl.launches.size() > 1) text += pl.ph4 ? " phases=ph4" : (pl.fused_phases ? " phases=fused" : " phases=4launch");
                text += " wg=" + num(bf3_workgroups((long long)d->N * c.tiles_y * c.tiles_x * c.co_tiles, c.lds, false));
                return AP_OK;
            });
            if (rc) return rc;
            break;
        default:
            for (const auto& L : pl.launches) {
                unsigned bits;
                if ((rc = igemm_launch_ok(d, pl, L, bits))) return rc;
                if (!text.empty()) text += "; ";
                text += "igemm " + igemm_word(*pl.k) + " taps=" + num((long long)L.taps.size());
            }
    }
    snprintf(buf, n, "%s", text.c_str());
    return AP_OK;
}

// every kernel word ap_conv2d_fwd_route can produce, one per line: the fixed instantiation lists of the small families and the registries
static int fwd_route_names(char* buf, int n) {
    if (!buf || n < 1) return fail(AP_ERR_INVALID, "fwd_route_names: bad buffer");
    std::string all;
    for (int c : kTSmallCouts) all += inst("tsmall", c) + "\n";
    for (int rb : kHeadRows) all += inst("head", rb) + "\n";
    for (const auto& c : kSmallCfgs) all += inst("small", c[0], c[1]) + "\n";
    for (int cop : kDirectCops) all += inst("direct", 7, cop) + "\n";
    all += "tapgemm\n";
    for (const auto& k : registry()) all += igemm_word(k) + "\n";
    for (const auto& k : bf3_registry()) all += word_of(k.name) + "\n";
    for (int kk : {3, 4}) all += word_of(ph4_kernel(kk)->name) + "\n";
    snprintf(buf, n, "%s", all.c_str());
    return (int)all.size() < n ? AP_OK : fail(AP_ERR_INVALID, "fwd_route_names: %d bytes needed", (int)all.size() + 1);
}

}  // namespace apamd

using namespace apamd;

extern "C" {

int ap_conv2d_fwd(const ap_conv_desc* d, const float* packed, const float* bias, float* y,
                  float* stat_partials, ap_stream_t stream) {
    return conv2d_fwd_impl(d, OutForm(), {packed, bias, y, stat_partials, (hipStream_t)stream});
}

int ap_conv2d_fwd_view(const ap_conv_desc* d, const ap_out_view* view, const float* packed, const float* bias, float* y,
                       ap_stream_t stream) {
    if (!view) return fail(AP_ERR_INVALID, "conv2d_fwd_view: null view");
    OutForm o;
    o.view = view;
    return conv2d_fwd_impl(d, o, {packed, bias, y, nullptr, (hipStream_t)stream});
}

int ap_conv2d_fwd_octet(const ap_conv_desc* d, const float* packed, const float* bias, float* y, float* stat_partials,
                        ap_stream_t stream) {
    OutForm o;
    o.octet = true;
    return conv2d_fwd_impl(d, o, {packed, bias, y, stat_partials, (hipStream_t)stream});
}

int ap_conv2d_fwd_bf16out(const ap_conv_desc* d, const float* packed, const float* bias, void* y_bf16, float* stat_partials,
                          ap_stream_t stream) {
    OutForm o;
    o.bf16 = true;
    return conv2d_fwd_impl(d, o, {packed, bias, reinterpret_cast<float*>(y_bf16), stat_partials, (hipStream_t)stream});
}

int ap_conv2d_fwd_route(const ap_conv_desc* d, int32_t with_stats, int32_t out_form, char* buf, int32_t buflen) {
    return fwd_route_text(d, with_stats, out_form, buf, buflen);
}

int ap_conv2d_fwd_route_names(char* buf, int32_t buflen) { return fwd_route_names(buf, buflen); }

int ap_conv2d_fwd_view_bf16out(const ap_conv_desc* d, const ap_out_view* view, const float* packed, const float* bias, void* y_bf16,
                               ap_stream_t stream) {
    if (!view) return fail(AP_ERR_INVALID, "conv2d_fwd_view_bf16out: null view");
    OutForm o;
    o.view = view;
    o.bf16 = true;
    return conv2d_fwd_impl(d, o, {packed, bias, reinterpret_cast<float*>(y_bf16), nullptr, (hipStream_t)stream});
}

}  // extern "C"
