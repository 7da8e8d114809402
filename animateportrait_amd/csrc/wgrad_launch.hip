// wgrad_launch.hip -- the launches of the general weight-gradient family: kernel tables, one launcher per family, the entry points.
//
// ap_conv2d_wgrad / _pre plan a layer (wgrad_plan.h: make_wgrad_plan) and launch its family:
//   narrow     wgrad_narrow.h -> wgrad_reduce_kernel
//   bf16 GEMM  both operands re-tiled into bf16 pixel-octet slots (wgrad_operand.hip: split_transpose_* / xs_transpose_kernel, or
//              the M-role operand as its producer wrote it: _pre) -> wgrad_bf16x3 -> wgrad_bf3_reduce_kernel
//   igemm      pad_materialize A (+ G unless g is plain and tile-aligned) -> wgrad_igemm_f32 -> wgrad_reduce_kernel
// ap_conv2d_wgrad_xs: the bf16 GEMM straight from the convolutions' split copies, no operand preparation (wgrad_xs.h).
// ap_pad_materialize exposes the igemm family's operand pass.
#include "wgrad_plan.h"
#include "wgrad_bf16x3.h"
#include "wgrad_xs.h"
#include "wgrad_igemm.h"
#include "wgrad_narrow.h"
// The last layer's vector-ALU weight gradient (ap_conv_final_wgrad) sums its partials with launch_wgrad_reduce, as the narrow and
// igemm families do; wgrad_igemm.h defines wgrad_reduce_kernel and pad_materialize_kernel with external linkage, so one translation
// unit only can include it: that entry point stays here, with launch_wgrad_reduce, like ap_pad_materialize with launch_pad.
#include "wgrad_final.h"

#include <algorithm>
#include <cstring>
#include <iterator>

namespace apamd {

// ------------------------------------------------------------------ kernel tables
template <class C>
static WgradKernel wk() {
    return WgradKernel{C::S, C::K, C::M_TILE, C::Q_TILE, C::PR, reinterpret_cast<const void*>(&wgrad_igemm_f32<C>),
                       4 * C::lds_floats()};
}

static const WgradKernel kWgradKernels[] = {
    wk<WgradCfg<1, 3, 2, 4, 2>>(), wk<WgradCfg<1, 4, 2, 4, 2>>(), wk<WgradCfg<1, 7, 2, 4, 2>>(),
    wk<WgradCfg<2, 3, 2, 4, 1>>(), wk<WgradCfg<2, 4, 2, 4, 1>>(),
    wk<WgradCfg<1, 7, 1, 3, 2>>(),                 // 64 x 192 tiles: the 7x7 stems (Cin = 3: Q = 147)
    wk<WgradCfg<2, 3, 1, 1, 1>>(),                 // 64 x 64 tiles: the landmark encoder's 8 -> 16 -> 16 layers
    wk<WgradCfg<2, 3, 1, 4, 1>>(),                 // 64 x 256 tiles: 64-output stride-2 layers
};

template <class C>
static WgradBf3Kernel bk(int form) {
    return WgradBf3Kernel{C::K, form, reinterpret_cast<const void*>(&wgrad_bf16x3<C>), C::lds_bytes(), C::NWAVES * 64};
}
// BF3_SPLIT: head + tail staged, three products per tap (AP_PRECISION_BF16X3); BF3_HEADS: head planes only, one product per tap
// (AP_PRECISION_BF16): two workgroups per CU; BF3_WIDE: the 8-wave workgroup (128 x 64 channel tile, WM = 4) of the split form
static const WgradBf3Kernel kWgradBf3Kernels[] = {
    bk<WgradBf3Cfg<3, 2>>(BF3_SPLIT), bk<WgradBf3Cfg<3, 1>>(BF3_HEADS), bk<WgradBf3Cfg<3, 2, 3, 4>>(BF3_WIDE),
    bk<WgradBf3Cfg<4, 2>>(BF3_SPLIT), bk<WgradBf3Cfg<4, 1>>(BF3_HEADS),
    // K = 2: the space-to-depth forms of stride-2 layers
    bk<WgradBf3Cfg<2, 2>>(BF3_SPLIT), bk<WgradBf3Cfg<2, 1>>(BF3_HEADS), bk<WgradBf3Cfg<2, 2, 2, 4>>(BF3_WIDE),
    // K = 7: the ROW form of the 7x7 stems (1 x 7 taps over 7 Cin row channels: KY = 1)
    bk<WgradBf3Cfg<7, 2, 1>>(BF3_SPLIT), bk<WgradBf3Cfg<7, 1, 1>>(BF3_HEADS),
};

#define APAMD_NARROW(...) reinterpret_cast<const void*>(&__VA_ARGS__)
static const WgradNarrowKernel kWgradNarrowKernels[] = {
    {3, 1, 1, 0, 8, APAMD_NARROW(wgrad_narrow_kernel<3, 1, 1, 8>)},
    {4, 2, 1, 0, 4, APAMD_NARROW(wgrad_narrow_kernel<4, 2, 1, 4>)},
    {4, 2, 2, 0, 4, APAMD_NARROW(wgrad_narrow_kernel<4, 2, 2, 4>)},
    {4, 2, 1, 1, 4, APAMD_NARROW(wgrad_narrow_s2k4_kernel<1, 4, 1>)},          // the LDS-staged form
    {4, 2, 2, 1, 4, APAMD_NARROW(wgrad_narrow_s2k4_kernel<2, 4, 1>)},
};
#undef APAMD_NARROW
const WgradNarrowKernel* narrow_kernel(int K, int S, int Cin, int ppt) {
    for (const auto& k : kWgradNarrowKernels)
        if (k.K == K && k.S == S && k.Cin == Cin && k.ppt == ppt) return &k;
    return nullptr;
}

KernelTable<WgradKernel> wgrad_igemm_kernels() { return {std::begin(kWgradKernels), std::end(kWgradKernels)}; }
KernelTable<WgradBf3Kernel> wgrad_bf3_kernels() { return {std::begin(kWgradBf3Kernels), std::end(kWgradBf3Kernels)}; }
KernelTable<WgradNarrowKernel> wgrad_narrow_kernels() { return {std::begin(kWgradNarrowKernels), std::end(kWgradNarrowKernels)}; }

// ------------------------------------------------------------------ the igemm family's operand pass (the bf16 GEMM's: wgrad_operand.hip)
static int launch_pad(const ap_src* segs, int nseg, int N, int C, int H, int W, int pad, int pad_mode, int Hp, int Wp,
                      float* out, hipStream_t stream) {
    PadParams p;
    memset(&p, 0, sizeof(p));
    p.nseg = nseg;
    int cbeg = 0;
    for (int s = 0; s < nseg; ++s) {
        fill_seg(p.seg[s], segs[s], cbeg);
        cbeg += segs[s].C;
    }
    p.N = N; p.C = C; p.H = H; p.W = W; p.pad = pad; p.pad_mode = pad_mode; p.Hp = Hp; p.Wp = Wp; p.out = out;
    if (N > 65535 || C > 65535) return fail(AP_ERR_UNSUPPORTED, "pad_materialize: N=%d C=%d", N, C);
    int bx = (Hp * Wp + 255) / 256;
    if (bx > 64) bx = 64;
    hipLaunchKernelGGL(pad_materialize_kernel, dim3(bx, C, N), dim3(256), 0, stream, p);
    return check_launch("pad_materialize_kernel");
}

// ------------------------------------------------------------------ one launcher per family
static int launch_narrow(const ap_wgrad_desc* d, const WgradPlan& pl, float* workspace, float* dw, hipStream_t stream) {
    const NarrowPlan& n = pl.narrow;
    WgradNarrowParams p;
    memset(&p, 0, sizeof(p));
    fill_seg(p.src, d->src[0], 0);
    p.g = d->g.data;
    p.N = d->N; p.M = d->M; p.GH = d->GH; p.GW = d->GW; p.H = d->H; p.W = d->W; p.pad = d->pad; p.pad_mode = d->pad_mode;
    p.rows_per_block = n.rows_per_block; p.gwc = n.gwc; p.gwc_shift = n.gwc_shift; p.rpi = n.rpi;
    p.partial = workspace;
    const dim3 grid(pl.P, (d->M + n.k->cob - 1) / n.k->cob);
    const size_t lds = n.k->ppt ? (size_t)2 * pl.Cin * (2 * n.rpi * n.k->ppt + 2) * (d->W + 2) * sizeof(float) : 0;
    void* args[] = {&p};
    (void)hipLaunchKernel(n.k->fn, grid, dim3(256), args, lds, stream);
    int rc = check_launch("wgrad_narrow_kernel");
    if (rc) return rc;
    launch_wgrad_reduce(stream, workspace, pl.P, (long long)d->M * pl.Q, dw);
    return check_launch("wgrad_reduce_kernel");
}

// dW = the sum of a bf16 GEMM's partial tiles (wgrad_bf16x3 or wgrad_xs_kernel), scattered into the layer's own layout
static int launch_bf3_reduce(const WgradPlan& pl, const ap_wgrad_desc* d, const float* partial, float* dw, hipStream_t stream) {
    const Bf16GemmPlan& b = pl.bf;
    const int blocks = (int)std::min<long long>((b.sum_floats + 255) / 256, 4096);
    hipLaunchKernelGGL(wgrad_bf3_reduce_kernel, dim3(blocks), dim3(256), 0, stream, partial, pl.P, d->M, b.Cb, b.taps, b.c_tiles,
                       b.sum_floats, b.s2d ? pl.Cin : 0, d->K, dw, b.wide ? 4 : 2);
    return check_launch("wgrad_bf3_reduce_kernel");
}

// the kernel table entry of a bf16 GEMM plan (b16: plain-bf16 arithmetic)
const WgradBf3Kernel* bf3_kernel(const Bf16GemmPlan& b, bool b16) {
    const WgradBf3Kernel* k = nullptr;
    for (const auto& c : kWgradBf3Kernels)
        if (c.K == b.Kb && c.form == (b.wide ? BF3_WIDE : (b16 ? BF3_HEADS : BF3_SPLIT))) k = &c;
    return k;
}

static int launch_bf16_gemm(const ap_wgrad_desc* d, const WgradPlan& pl, const void* g_t, bool from_xs, float* workspace, float* dw,
                            hipStream_t stream) {
    const Bf16GemmPlan& b = pl.bf;
    const bool b16 = d->precision == AP_PRECISION_BF16;
    const WgradBf3Kernel* k = bf3_kernel(b, b16);
    if (!k) return fail(AP_ERR_UNSUPPORTED, b.wide ? "wgrad: no 8-wave kernel for k=%d" : "wgrad: no split-bf16 kernel for k=%d", b.Kb);
    int rc = ensure_dyn_lds(k->fn, 160 * 1024);
    if (rc) return rc;
    uint4* at = reinterpret_cast<uint4*>(workspace);
    uint4* gt = reinterpret_cast<uint4*>(workspace + pl.a_floats);
    float* partial = workspace + pl.a_floats + pl.g_floats;
    rc = launch_bf16_gemm_operand(d, pl, from_xs, at, stream);
    if (rc) return rc;
    if (g_t) {
        gt = reinterpret_cast<uint4*>(const_cast<void*>(g_t));
    } else {
        ap_src g = d->g;
        g.C = d->M;
        rc = launch_split_transpose(&g, 1, d->N, d->M, d->GH, d->GW, 0, AP_PAD_ZERO, b.GHp, b.GX8, b.Mp, gt, stream, 0, b16);
        if (rc) return rc;
    }
    WgradBf3Params p;
    memset(&p, 0, sizeof(p));
    p.gt = gt; p.at = at;
    p.N = d->N; p.M = d->M; p.Cin = b.Cb; p.Q = b.Cb * b.taps;
    p.GHp = b.GHp; p.GX8 = b.GX8; p.Mp = b.Mp; p.Hp = b.Hp; p.AX8 = b.AX8; p.Cp = b.Cp;
    p.tiles_x = pl.tiles_x; p.tiles_y = pl.tiles_y; p.nstages = pl.nstages; p.P = pl.P;
    p.m_tiles = pl.m_tiles; p.c_tiles = b.c_tiles;
    p.partial = partial;
#ifdef APAMD_ABLATION
    p.ablate = sw(SW_ABLATE);
#endif
    void* args[] = {&p};
    const unsigned nblk = (unsigned)(pl.m_tiles * b.c_tiles * pl.P);
    hipError_t e = hipLaunchKernel(k->fn, dim3(nblk), dim3(k->threads), args, k->lds_bytes, stream);
    if (e != hipSuccess) return fail(AP_ERR_LAUNCH, "wgrad_bf16x3 launch: %s", hipGetErrorString(e));
    return launch_bf3_reduce(pl, d, partial, dw, stream);
}

static int launch_igemm(const ap_wgrad_desc* d, const WgradPlan& pl, float* workspace, float* dw, hipStream_t stream) {
    const IgemmPlan& g = pl.ig;
    int rc = ensure_dyn_lds(pl.k->fn, 160 * 1024);
    if (rc) return rc;
    float* a_pad = workspace;
    float* g_pad = workspace + pl.a_floats;
    float* partial = g_pad + pl.g_floats;
    rc = launch_pad(d->src, d->nsrc, d->N, pl.Cin, d->H, d->W, d->pad, d->pad_mode, g.Hp, g.Wp, a_pad, stream);
    if (rc) return rc;
    if (!g.g_direct) {
        ap_src gs = d->g;
        gs.C = d->M;
        rc = launch_pad(&gs, 1, d->N, d->M, d->GH, d->GW, 0, AP_PAD_ZERO, g.GHp, g.GWp, g_pad, stream);
        if (rc) return rc;
    }
    WgradKParams p;
    memset(&p, 0, sizeof(p));
    p.g = g.g_direct ? d->g.data : g_pad;
    p.a = a_pad;
    p.N = d->N; p.M = d->M; p.Cin = pl.Cin; p.Q = pl.Q;
    p.GHp = g.GHp; p.GWp = g.GWp; p.Hp = g.Hp; p.Wp = g.Wp;
    p.tiles_x = pl.tiles_x; p.tiles_y = pl.tiles_y; p.nstages = pl.nstages; p.P = pl.P;
    p.m_tiles = pl.m_tiles; p.q_tiles = g.q_tiles;
    p.partial = partial;
#ifdef APAMD_ABLATION
    p.ablate = sw(SW_ABLATE);
#endif
    void* args[] = {&p};
    const unsigned nblk = (unsigned)(pl.m_tiles * g.q_tiles * pl.P);
    hipError_t e = hipLaunchKernel(pl.k->fn, dim3(nblk), dim3(256), args, pl.k->lds_bytes, stream);
    if (e != hipSuccess) return fail(AP_ERR_LAUNCH, "wgrad_igemm_f32 launch: %s", hipGetErrorString(e));
    launch_wgrad_reduce(stream, partial, pl.P, (long long)d->M * pl.Q, dw);
    return check_launch("wgrad_reduce_kernel");
}

// g_t: the M-role operand already in the kernel's layout (ap_conv2d_wgrad_gt_dims), written by its producer
// (ap_instnorm_bwd_split) -- the transposition pass over d->g is skipped and d->g.data is not read
static int wgrad_impl(const ap_wgrad_desc* d, const void* g_t, float* workspace, float* dw, ap_stream_t stream_) {
    WgradPlan pl;
    int rc = make_wgrad_plan(d, pl);
    if (rc) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    if (g_t && !pl.bf16_gemm()) return fail(AP_ERR_UNSUPPORTED, "wgrad: a prepared operand needs the bf16 matrix plan (ap_conv2d_wgrad_gt_dims)");
    if (!workspace || !dw || (!d->g.data && !g_t)) return fail(AP_ERR_INVALID, "wgrad: null pointer");
    if ((d->g.mean == nullptr) != (d->g.rstd == nullptr)) return fail(AP_ERR_INVALID, "wgrad: g mean/rstd mismatch");
    const bool from_xs = wgrad_xs_route(d, pl);
    for (int s = 0; s < d->nsrc; ++s) {
        if (!d->src[s].data && !from_xs) return fail(AP_ERR_INVALID, "wgrad: segment %d: null data", s);
        if ((d->src[s].mean == nullptr) != (d->src[s].rstd == nullptr))
            return fail(AP_ERR_INVALID, "wgrad: segment %d mean/rstd mismatch", s);
        if ((d->src[s].act & 0x100) && !pl.bf16_gemm())      // bit 8: bf16 data (launch_split_transpose)
            return fail(AP_ERR_UNSUPPORTED, "wgrad: segment %d holds bf16 values but the layer is not on the bf16 matrix plan", s);
    }
    switch (pl.family) {
    case WgradFamily::Narrow: return launch_narrow(d, pl, workspace, dw, stream);
    case WgradFamily::Bf16Gemm: return launch_bf16_gemm(d, pl, g_t, from_xs, workspace, dw, stream);
    default: return launch_igemm(d, pl, workspace, dw, stream);
    }
}

// ------------------------------------------------------------------ both operands from the split copies (wgrad_xs.h)
template <class C>
static int launch_wgrad_xs(const WgradXsParams& p, unsigned nblk, hipStream_t stream) {
    const void* fn = reinterpret_cast<const void*>(&wgrad_xs_kernel<C>);
    int rc = ensure_dyn_lds(fn, 160 * 1024);
    if (rc) return rc;
    WgradXsParams q = p;
    void* args[] = {&q};
    hipError_t e = hipLaunchKernel(fn, dim3(nblk), dim3(C::NT), args, C::lds_bytes(), stream);
    if (e != hipSuccess) return fail(AP_ERR_LAUNCH, "wgrad_xs launch: %s", hipGetErrorString(e));
    return AP_OK;
}

// by (kernel size the GEMM sees, staged parts, wave rows): split bf16 everywhere, plain bf16 on the 3x3 layers
static const WgradXsKernel kWgradXsKernels[] = {
    {2, 2, 2, &launch_wgrad_xs<WgradXsCfg<2, 2, 2>>}, {2, 2, 4, &launch_wgrad_xs<WgradXsCfg<2, 2, 4>>},
    {3, 1, 2, &launch_wgrad_xs<WgradXsCfg<3, 1, 2>>}, {3, 2, 2, &launch_wgrad_xs<WgradXsCfg<3, 2, 2>>},
    {3, 2, 4, &launch_wgrad_xs<WgradXsCfg<3, 2, 4>>}, {4, 2, 2, &launch_wgrad_xs<WgradXsCfg<4, 2, 2>>},
};
const WgradXsKernel* xs_kernel(const ap_wgrad_desc* d, const Bf16GemmPlan& b) {
    const int parts = d->precision == AP_PRECISION_BF16 ? 1 : 2, wm = b.wide ? 4 : 2;
    const WgradXsKernel* k = nullptr;
    for (const auto& c : kWgradXsKernels)
        if (c.Kb == b.Kb && c.parts == parts && c.wm == wm) k = &c;
    return k;
}
KernelTable<WgradXsKernel> wgrad_xs_kernels() { return {std::begin(kWgradXsKernels), std::end(kWgradXsKernels)}; }

// pixel-tile split of wgrad_final_kernel: ~1024 workgroups in all
static void final_split(int N, int C, int H, int W, int& tiles_x, int& tiles_y, int& tpb, int& P) {
    tiles_x = (W + 63) / 64;
    tiles_y = (H + 16 * kFinalStrips - 1) / (16 * kFinalStrips);
    const long long total = (long long)N * tiles_x * tiles_y;
    long long want = std::max<long long>(1, 1024 / std::max(C, 1));
    if (want > total) want = total;
    tpb = (int)((total + want - 1) / want);
    P = (int)((total + tpb - 1) / tpb);
}

}  // namespace apamd

using namespace apamd;

extern "C" {

int ap_conv2d_wgrad(const ap_wgrad_desc* d, float* workspace, float* dw, ap_stream_t stream) {
    return wgrad_impl(d, nullptr, workspace, dw, stream);
}

int ap_conv2d_wgrad_pre(const ap_wgrad_desc* d, const void* g_t, float* workspace, float* dw, ap_stream_t stream) {
    if (!g_t) return fail(AP_ERR_INVALID, "wgrad_pre: null operand");
    return wgrad_impl(d, g_t, workspace, dw, stream);
}

int ap_conv2d_wgrad_xs(const ap_wgrad_desc* d, const void* g_xs, float* workspace, float* dw, ap_stream_t stream_) {
    WgradPlan pl;
    int rc = make_wgrad_plan(d, pl);
    if (rc) return rc;
    if (!g_xs || !workspace || !dw) return fail(AP_ERR_INVALID, "wgrad_xs: null pointer");
    if (!wgrad_xs_direct_ok(d, pl)) return fail(AP_ERR_UNSUPPORTED, "wgrad_xs: the layer is not on this route (ap_conv2d_wgrad_xs_ok)");
    hipStream_t stream = (hipStream_t)stream_;
    const Bf16GemmPlan& b = pl.bf;
    WgradXsParams p;
    memset(&p, 0, sizeof(p));
    p.g_xs = reinterpret_cast<const uint4*>(g_xs);
    p.N = d->N; p.M = d->M; p.GH = d->GH; p.GW = d->GW;
    if (b.s2d) {
        p.nseg = 1;
        p.a_xs[0] = reinterpret_cast<const uint4*>(d->src_xs_s2d ? d->src_xs_s2d : d->src_xs[0]);
        p.a_cg_begin[0] = 0; p.a_cg_begin[1] = b.Cb / 8;
        p.H = b.Hb; p.W = b.Wb; p.pad = 0; p.pad_mode = AP_PAD_ZERO;
        p.s2d_c = d->src_xs_s2d ? 0 : pl.Cin;
    } else {
        p.nseg = d->nsrc;
        int cg = 0;
        for (int s = 0; s < d->nsrc; ++s) {
            p.a_xs[s] = reinterpret_cast<const uint4*>(d->src_xs[s]);
            p.a_cg_begin[s] = cg;
            cg += d->src[s].C / 8;
        }
        p.a_cg_begin[d->nsrc] = cg;
        p.H = d->H; p.W = d->W; p.pad = d->pad; p.pad_mode = d->pad_mode;
    }
    p.tiles_x = pl.tiles_x; p.tiles_y = pl.tiles_y; p.nstages = pl.nstages; p.P = pl.P; p.m_tiles = pl.m_tiles; p.c_tiles = b.c_tiles;
    p.partial = workspace;
    const WgradXsKernel* k = xs_kernel(d, b);
    if (!k)
        return fail(AP_ERR_UNSUPPORTED, "wgrad_xs: no kernel for k=%d, %d parts, %d wave rows", b.Kb, d->precision == AP_PRECISION_BF16 ? 1 : 2,
                    b.wide ? 4 : 2);
    rc = k->launch(p, (unsigned)(pl.m_tiles * b.c_tiles * pl.P), stream);
    if (rc) return rc;
    return launch_bf3_reduce(pl, d, workspace, dw, stream);
}

int ap_pad_materialize(const ap_src* src, int32_t nsrc, int32_t N, int32_t H, int32_t W, int32_t pad, int32_t pad_mode,
                       int32_t Hp, int32_t Wp, float* out, ap_stream_t stream) {
    if (!src || !out || nsrc < 1 || nsrc > kMaxSeg) return fail(AP_ERR_INVALID, "pad_materialize: bad arguments");
    if (Hp < H + 2 * pad || Wp < W + 2 * pad) return fail(AP_ERR_INVALID, "pad_materialize: output smaller than padded input");
    if (pad_mode == AP_PAD_REFLECT && (pad >= H || pad >= W)) return fail(AP_ERR_INVALID, "pad_materialize: reflection pad too large");
    int C = 0;
    for (int s = 0; s < nsrc; ++s) {
        if (!src[s].data || src[s].C < 1) return fail(AP_ERR_INVALID, "pad_materialize: segment %d", s);
        if ((src[s].mean == nullptr) != (src[s].rstd == nullptr)) return fail(AP_ERR_INVALID, "pad_materialize: mean/rstd mismatch");
        C += src[s].C;
    }
    return launch_pad(src, nsrc, N, C, H, W, pad, pad_mode, Hp, Wp, out, (hipStream_t)stream);
}

int64_t ap_conv_final_wgrad_workspace_floats(int32_t N, int32_t C, int32_t H, int32_t W) {
    if (N < 1 || C < 1 || H < 1 || W < 1) return fail(AP_ERR_INVALID, "conv_final_wgrad: bad sizes");
    int tx, ty, tpb, P;
    final_split(N, C, H, W, tx, ty, tpb, P);
    return (int64_t)P * C * 49;
}

int ap_conv_final_wgrad(const ap_src* src, const float* g, int32_t N, int32_t H, int32_t W, int32_t K, int32_t pad,
                        int32_t pad_mode, float* workspace, float* dw, ap_stream_t stream_) {
    if (!src || !src->data || !g || !workspace || !dw) return fail(AP_ERR_INVALID, "conv_final_wgrad: null pointer");
    if ((src->mean == nullptr) != (src->rstd == nullptr)) return fail(AP_ERR_INVALID, "conv_final_wgrad: mean/rstd mismatch");
    if (K != 7 || pad != 3 || N < 1 || src->C < 1 || src->C > 65535 || H < 1 || W < 1)
        return fail(AP_ERR_UNSUPPORTED, "conv_final_wgrad: built for 7x7 pad-3 layers with one output channel (K=%d, pad=%d)", K, pad);
    if (pad_mode == AP_PAD_REFLECT && (pad >= H || pad >= W)) return fail(AP_ERR_INVALID, "conv_final_wgrad: reflection pad too large");
    if (src->act < 0 || src->act > 2) return fail(AP_ERR_INVALID, "conv_final_wgrad: act %d", src->act);
    hipStream_t stream = (hipStream_t)stream_;
    WgradFinalParams p;
    memset(&p, 0, sizeof(p));
    fill_seg(p.src, *src, 0);
    p.g = g; p.N = N; p.C = src->C; p.H = H; p.W = W; p.pad_mode = pad_mode;
    int P;
    final_split(N, src->C, H, W, p.tiles_x, p.tiles_y, p.tiles_per_block, P);
    p.partial = workspace;
    if ((W & 3) == 0) hipLaunchKernelGGL(wgrad_final_kernel<true>, dim3(P, src->C), dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(wgrad_final_kernel<false>, dim3(P, src->C), dim3(256), 0, stream, p);
    int rc = check_launch("wgrad_final_kernel");
    if (rc) return rc;
    const long long n = (long long)src->C * 49;
    launch_wgrad_reduce(stream, workspace, P, n, dw);
    return check_launch("wgrad_reduce_kernel");
}

}  // extern "C"
