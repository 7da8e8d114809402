// wgrad_host.hip -- C ABI of the weight-gradient operators.
//
// ap_conv2d_wgrad / _pre plan a layer (make_wgrad_plan) into one of three families and launch it:
//   narrow     1..2 input channels: one streaming pass over the fp32 tensors (wgrad_narrow.h) -> wgrad_reduce_kernel
//   bf16 GEMM  both operands re-tiled into bf16 pixel-octet slots (split_transpose_* / xs_transpose_kernel, or the M-role
//              operand as its producer wrote it: _pre) -> wgrad_bf16x3 -> wgrad_bf3_reduce_kernel; a stride-2 layer runs as its
//              space-to-depth view, a 7x7 stem (opt-in) as its row view, 128-output multiples on the 8-wave workgroup
//   igemm      exact fp32: pad_materialize A (+ G unless g is plain and tile-aligned) -> wgrad_igemm_f32 -> wgrad_reduce_kernel
// The caller provides ONE workspace; its layout is  [A prepared][G prepared (optional)][partials].
// ap_conv2d_wgrad_xs: the bf16 GEMM straight from the convolutions' split copies, no operand preparation (wgrad_xs.h).
// Layers with kernels of their own: ap_conv_head_wgrad (conv_head.h), ap_conv_final_wgrad (wgrad_final.h), ap_wgrad_k7_bf16 and
// ap_wgrad_d0_bf16 (wgrad_k7.h).  ap_pad_materialize exposes the igemm family's operand pass.
#include "common.h"
#include "conv_head.h"
#include "wgrad_bf16x3.h"
#include "wgrad_xs.h"
#include "wgrad_igemm.h"
#include "wgrad_narrow.h"
#include "wgrad_final.h"
#include "wgrad_k7.h"

#include <algorithm>
#include <atomic>
#include <climits>
#include <cstring>
#include <string>

namespace apamd {

// ------------------------------------------------------------------ kernel tables
struct WgradKernel {
    int S, K, M_TILE, Q_TILE, PR;
    const void* fn;
    size_t lds_bytes;
};

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

// split-bf16 instantiations by kernel size (stride 1) and form
enum { BF3_SPLIT, BF3_HEADS, BF3_WIDE };
struct WgradBf3Kernel {
    int K, form;
    const void* fn;
    size_t lds_bytes;
    int threads;
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

// streaming kernels for 1..2 input channels, by (K, S, Cin, ppt); cob = output channels per workgroup
struct WgradNarrowKernel {
    int K, S, Cin, ppt, cob;
    const void* fn;
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
static const WgradNarrowKernel* narrow_kernel(int K, int S, int Cin, int ppt) {
    for (const auto& k : kWgradNarrowKernels)
        if (k.K == K && k.S == S && k.Cin == Cin && k.ppt == ppt) return &k;
    return nullptr;
}

// ------------------------------------------------------------------ the plan: one family per layer
enum class WgradFamily { Narrow, Bf16Gemm, Igemm };

// streaming kernel for 1..2 input channels (wgrad_narrow.h)
struct NarrowPlan {
    const WgradNarrowKernel* k = nullptr;
    int gwc = 0, gwc_shift = 0, rpi = 0, rows_per_block = 0;
};
// split-bf16 kernel (wgrad_bf16x3.h): operands as [n][part][row][x/8][channel] pixel-octet slots
struct Bf16GemmPlan {
    bool s2d = false;       // the space-to-depth form of a stride-2 layer: a 2 x 2 stride-1 layer over 4 Cin channels
    bool rows = false;      // the row form of a 7x7 stem: a 1 x 7 layer over 7 Cin channels (channel ci * 7 + ky = the input shifted by ky rows)
    bool wide = false;      // the 8-wave workgroup: 128-channel M tiles (split-bf16 arithmetic, K <= 3, M % 128 == 0)
    int Kb = 0, Cb = 0, Hb = 0, Wb = 0;     // kernel size, channels and operand size the kernel sees
    int c_tiles = 0, Mp = 0, Cp = 0, GHp = 0, GX8 = 0, Hp = 0, AX8 = 0;
    int taps = 0;                           // taps per accumulator tile
    long long sum_floats = 0;               // one workgroup's partial sums = what the reduction adds up (accumulator-order tiles)
};
// exact-fp32 implicit GEMM (wgrad_igemm.h)
struct IgemmPlan {
    int q_tiles = 0, GHp = 0, GWp = 0, Hp = 0, Wp = 0;
    bool g_direct = false;
};
struct WgradPlan {
    WgradFamily family = WgradFamily::Igemm;
    int Cin = 0, Q = 0, P = 0;
    int tiles_x = 0, tiles_y = 0, nstages = 0, m_tiles = 0;          // pixel and M tiling of the two GEMM families
    long long a_floats = 0, g_floats = 0, part_floats = 0;           // the workspace
    const WgradKernel* k = nullptr;         // the fp32 kernel of the layer's (stride, K): a layer without one is not served at all
    NarrowPlan narrow;
    Bf16GemmPlan bf;
    IgemmPlan ig;
    bool bf16_gemm() const { return family == WgradFamily::Bf16Gemm; }
};

// several tile shapes of a family: the one whose padded (M x Q) tile grid wastes least (the 7x7 stems are
// M = 32..64 by Q = 147: 64 x 192 tiles are 77 % full where 128 x 256 ones are 29 %)
static const WgradKernel* pick_igemm_tile(const ap_wgrad_desc* d) {
    int cin = 0;
    for (int s = 0; s < d->nsrc; ++s) cin += d->src[s].C;
    const long long Q = (long long)cin * d->K * d->K;
    const WgradKernel* pick = nullptr;
    long long best = -1;
    for (const auto& k : kWgradKernels)
        if (k.S == d->stride && k.K == d->K) {
            const long long padded = ((d->M + k.M_TILE - 1) / k.M_TILE) * (long long)k.M_TILE *
                                     (((Q + k.Q_TILE - 1) / k.Q_TILE) * k.Q_TILE);
            // (a smaller tile re-reads its operands more often: it must save at least 30 % of the padded work)
            if (best < 0 || padded * 10 < best * 7) { best = padded; pick = &k; }
        }
    return pick;
}

// the descriptor's own consistency; fills Cin, Q and the fp32 kernel
static int check_wgrad_desc(const ap_wgrad_desc* d, WgradPlan& pl) {
    if (!d) return fail(AP_ERR_INVALID, "wgrad: null descriptor");
    if (d->nsrc < 1 || d->nsrc > kMaxSeg) return fail(AP_ERR_INVALID, "wgrad: nsrc=%d", d->nsrc);
    if (d->N < 1 || d->M < 1 || d->GH < 1 || d->GW < 1 || d->H < 1 || d->W < 1) return fail(AP_ERR_INVALID, "wgrad: bad dims");
    pl.k = pick_igemm_tile(d);
    if (!pl.k) return fail(AP_ERR_UNSUPPORTED, "wgrad: no kernel for stride %d, k %d", d->stride, d->K);
    if (d->pad_mode == AP_PAD_REFLECT && (d->pad >= d->H || d->pad >= d->W))
        return fail(AP_ERR_INVALID, "wgrad: reflection pad %d >= input size", d->pad);
    // the iterated grid must be the conv output grid of the shifted tensor
    const int oh = (d->H + 2 * d->pad - d->K) / d->stride + 1, ow = (d->W + 2 * d->pad - d->K) / d->stride + 1;
    if (oh != d->GH || ow != d->GW)
        return fail(AP_ERR_INVALID, "wgrad: grid %dx%d does not match conv output %dx%d", d->GH, d->GW, oh, ow);
    pl.Cin = 0;
    for (int s = 0; s < d->nsrc; ++s) {
        if (d->src[s].C < 1) return fail(AP_ERR_INVALID, "wgrad: segment %d has C=%d", s, d->src[s].C);
        pl.Cin += d->src[s].C;
    }
    pl.Q = pl.Cin * d->K * d->K;
    return AP_OK;
}

// 1..2 input channels (landmark encoder / PatchGAN first layer): one streaming pass, no operand copies (wgrad_narrow.h)
static bool plan_narrow(const ap_wgrad_desc* d, WgradPlan& pl) {
    if (d->nsrc != 1 || d->g.mean != nullptr || d->g.act != AP_ACT_NONE) return false;
    const int S = d->stride, K = d->K;
    const WgradNarrowKernel* k = narrow_kernel(K, S, pl.Cin, 0);
    if (!k) return false;
    NarrowPlan& n = pl.narrow;
    const int groups = (d->M + k->cob - 1) / k->cob;
    int gwc = 1, sh = 0;
    while (gwc < d->GW && gwc < 256) { gwc <<= 1; ++sh; }
    n.gwc = gwc; n.gwc_shift = sh; n.rpi = 256 / gwc;
    const long long total_rows = (long long)d->N * d->GH;
    const long long P = std::max<long long>(1, 1024 / groups);
    long long rpb = (total_rows + P - 1) / P;
    // K = 4 stride 2 with zero pad 1 on rows a workgroup spans exactly (the PatchGAN first layer): the LDS-staged
    // form (one output pixel per thread and iteration: 2 and 4 measured slower, 277 registers) (wgrad_narrow_s2k4_kernel)
    constexpr int kNarrowPPT = 1;
    if (K == 4 && S == 2 && d->pad == 1 && d->pad_mode == AP_PAD_ZERO && gwc == d->GW && d->W == 2 * d->GW &&
        d->H == 2 * d->GH && (d->GH % (n.rpi * kNarrowPPT)) == 0)
        k = narrow_kernel(K, S, pl.Cin, kNarrowPPT);
    n.k = k;
    const int rit = n.rpi * (k->ppt ? k->ppt : 1);
    rpb = (rpb + rit - 1) / rit * rit;
    n.rows_per_block = (int)rpb;
    pl.family = WgradFamily::Narrow;
    pl.P = (int)((total_rows + rpb - 1) / rpb);
    pl.part_floats = (long long)pl.P * d->M * pl.Q;
    return true;
}

// APAMD_WGRAD_BLOCKS (tuning / test knob) in place of a family's own workgroup target; `tell`: never silent
static int wgrad_block_target(int own, bool tell) {
    const int forced = env_int("APAMD_WGRAD_BLOCKS", INT_MIN);
    if (forced == INT_MIN) return own;
    static std::atomic<bool> told{false};
    if (tell && !told.exchange(true)) fprintf(stderr, "libapamd: APAMD_WGRAD_BLOCKS=%d overrides the workgroup count\n", forced);
    return forced;
}

// which layer the bf16 GEMM kernel sees (Kb / Cb / Hb / Wb), or false: the layer is not on the bf16 matrix pipe
static bool bf16_gemm_view(const ap_wgrad_desc* d, const WgradPlan& pl, Bf16GemmPlan& b) {
    const int S = d->stride, K = d->K;
    const bool no_bf = env_int("APAMD_NO_BF16X3", 0) != 0;
    const bool bf_ok = d->precision != AP_PRECISION_FP32 && d->M >= 48 && !no_bf;
    b.Kb = K; b.Cb = pl.Cin; b.Hb = d->H; b.Wb = d->W;
    // stride-2 3x3 / 4x4 pad-1 layers (the generator's encoder, the PatchGAN body): the space-to-depth form -- a 2 x 2
    // stride-1 layer over 4 Cin channels -- runs on the same bf16 GEMM kernel (16x the fp32 MFMA rate per product; a
    // 3x3 layer carries 7 of 16 all-zero taps along)
    b.s2d = bf_ok && S == 2 && (K == 3 || K == 4) && d->pad == 1 && d->pad_mode == AP_PAD_ZERO && pl.Cin >= 8 &&
            d->H % 2 == 0 && d->W % 2 == 0 && !env_int("APAMD_NO_S2D_WGRAD", 0);
    if (b.s2d) { b.Kb = 2; b.Cb = 4 * pl.Cin; b.Hb = d->H / 2 + 1; b.Wb = d->W / 2 + 1; }
    // 7x7 stems on a few channels (the generator's three input layers): the row form -- a 1 x 7 layer over 7 Cin channels -- as the
    // forward pass runs them (ap_split_prepass_rows); one 64-channel tile holds up to 9 input channels
    // OPT-IN (APAMD_ROWS_WGRAD=1), plain-bf16 arithmetic only.  Measured in the train step at 2B = 32 (profiles/r05_wgrad_routes.md):
    // the kernel itself takes 125 us, but both operands have to be prepared for this one launch -- the 64-channel gradient at
    // 256 x 256 into pixel-octet slots (~140 us) and the row view padded from 21 to the kernel's 64 channels (~210 us, 277 MB
    // written) -- so the whole operator is ~470 us and 1.1 GB more HBM traffic per stem against 433 us on the fp32 kernel (and ~680 us
    // with three products and both parts).  Kept for the tests and as the starting point of a 32-channel tile.
    b.rows = d->precision == AP_PRECISION_BF16 && d->M >= 24 && !no_bf && env_int("APAMD_ROWS_WGRAD", 0) && S == 1 && K == 7 &&
             d->pad == 3 && d->nsrc == 1 && pl.Cin * 7 <= 64;
    if (b.rows) b.Cb = 7 * pl.Cin;
    if (!(b.s2d || b.rows || (bf_ok && S == 1 && (K == 3 || K == 4) && pl.Cin >= 32))) return false;
    // split-bf16 arithmetic on 128-output multiples: the 8-wave workgroup (two waves per SIMD where the 4-wave one, whose
    // head + tail stages fill the LDS, has one)
    // (plain bf16 keeps two 4-wave workgroups per CU: the 8-wave form measured the same, 160.9 against 160.0 us per 3x3 layer)
    b.wide = d->precision == AP_PRECISION_BF16X3 && !b.rows && b.Kb <= 3 && d->M % 128 == 0;
    return true;
}

// wide layer: operands split into bf16 head + tail, bf16 matrix pipe (wgrad_bf16x3.h)
static bool plan_bf16_gemm(const ap_wgrad_desc* d, WgradPlan& pl) {
    Bf16GemmPlan& b = pl.bf;
    if (!bf16_gemm_view(d, pl, b)) return false;
    pl.family = WgradFamily::Bf16Gemm;
    pl.tiles_x = (d->GW + 31) / 32;
    pl.tiles_y = (d->GH + 1) / 2;
    pl.nstages = d->N * pl.tiles_y * pl.tiles_x;
    const int mtile = b.wide ? 128 : 64;
    pl.m_tiles = (d->M + mtile - 1) / mtile;
    b.c_tiles = (b.Cb + 63) / 64;
    // one workgroup per CU (its LDS stages fill a CU); two with head-only staging
    const bool two_per_cu = d->precision == AP_PRECISION_BF16 && (b.Kb <= 3 || b.rows) && !b.wide;
    int P = wgrad_block_target(num_cus() * (two_per_cu ? 2 : 1), true) / (pl.m_tiles * b.c_tiles);
    if (P > pl.nstages / 2) P = pl.nstages / 2;
    if (P < 1) P = 1;
    pl.P = P;
    b.Mp = pl.m_tiles * mtile;
    b.Cp = b.c_tiles * 64;
    b.GHp = pl.tiles_y * 2;
    b.GX8 = pl.tiles_x * 4;
    b.Hp = b.rows ? b.GHp : b.GHp + b.Kb - 1;
    b.AX8 = pl.tiles_x * 4 + 1;
    b.taps = b.rows ? b.Kb : b.Kb * b.Kb;
    b.sum_floats = (long long)pl.m_tiles * b.c_tiles * (b.wide ? 8 : 4) * b.taps * 1024;
    pl.a_floats = (long long)d->N * 2 * b.Hp * b.AX8 * b.Cp * 4;      // 16-byte slots -> floats
    pl.g_floats = (long long)d->N * 2 * b.GHp * b.GX8 * b.Mp * 4;
    pl.part_floats = pl.P * b.sum_floats;
    return true;
}

static void plan_igemm(const ap_wgrad_desc* d, WgradPlan& pl) {
    IgemmPlan& g = pl.ig;
    const int S = d->stride, K = d->K, PR = pl.k->PR;
    pl.family = WgradFamily::Igemm;
    pl.tiles_x = (d->GW + 31) / 32;
    pl.tiles_y = (d->GH + PR - 1) / PR;
    pl.nstages = d->N * pl.tiles_y * pl.tiles_x;
    pl.m_tiles = (d->M + pl.k->M_TILE - 1) / pl.k->M_TILE;
    g.q_tiles = (pl.Q + pl.k->Q_TILE - 1) / pl.k->Q_TILE;
    int P = (wgrad_block_target(1024, false) + pl.m_tiles * g.q_tiles - 1) / (pl.m_tiles * g.q_tiles);
    if (P > pl.nstages) P = pl.nstages;
    if (P < 1) P = 1;
    pl.P = P;
    g.GHp = pl.tiles_y * PR;
    g.GWp = pl.tiles_x * 32;
    g.Hp = (g.GHp - 1) * S + K;
    g.Wp = (int)round4((long long)(g.GWp - 1) * S + K);
    // every padded row/plane the kernel can touch must exist
    if (g.Hp < d->H + 2 * d->pad) g.Hp = d->H + 2 * d->pad;
    if (g.Wp < d->W + 2 * d->pad) g.Wp = (int)round4(d->W + 2 * d->pad);
    g.g_direct = d->g.mean == nullptr && d->g.act == AP_ACT_NONE && g.GHp == d->GH && g.GWp == d->GW;
    pl.a_floats = round4((long long)d->N * pl.Cin * g.Hp * g.Wp);
    pl.g_floats = g.g_direct ? 0 : round4((long long)d->N * d->M * g.GHp * g.GWp);
    pl.part_floats = (long long)pl.P * d->M * pl.Q;
}

static int make_wgrad_plan(const ap_wgrad_desc* d, WgradPlan& pl) {
    int rc = check_wgrad_desc(d, pl);
    if (rc) return rc;
    if (!plan_narrow(d, pl) && !plan_bf16_gemm(d, pl)) plan_igemm(d, pl);
    return AP_OK;
}

// ------------------------------------------------------------------ the forward pass's split copies as operands
// can the forward pass's split copies the descriptor carries serve as the shifted operand of this plan?
static bool xs_copies_serve(const ap_wgrad_desc* d, const WgradPlan& pl) {
    if (!pl.bf16_gemm() || pl.bf.rows) return false;
    if (d->precision != AP_PRECISION_BF16 && d->xs_parts != 2) return false;      // a split-bf16 product reads the tail planes
    if (d->xs_parts != 1 && d->xs_parts != 2) return false;
    // the space-to-depth form: the forward pass's space-to-depth copy, or the plain one (the view is then gathered from it)
    if (pl.bf.s2d) return (d->src_xs_s2d != nullptr || d->src_xs[0] != nullptr) && d->nsrc == 1 && pl.Cin % 8 == 0;
    for (int s = 0; s < d->nsrc; ++s)
        if (!d->src_xs[s] || d->src[s].C % 8 != 0) return false;
    return true;
}

// ... re-tiled into the kernel's layout (xs_transpose_kernel) in place of normalising + splitting the fp32 tensors again
static bool wgrad_xs_route(const ap_wgrad_desc* d, const WgradPlan& pl) {
    return xs_copies_serve(d, pl) && !env_int("APAMD_NO_XS_WGRAD", 0);
}

// (the kernels index a copy's 16-byte slots with 32 bits)
static bool xs_slots_fit(int N, int C, int H, int W) { return (long long)N * 2 * (C / 8) * ((long long)H * W + 1) < (1LL << 31); }

// ... both operands straight from the split copies (wgrad_xs.h): no operand preparation at all
static bool wgrad_xs_direct_ok(const ap_wgrad_desc* d, const WgradPlan& pl) {
    if (!xs_copies_serve(d, pl) || env_int("APAMD_NO_XS_DIRECT", 0) || d->M % 8 != 0) return false;
    const bool split = d->precision == AP_PRECISION_BF16X3;
    if (!xs_slots_fit(d->N, d->M, d->GH, d->GW)) return false;
    // the 2 x 2 layer over the space-to-depth view (split-bf16 only)
    if (pl.bf.s2d) return split && xs_slots_fit(d->N, pl.bf.Cb, pl.bf.Hb, pl.bf.Wb);
    // 3x3, and (split bf16) the PatchGAN's 4x4 stride-1 layers: 16 accumulator tiles, the 4-wave workgroup, one per CU
    if (d->stride != 1 || !(d->K == 3 || (d->K == 4 && split))) return false;
    for (int s = 0; s < d->nsrc; ++s)
        if (!xs_slots_fit(d->N, d->src[s].C, d->H, d->W)) return false;
    return true;
}

// ------------------------------------------------------------------ operand passes
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

// which of the four operand-preparation kernels re-tiles an operand (launch_split_transpose launches it, ap_conv2d_wgrad_route names
// it), or one of the two refusals.  any_b16: a segment holds bf16 values (ap_src.act bit 8); W: the source's width
enum SplitTForm { ST_GENERAL, ST_VEC, ST_PAD_ROWS, ST_S2D_ROWS, ST_NO_ROW_VIEW = -1, ST_B16_NEEDS_PAD_ROWS = -2 };
static bool split_transpose_whole_rows(int W, int s2d_c) { return W == 64 || W == 128 || W == 256 || (W == 32 && s2d_c == 0); }
static int split_transpose_form(int nseg, bool any_b16, int C, int W, int pad, int X8, int Cp, int s2d_c, int rows_k) {
    const bool whole_rows = split_transpose_whole_rows(W, s2d_c);
    const bool pad_rows = whole_rows && s2d_c == 0 && pad == 1;
    if (rows_k > 0) return (any_b16 || s2d_c) ? ST_NO_ROW_VIEW : ST_GENERAL;      // the row view exists in the general kernel only
    if (any_b16 && !pad_rows) return ST_B16_NEEDS_PAD_ROWS;
    if (nseg == 1 && pad == 0 && s2d_c == 0 && X8 * 8 == W) return ST_VEC;
    if (pad_rows) return ST_PAD_ROWS;
    if (whole_rows && s2d_c > 0 && s2d_c % 32 == 0 && nseg == 1 && C == 4 * s2d_c && Cp == C) return ST_S2D_ROWS;
    return ST_GENERAL;
}
static int split_transpose_refusal(int form) {
    if (form == ST_NO_ROW_VIEW) return fail(AP_ERR_UNSUPPORTED, "split_transpose: row view of a bf16 / space-to-depth source");
    return fail(AP_ERR_UNSUPPORTED, "split_transpose: a bf16 source needs the padded-row form (pad 1, W in {32, 64, 128, 256})");
}
static bool any_bf16_segment(const ap_src* segs, int nseg) {
    for (int s = 0; s < nseg; ++s)
        if ((segs[s].act >> 8) & 1) return true;
    return false;
}

static int launch_split_transpose(const ap_src* segs, int nseg, int N, int C, int H, int W, int pad, int pad_mode,
                                  int Hp, int X8, int Cp, uint4* out, hipStream_t stream, int s2d_c, int heads_only, int rows_k = 0) {
    SplitTParams p;
    memset(&p, 0, sizeof(p));
    p.nseg = nseg;
    int cbeg = 0;
    for (int s = 0; s < nseg; ++s) {
        fill_seg(p.seg[s], segs[s], cbeg);
        // ap_src.act bit 8: the segment's data are bf16 values (a raw output of ap_conv2d_fwd_bf16out); only the padded-row kernel reads those
        p.seg[s].act = segs[s].act & 0xff;
        p.seg[s].pad_ = (segs[s].act >> 8) & 1;
        cbeg += segs[s].C;
    }
    p.N = N; p.C = C; p.H = H; p.W = W; p.pad = pad; p.pad_mode = pad_mode; p.Hp = Hp; p.X8 = X8; p.Cp = Cp; p.out = out;
    p.s2d_c = s2d_c;
    p.heads_only = heads_only;
    p.rows_k = rows_k;
    const bool whole_rows = split_transpose_whole_rows(W, s2d_c);
    const int form = split_transpose_form(nseg, any_bf16_segment(segs, nseg), C, W, pad, X8, Cp, s2d_c, rows_k);
    if (form < 0) return split_transpose_refusal(form);
    if (N > 65535 || Cp / 64 > 65535) return fail(AP_ERR_UNSUPPORTED, "split_transpose: N=%d C=%d", N, C);
    const int R = whole_rows ? 256 / W : 1;                                       // source rows per workgroup of the row forms
    const size_t row_lds = (size_t)64 * (R * X8 * 8 + 1) * sizeof(float);
    int rc = AP_OK;
    switch (form) {
    case ST_VEC: {      // unpadded operand with whole octet rows: 16-byte loads, 1 KiB per wave
        const size_t lds = 64 * 257 * sizeof(float);
        if ((rc = ensure_dyn_lds(reinterpret_cast<const void*>(&split_transpose_vec_kernel), (int)lds))) return rc;
        hipLaunchKernelGGL(split_transpose_vec_kernel, dim3((Hp * X8 + 31) / 32, Cp / 64, N), dim3(256), lds, stream, p);
        return check_launch("split_transpose_vec_kernel");
    }
    case ST_PAD_ROWS:   // padded rows, 16-byte loads
        if ((rc = ensure_dyn_lds(reinterpret_cast<const void*>(&split_transpose_pad_kernel), 96 * 1024))) return rc;
        hipLaunchKernelGGL(split_transpose_pad_kernel, dim3((Hp + R - 1) / R, Cp / 64, N), dim3(256), row_lds, stream, p);
        return check_launch("split_transpose_pad_kernel");
    case ST_S2D_ROWS:   // space-to-depth view, whole source rows
        if ((rc = ensure_dyn_lds(reinterpret_cast<const void*>(&split_transpose_s2d_kernel), 96 * 1024))) return rc;
        hipLaunchKernelGGL(split_transpose_s2d_kernel, dim3(((Hp + R - 1) / R) * 2, s2d_c / 32, N), dim3(256), row_lds, stream, p);
        return check_launch("split_transpose_s2d_kernel");
    default:
        hipLaunchKernelGGL(split_transpose_kernel, dim3((Hp * X8 + 7) / 8, Cp / 64, N), dim3(256), 0, stream, p);
        return check_launch("split_transpose_kernel");
    }
}

// the shifted operand re-tiled from the forward pass's split copies (xs_transpose_kernel); C = channels of the view
static int launch_xs_transpose(const void* const* xs, const int* seg_c, int nseg, int N, int H, int W, int pad, int pad_mode,
                               int Hp, int X8, int Cp, int parts, uint4* out, hipStream_t stream, int s2d_c = 0, int H0 = 0, int W0 = 0) {
    XsTParams p;
    memset(&p, 0, sizeof(p));
    p.nseg = nseg;
    int cg = 0;
    for (int s = 0; s < nseg; ++s) {
        p.xs[s] = reinterpret_cast<const uint4*>(xs[s]);
        p.cg_begin[s] = cg;
        cg += seg_c[s] / 8;
    }
    p.cg_begin[nseg] = cg;
    p.N = N; p.H = H; p.W = W; p.pad = pad; p.pad_mode = pad_mode; p.Hp = Hp; p.X8 = X8; p.Cp = Cp; p.parts = parts; p.out = out;
    p.s2d_c = s2d_c; p.H0 = H0; p.W0 = W0;
    if (N > 65535 || Cp / 8 > 65535) return fail(AP_ERR_UNSUPPORTED, "xs_transpose: N=%d Cp=%d", N, Cp);
    hipLaunchKernelGGL(xs_transpose_kernel, dim3((Hp * X8 + 31) / 32, (Cp / 8 + kXsCgPerThread - 1) / kXsCgPerThread, N), dim3(256), 0,
                       stream, p);
    return check_launch("xs_transpose_kernel");
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

// the shifted operand of a bf16 GEMM plan in pixel-octet slots: from the forward pass's split copies or from the fp32 tensors
static int launch_bf16_gemm_operand(const ap_wgrad_desc* d, const WgradPlan& pl, bool from_xs, uint4* at, hipStream_t stream) {
    const Bf16GemmPlan& b = pl.bf;
    const bool b16 = d->precision == AP_PRECISION_BF16;
    if (!from_xs)
        return launch_split_transpose(d->src, d->nsrc, d->N, b.Cb, d->H, d->W, b.s2d ? 0 : d->pad, d->pad_mode, b.Hp, b.AX8, b.Cp, at,
                                      stream, b.s2d ? pl.Cin : 0, b16, b.rows ? b.Kb : 0);
    const int parts = b16 ? 1 : 2;
    if (b.s2d) {
        // the forward pass staged the space-to-depth copy (2 x 2 form) or, where it ran the stride-2 kernel, the plain one
        const void* xs[1] = {d->src_xs_s2d ? d->src_xs_s2d : d->src_xs[0]};
        const int cs[1] = {b.Cb};
        return launch_xs_transpose(xs, cs, 1, d->N, b.Hb, b.Wb, 0, AP_PAD_ZERO, b.Hp, b.AX8, b.Cp, parts, at, stream,
                                   d->src_xs_s2d ? 0 : pl.Cin, d->H, d->W);
    }
    int cs[kMaxSeg];
    for (int s = 0; s < d->nsrc; ++s) cs[s] = d->src[s].C;
    return launch_xs_transpose(d->src_xs, cs, d->nsrc, d->N, d->H, d->W, d->pad, d->pad_mode, b.Hp, b.AX8, b.Cp, parts, at, stream);
}

// the kernel table entry of a bf16 GEMM plan (b16: plain-bf16 arithmetic)
static const WgradBf3Kernel* bf3_kernel(const Bf16GemmPlan& b, bool b16) {
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
    p.ablate = env_int("APAMD_ABLATE", 0);
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
    p.ablate = env_int("APAMD_ABLATE", 0);
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
struct WgradXsKernel {
    int Kb, parts, wm;
    int (*launch)(const WgradXsParams&, unsigned, hipStream_t);
};
static const WgradXsKernel kWgradXsKernels[] = {
    {2, 2, 2, &launch_wgrad_xs<WgradXsCfg<2, 2, 2>>}, {2, 2, 4, &launch_wgrad_xs<WgradXsCfg<2, 2, 4>>},
    {3, 1, 2, &launch_wgrad_xs<WgradXsCfg<3, 1, 2>>}, {3, 2, 2, &launch_wgrad_xs<WgradXsCfg<3, 2, 2>>},
    {3, 2, 4, &launch_wgrad_xs<WgradXsCfg<3, 2, 4>>}, {4, 2, 2, &launch_wgrad_xs<WgradXsCfg<4, 2, 2>>},
};
static const WgradXsKernel* xs_kernel(const ap_wgrad_desc* d, const Bf16GemmPlan& b) {
    const int parts = d->precision == AP_PRECISION_BF16 ? 1 : 2, wm = b.wide ? 4 : 2;
    const WgradXsKernel* k = nullptr;
    for (const auto& c : kWgradXsKernels)
        if (c.Kb == b.Kb && c.parts == parts && c.wm == wm) k = &c;
    return k;
}

// ------------------------------------------------------------------ the plan as text (ap_conv2d_wgrad_route)
// how an operand reaches its kernel: through one of the four split_transpose kernels (by SplitTForm), re-tiled from the forward pass's
// split copies, padded in fp32 for the igemm kernel, read where it lies, or not at all (the caller brings it)
static const char* const kSplitTForms[] = {"general", "vec", "pad_rows", "s2d_rows"};
static const char* const kOtherForms[] = {"xs_transpose", "pad", "direct", "none"};
static const char* const kBf3Forms[] = {"split", "heads", "wide"};

static void bf3_name(const WgradBf3Kernel& k, char* out, int n) {
    // K = 2 is only ever the space-to-depth view, K = 7 the row view (kWgradBf3Kernels)
    snprintf(out, n, "bf16gemm<%d,%s>%s", k.K, kBf3Forms[k.form], k.K == 2 ? "+s2d" : (k.K == 7 ? "+rows" : ""));
}

// what wgrad_impl would launch for this descriptor, from the same plan: nothing is launched, no pointer is followed
static int wgrad_route_text(const ap_wgrad_desc* d, char* buf, int n) {
    WgradPlan pl;
    int rc = make_wgrad_plan(d, pl);
    if (rc) return rc;
    if (!buf || n < 1) return fail(AP_ERR_INVALID, "wgrad_route: bad buffer");
    char kernel[64], xs[32] = "";
    const char *g = "direct", *a = "direct";
    switch (pl.family) {
    case WgradFamily::Narrow:
        snprintf(kernel, sizeof(kernel), "narrow<%d,%d,%d,%d>", pl.narrow.k->K, pl.narrow.k->S, pl.narrow.k->Cin, pl.narrow.k->ppt);
        break;
    case WgradFamily::Bf16Gemm: {
        const Bf16GemmPlan& b = pl.bf;
        const WgradBf3Kernel* k = bf3_kernel(b, d->precision == AP_PRECISION_BF16);
        if (!k) return fail(AP_ERR_UNSUPPORTED, b.wide ? "wgrad: no 8-wave kernel for k=%d" : "wgrad: no split-bf16 kernel for k=%d", b.Kb);
        bf3_name(*k, kernel, sizeof(kernel));
        // (the arguments of launch_bf16_gemm's two launch_split_transpose calls)
        // no gradient tensor: the caller brings that operand prepared (ap_conv2d_wgrad_pre) or as a split copy (ap_conv2d_wgrad_xs)
        const bool a_xs = wgrad_xs_route(d, pl), g_own = d->g.data != nullptr;
        int fa = ST_GENERAL, fg = ST_GENERAL;
        if (!a_xs)
            fa = split_transpose_form(d->nsrc, any_bf16_segment(d->src, d->nsrc), b.Cb, d->W, b.s2d ? 0 : d->pad, b.AX8, b.Cp,
                                      b.s2d ? pl.Cin : 0, b.rows ? b.Kb : 0);
        if (g_own) fg = split_transpose_form(1, any_bf16_segment(&d->g, 1), d->M, d->GW, 0, b.GX8, b.Mp, 0, 0);
        if (fa < 0 || fg < 0) return split_transpose_refusal(fa < 0 ? fa : fg);
        a = a_xs ? "xs_transpose" : kSplitTForms[fa];
        g = g_own ? kSplitTForms[fg] : "none";
        if (wgrad_xs_direct_ok(d, pl))
            if (const WgradXsKernel* x = xs_kernel(d, b)) snprintf(xs, sizeof(xs), " xs<%d,%d,%d>", x->Kb, x->parts, x->wm);
        break;
    }
    default:
        snprintf(kernel, sizeof(kernel), "igemm<%d,%d,%d,%d,%d>", pl.k->S, pl.k->K, pl.k->M_TILE, pl.k->Q_TILE, pl.k->PR);
        a = "pad";
        g = pl.ig.g_direct ? "direct" : "pad";
    }
    snprintf(buf, n, "%s g=%s a=%s P=%d nstages=%d%s", kernel, g, a, pl.P, pl.nstages, xs);
    return AP_OK;
}

// every kernel table entry and operand form ap_conv2d_wgrad_route can name, one per line
static int wgrad_route_names(char* buf, int n) {
    if (!buf || n < 1) return fail(AP_ERR_INVALID, "wgrad_route_names: bad buffer");
    std::string all;
    char name[64];
    for (const auto& k : kWgradNarrowKernels) {
        snprintf(name, sizeof(name), "narrow<%d,%d,%d,%d>\n", k.K, k.S, k.Cin, k.ppt);
        all += name;
    }
    for (const auto& k : kWgradBf3Kernels) {
        bf3_name(k, name, sizeof(name));
        all += name;
        all += "\n";
    }
    for (const auto& k : kWgradKernels) {
        snprintf(name, sizeof(name), "igemm<%d,%d,%d,%d,%d>\n", k.S, k.K, k.M_TILE, k.Q_TILE, k.PR);
        all += name;
    }
    for (const auto& k : kWgradXsKernels) {
        snprintf(name, sizeof(name), "xs<%d,%d,%d>\n", k.Kb, k.parts, k.wm);
        all += name;
    }
    for (const char* f : kSplitTForms) all += std::string(f) + "\n";
    for (const char* f : kOtherForms) all += std::string(f) + "\n";
    snprintf(buf, n, "%s", all.c_str());
    return (int)all.size() < n ? AP_OK : fail(AP_ERR_INVALID, "wgrad_route_names: %d bytes needed", (int)all.size() + 1);
}

// ------------------------------------------------------------------ the 7x7 edge layers and the PatchGAN's first layer (wgrad_k7.h)
struct K7Plan {
    int MT, NT, R, A, NW, RB, bpi, grid;
    long long narrow_floats, part_floats;
    size_t lds;
};
// the part both forms share, after MT / NT / R / A / NW: the row split, the workspace and the LDS of a workgroup;
// nrows = narrow rows in LDS per image row (channels x copies)
static void k7_plan_finish(K7Plan& k, int N, int nrows) {
    const RowSplit rs = split_rows(N, k.R, true);
    k.RB = rs.RB; k.bpi = rs.bpi; k.grid = rs.grid;
    k.narrow_floats = round4(((long long)N * nrows * k.A * k.NW + 1) / 2);
    k.part_floats = (long long)k.grid * k.MT * k.NT * 1024;
    const size_t tiles = (size_t)k.MT * 32 * ((k.NW - 8) * 2 + 16) + (size_t)8 * nrows * (k.NW + 8) * 2;
    const size_t red = (size_t)k.MT * k.NT * 16 * 64 * 4;
    k.lds = std::max(tiles, red);
}

static bool k7_plan(int N, int MW, int CN, int H, int W, int final_form, K7Plan& k) {
    if (N < 1 || H < 4 || W < 16 || W > 256 || (W & 15) || (MW != 32 && MW != 64)) return false;
    if (final_form ? CN != 1 : (CN != 1 && CN != 3)) return false;
    k.MT = MW / 32;
    k.NT = (CN * 49 + 31) / 32;
    k.R = final_form ? H + 6 : H;
    k.A = k.R + 6;
    k.NW = W + 16;
    k7_plan_finish(k, N, CN * 2);
    return true;
}

// weight gradient of the PatchGAN's first layer: form 2 of the same kernel (wide = the output gradient [N][64][H/2][W/2])
static bool d0w_plan(int N, int M, int Cin, int H, int W, K7Plan& k) {
    if (N < 1 || M != 64 || (Cin != 1 && Cin != 2) || H < 2 || (H & 1) || W < 32 || W > 512 || (W & 31)) return false;
    const int OH = H / 2, OW = W / 2;                              // OW: a multiple of 16 in 16..256
    // the ring's two new rows per tile are fetched with at most two 16-byte loads per thread (wgrad_k7.h, NQ)
    if (Cin * 4 * ((OW + 16) / 8) * 2 > 512) return false;
    k.MT = 2;
    k.NT = 1;
    k.R = OH;
    k.A = H + 2;
    k.NW = OW + 16;
    k7_plan_finish(k, N, Cin * 4);
    return true;
}

// wgrad_k7_kernel<MT, NT, FORM, WB16> by (MT, NT, form, a bf16-stored wide operand); form 0: a stem, 1: the last layer, 2: d0
struct K7Kernel {
    int MT, NT, form;
    bool b16;
    const void* fn;
};
#define APAMD_K7(MT, NT, FORM, B16) {MT, NT, FORM, B16, reinterpret_cast<const void*>(&wgrad_k7_kernel<MT, NT, FORM, B16>)}
static const K7Kernel kK7Kernels[] = {
    APAMD_K7(1, 2, 1, false), APAMD_K7(2, 2, 1, false),
    APAMD_K7(1, 2, 0, false), APAMD_K7(2, 2, 0, false), APAMD_K7(1, 2, 0, true), APAMD_K7(2, 2, 0, true),
    APAMD_K7(1, 5, 0, false), APAMD_K7(2, 5, 0, false), APAMD_K7(1, 5, 0, true), APAMD_K7(2, 5, 0, true),
    APAMD_K7(2, 1, 2, false),
};
#undef APAMD_K7

// the main kernel of a K7Plan over the prepared narrow operand, and the sum of its workgroups' partial tiles
static int launch_k7(const K7Plan& k, WgradK7Params& p, int form, bool b16, float* workspace, float* dw, hipStream_t stream) {
    p.narrow = reinterpret_cast<const unsigned short*>(workspace);
    p.R = k.R; p.A = k.A; p.NW = k.NW; p.RB = k.RB; p.blocks_per_img = k.bpi;
    p.partial = workspace + k.narrow_floats;
    const void* fn = nullptr;
    for (const auto& c : kK7Kernels)
        if (c.MT == k.MT && c.NT == k.NT && c.form == form && c.b16 == b16) fn = c.fn;
    if (!fn) return fail(AP_ERR_UNSUPPORTED, "wgrad_k7: no kernel for tiles %d x %d, form %d", k.MT, k.NT, form);
    int rc = ensure_dyn_lds(fn, 160 * 1024);
    if (rc) return rc;
    void* args[] = {&p};
    hipError_t e = hipLaunchKernel(fn, dim3(k.grid), dim3(256), args, k.lds, stream);
    if (e != hipSuccess) return fail(AP_ERR_LAUNCH, "%s launch: %s", form == 2 ? "wgrad_d0" : "wgrad_k7", hipGetErrorString(e));
    const int total = k.MT * k.NT * 1024;
    hipLaunchKernelGGL(wgrad_k7_reduce_kernel, dim3(total / 64), dim3(256), 0, stream, p.partial, k.grid, total, k.NT, p.MW, p.CN,
                       form == 1 ? 1 : 0, dw, form == 2 ? 16 : 49);
    return check_launch("wgrad_k7_reduce_kernel");
}

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

int64_t ap_conv2d_wgrad_workspace_floats(const ap_wgrad_desc* d) {
    WgradPlan pl;
    int rc = make_wgrad_plan(d, pl);
    if (rc) return rc;
    return pl.a_floats + pl.g_floats + pl.part_floats;
}

int ap_conv2d_wgrad_gt_dims(const ap_wgrad_desc* d, int32_t* dims) {
    WgradPlan pl;
    int rc = make_wgrad_plan(d, pl);
    if (rc) return rc;
    if (!dims) return fail(AP_ERR_INVALID, "wgrad_gt_dims: null pointer");
    if (!pl.bf16_gemm()) return 0;
    dims[0] = pl.bf.GHp; dims[1] = pl.bf.GX8; dims[2] = pl.bf.Mp;
    return 1;
}

int ap_conv2d_wgrad_route(const ap_wgrad_desc* d, char* buf, int32_t buflen) { return wgrad_route_text(d, buf, buflen); }

int ap_conv2d_wgrad_route_names(char* buf, int32_t buflen) { return wgrad_route_names(buf, buflen); }

int ap_conv2d_wgrad(const ap_wgrad_desc* d, float* workspace, float* dw, ap_stream_t stream) {
    return wgrad_impl(d, nullptr, workspace, dw, stream);
}

int ap_conv2d_wgrad_pre(const ap_wgrad_desc* d, const void* g_t, float* workspace, float* dw, ap_stream_t stream) {
    if (!g_t) return fail(AP_ERR_INVALID, "wgrad_pre: null operand");
    return wgrad_impl(d, g_t, workspace, dw, stream);
}

int32_t ap_conv2d_wgrad_xs_ok(const ap_wgrad_desc* d) {
    WgradPlan pl;
    if (make_wgrad_plan(d, pl)) return 0;
    return wgrad_xs_direct_ok(d, pl) ? 1 : 0;
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

int ap_conv_head_wgrad(const ap_src* src, const float* g, int32_t N, int32_t H, int32_t W, int32_t K, int32_t pad,
                       float* dw, ap_stream_t stream) {
    if (!src || !src->data || !g || !dw) return fail(AP_ERR_INVALID, "conv_head_wgrad: null pointer");
    if ((src->mean == nullptr) != (src->rstd == nullptr)) return fail(AP_ERR_INVALID, "conv_head_wgrad: mean/rstd mismatch");
    const int OH = H + 2 * pad - K + 1, OW = W + 2 * pad - K + 1;
    if (K != 4 || pad != 1 || N < 1 || src->C < 1 || src->C > 65535 || OH < 1 || OW < 1 || W > kHeadMaxW || H > kHeadMaxH)
        return fail(AP_ERR_UNSUPPORTED, "conv_head_wgrad: built for 4x4 pad-1 heads on maps up to %dx%d (K=%d, pad=%d, %dx%d)",
                    kHeadMaxH, kHeadMaxW, K, pad, H, W);
    HeadParams p;
    memset(&p, 0, sizeof(p));
    fill_seg(p.src, *src, 0);
    p.N = N; p.C = src->C; p.H = H; p.W = W; p.OH = OH; p.OW = OW;
    p.g = g; p.dw = dw;
    hipLaunchKernelGGL(conv_head_wgrad_kernel, dim3(src->C), dim3(256), 0, (hipStream_t)stream, p);
    return check_launch("conv_head_wgrad_kernel");
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

// ---- the 7x7 edge layers at full resolution on the bf16 matrix pipe (wgrad_k7.h; plain-bf16 arithmetic)
int32_t ap_wgrad_k7_bf16_ok(int32_t N, int32_t MW, int32_t CN, int32_t H, int32_t W, int32_t final_form) {
    K7Plan k;
    return k7_plan(N, MW, CN, H, W, final_form, k) ? 1 : 0;
}

int64_t ap_wgrad_k7_bf16_workspace_floats(int32_t N, int32_t MW, int32_t CN, int32_t H, int32_t W, int32_t final_form) {
    K7Plan k;
    if (!k7_plan(N, MW, CN, H, W, final_form, k)) return fail(AP_ERR_UNSUPPORTED, "wgrad_k7_bf16: shape not served (see ap_wgrad_k7_bf16_ok)");
    return k.narrow_floats + k.part_floats;
}

int ap_wgrad_k7_bf16(const ap_src* wide, const ap_src* narrow, int32_t N, int32_t H, int32_t W, int32_t final_form, float* workspace,
                     float* dw, ap_stream_t stream_) {
    if (!wide || !wide->data || !narrow || !narrow->data || !workspace || !dw) return fail(AP_ERR_INVALID, "wgrad_k7_bf16: null pointer");
    if ((wide->mean == nullptr) != (wide->rstd == nullptr)) return fail(AP_ERR_INVALID, "wgrad_k7_bf16: mean/rstd mismatch");
    if (narrow->mean || narrow->rstd || narrow->act != AP_ACT_NONE)
        return fail(AP_ERR_UNSUPPORTED, "wgrad_k7_bf16: the narrow operand must be a plain tensor");
    const bool wb16 = (wide->act & 0x100) != 0;                  // ap_src.act bit 8: the tensor holds bf16 values
    const int wact = wide->act & 0xff;
    if (wact < 0 || wact > 2) return fail(AP_ERR_INVALID, "wgrad_k7_bf16: act %d", wact);
    if (!final_form && (wide->mean || wact != AP_ACT_NONE))
        return fail(AP_ERR_UNSUPPORTED, "wgrad_k7_bf16: the stem form takes a plain gradient");
    if (final_form && wb16) return fail(AP_ERR_UNSUPPORTED, "wgrad_k7_bf16: a bf16-stored wide operand is read in the stem form only");
    K7Plan k;
    if (!k7_plan(N, wide->C, narrow->C, H, W, final_form, k))
        return fail(AP_ERR_UNSUPPORTED, "wgrad_k7_bf16: N=%d wide C=%d narrow C=%d %dx%d form %d not served", N, wide->C, narrow->C, H, W, final_form);
    hipStream_t stream = (hipStream_t)stream_;
    K7NarrowParams np;
    np.src = narrow->data; np.dst = reinterpret_cast<unsigned*>(workspace);
    np.N = N; np.CN = narrow->C; np.H = H; np.W = W; np.A = k.A; np.NW = k.NW; np.final_form = final_form;
    const long long ndw = (long long)N * narrow->C * k.A * (k.NW / 2);
    hipLaunchKernelGGL(wgrad_k7_narrow_kernel, dim3((unsigned)std::min<long long>((ndw + 255) / 256, 4096)), dim3(256), 0, stream, np);
    int rc = check_launch("wgrad_k7_narrow_kernel");
    if (rc) return rc;
    WgradK7Params p;
    memset(&p, 0, sizeof(p));
    p.wide = wide->data; p.wmean = wide->mean; p.wrstd = wide->rstd; p.wact = wact;
    p.N = N; p.MW = wide->C; p.CN = narrow->C; p.H = H; p.W = W;
    return launch_k7(k, p, final_form ? 1 : 0, wb16, workspace, dw, stream);
}

// ---- weight gradient of the PatchGAN's first layer (d0w_plan)
int32_t ap_wgrad_d0_bf16_ok(int32_t N, int32_t M, int32_t Cin, int32_t H, int32_t W) {
    K7Plan k;
    return d0w_plan(N, M, Cin, H, W, k) ? 1 : 0;
}

int64_t ap_wgrad_d0_bf16_workspace_floats(int32_t N, int32_t M, int32_t Cin, int32_t H, int32_t W) {
    K7Plan k;
    if (!d0w_plan(N, M, Cin, H, W, k)) return fail(AP_ERR_UNSUPPORTED, "wgrad_d0_bf16: shape not served (see ap_wgrad_d0_bf16_ok)");
    return k.narrow_floats + k.part_floats;
}

int ap_wgrad_d0_bf16(const float* g, const float* x, int32_t N, int32_t M, int32_t Cin, int32_t H, int32_t W, float* workspace, float* dw,
                     ap_stream_t stream_) {
    if (!g || !x || !workspace || !dw) return fail(AP_ERR_INVALID, "wgrad_d0_bf16: null pointer");
    K7Plan k;
    if (!d0w_plan(N, M, Cin, H, W, k))
        return fail(AP_ERR_UNSUPPORTED, "wgrad_d0_bf16: N=%d %d <- %d channels %dx%d not served (1 | 2 -> 64, even H, W a multiple of 32 up to 512)", N, M, Cin, H, W);
    hipStream_t stream = (hipStream_t)stream_;
    K7NarrowParams np;
    np.src = x; np.dst = reinterpret_cast<unsigned*>(workspace);
    np.N = N; np.CN = Cin; np.H = H; np.W = W; np.A = k.A; np.NW = k.NW; np.final_form = 2;
    const long long ndw = (long long)N * Cin * k.A * 2 * (k.NW / 2);
    hipLaunchKernelGGL(wgrad_d0_narrow_kernel, dim3((unsigned)std::min<long long>((ndw + 255) / 256, 4096)), dim3(256), 0, stream, np);
    int rc = check_launch("wgrad_d0_narrow_kernel");
    if (rc) return rc;
    WgradK7Params p;
    memset(&p, 0, sizeof(p));
    p.wide = g;
    p.N = N; p.MW = M; p.CN = Cin; p.H = H / 2; p.W = W / 2;
    return launch_k7(k, p, 2, false, workspace, dw, stream);
}

}  // extern "C"
