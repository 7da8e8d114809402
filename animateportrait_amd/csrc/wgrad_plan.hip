// wgrad_plan.hip -- the weight-gradient planner and its queries.  make_wgrad_plan puts a layer into one of three families:
//   narrow     1..2 input channels: one streaming pass over the fp32 tensors (wgrad_narrow.h)
//   bf16 GEMM  both operands in bf16 pixel-octet slots on the matrix pipe (wgrad_bf16x3.h); a stride-2 layer runs as its
//              space-to-depth view, a 7x7 stem (opt-in) as its row view, 128-output multiples on the 8-wave workgroup
//   igemm      exact fp32 (wgrad_igemm.h)
// and sizes the caller's ONE workspace, laid out  [A prepared][G prepared (optional)][partials].  ap_conv2d_wgrad_route states the
// plan as text.  Launches nothing and includes no kernel header: the kernel tables are read through wgrad_plan.h's accessors.
#include "wgrad_plan.h"

#include <algorithm>
#include <atomic>
#include <string>

namespace apamd {

// several tile shapes of a family: the one whose padded (M x Q) tile grid wastes least (the 7x7 stems are
// M = 32..64 by Q = 147: 64 x 192 tiles are 77 % full where 128 x 256 ones are 29 %)
static const WgradKernel* pick_igemm_tile(const ap_wgrad_desc* d) {
    int cin = 0;
    for (int s = 0; s < d->nsrc; ++s) cin += d->src[s].C;
    const long long Q = (long long)cin * d->K * d->K;
    const WgradKernel* pick = nullptr;
    long long best = -1;
    for (const auto& k : wgrad_igemm_kernels())
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
    const int forced = sw(SW_WGRAD_BLOCKS);
    if (!forced) return own;
    static std::atomic<bool> told{false};
    if (tell && !told.exchange(true)) fprintf(stderr, "libapamd: APAMD_WGRAD_BLOCKS=%d overrides the workgroup count\n", forced);
    return forced;
}

// which layer the bf16 GEMM kernel sees (Kb / Cb / Hb / Wb), or false: the layer is not on the bf16 matrix pipe
static bool bf16_gemm_view(const ap_wgrad_desc* d, const WgradPlan& pl, Bf16GemmPlan& b) {
    const int S = d->stride, K = d->K;
    const bool no_bf = sw(SW_NO_BF16X3) != 0;
    const bool bf_ok = d->precision != AP_PRECISION_FP32 && d->M >= 48 && !no_bf;
    b.Kb = K; b.Cb = pl.Cin; b.Hb = d->H; b.Wb = d->W;
    // stride-2 3x3 / 4x4 pad-1 layers (the generator's encoder, the PatchGAN body): the space-to-depth form -- a 2 x 2
    // stride-1 layer over 4 Cin channels -- runs on the same bf16 GEMM kernel (16x the fp32 MFMA rate per product; a
    // 3x3 layer carries 7 of 16 all-zero taps along)
    b.s2d = bf_ok && S == 2 && (K == 3 || K == 4) && d->pad == 1 && d->pad_mode == AP_PAD_ZERO && pl.Cin >= 8 &&
            d->H % 2 == 0 && d->W % 2 == 0 && !sw(SW_NO_S2D_WGRAD);
    if (b.s2d) { b.Kb = 2; b.Cb = 4 * pl.Cin; b.Hb = d->H / 2 + 1; b.Wb = d->W / 2 + 1; }
    // 7x7 stems on a few channels (the generator's three input layers): the row form -- a 1 x 7 layer over 7 Cin channels -- as the
    // forward pass runs them (ap_split_prepass_rows); one 64-channel tile holds up to 9 input channels
    // OPT-IN (APAMD_ROWS_WGRAD=1), plain-bf16 arithmetic only.  Measured in the train step at 2B = 32 (profiles/r05_wgrad_routes.md):
    // the kernel itself takes 125 us, but both operands have to be prepared for this one launch -- the 64-channel gradient at
    // 256 x 256 into pixel-octet slots (~140 us) and the row view padded from 21 to the kernel's 64 channels (~210 us, 277 MB
    // written) -- so the whole operator is ~470 us and 1.1 GB more HBM traffic per stem against 433 us on the fp32 kernel (and ~680 us
    // with three products and both parts).  Kept for the tests and as the starting point of a 32-channel tile.
    b.rows = d->precision == AP_PRECISION_BF16 && d->M >= 24 && !no_bf && sw(SW_ROWS_WGRAD) && S == 1 && K == 7 &&
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

int make_wgrad_plan(const ap_wgrad_desc* d, WgradPlan& pl) {
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
bool wgrad_xs_route(const ap_wgrad_desc* d, const WgradPlan& pl) {
    return xs_copies_serve(d, pl) && !sw(SW_NO_XS_WGRAD);
}

// (the kernels index a copy's 16-byte slots with 32 bits)
static bool xs_slots_fit(int N, int C, int H, int W) { return (long long)N * 2 * (C / 8) * ((long long)H * W + 1) < (1LL << 31); }

// ... both operands straight from the split copies (wgrad_xs.h): no operand preparation at all
bool wgrad_xs_direct_ok(const ap_wgrad_desc* d, const WgradPlan& pl) {
    if (!xs_copies_serve(d, pl) || sw(SW_NO_XS_DIRECT) || d->M % 8 != 0) return false;
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

// ------------------------------------------------------------------ the form of an operand pass (SplitTForm)
bool split_transpose_whole_rows(int W, int s2d_c) { return W == 64 || W == 128 || W == 256 || (W == 32 && s2d_c == 0); }
int split_transpose_form(int nseg, bool any_b16, int C, int W, int pad, int X8, int Cp, int s2d_c, int rows_k) {
    const bool whole_rows = split_transpose_whole_rows(W, s2d_c);
    const bool pad_rows = whole_rows && s2d_c == 0 && pad == 1;
    if (rows_k > 0) return (any_b16 || s2d_c) ? ST_NO_ROW_VIEW : ST_GENERAL;      // the row view exists in the general kernel only
    if (any_b16 && !pad_rows) return ST_B16_NEEDS_PAD_ROWS;
    if (nseg == 1 && pad == 0 && s2d_c == 0 && X8 * 8 == W) return ST_VEC;
    if (pad_rows) return ST_PAD_ROWS;
    if (whole_rows && s2d_c > 0 && s2d_c % 32 == 0 && nseg == 1 && C == 4 * s2d_c && Cp == C) return ST_S2D_ROWS;
    return ST_GENERAL;
}
int split_transpose_refusal(int form) {
    if (form == ST_NO_ROW_VIEW) return fail(AP_ERR_UNSUPPORTED, "split_transpose: row view of a bf16 / space-to-depth source");
    return fail(AP_ERR_UNSUPPORTED, "split_transpose: a bf16 source needs the padded-row form (pad 1, W in {32, 64, 128, 256})");
}
bool any_bf16_segment(const ap_src* segs, int nseg) {
    for (int s = 0; s < nseg; ++s)
        if ((segs[s].act >> 8) & 1) return true;
    return false;
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
    for (const auto& k : wgrad_narrow_kernels()) {
        snprintf(name, sizeof(name), "narrow<%d,%d,%d,%d>\n", k.K, k.S, k.Cin, k.ppt);
        all += name;
    }
    for (const auto& k : wgrad_bf3_kernels()) {
        bf3_name(k, name, sizeof(name));
        all += name;
        all += "\n";
    }
    for (const auto& k : wgrad_igemm_kernels()) {
        snprintf(name, sizeof(name), "igemm<%d,%d,%d,%d,%d>\n", k.S, k.K, k.M_TILE, k.Q_TILE, k.PR);
        all += name;
    }
    for (const auto& k : wgrad_xs_kernels()) {
        snprintf(name, sizeof(name), "xs<%d,%d,%d>\n", k.Kb, k.parts, k.wm);
        all += name;
    }
    for (const char* f : kSplitTForms) all += std::string(f) + "\n";
    for (const char* f : kOtherForms) all += std::string(f) + "\n";
    snprintf(buf, n, "%s", all.c_str());
    return (int)all.size() < n ? AP_OK : fail(AP_ERR_INVALID, "wgrad_route_names: %d bytes needed", (int)all.size() + 1);
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

int32_t ap_conv2d_wgrad_xs_ok(const ap_wgrad_desc* d) {
    WgradPlan pl;
    if (make_wgrad_plan(d, pl)) return 0;
    return wgrad_xs_direct_ok(d, pl) ? 1 : 0;
}

}  // extern "C"
