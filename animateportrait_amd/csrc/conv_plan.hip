// conv_plan.hip -- the convolution planner: kernel registries, make_plan and its steps, and the plan queries of the C ABI
// (conv_plan.h states the contract with the packer and the launchers).  Launches nothing.
#include "conv_plan.h"
#include "conv_head.h"      // kHeadMaxW only: the widest map of the half-wave head kernel (launched by conv_fwd.hip)

#include <utility>
#include <vector>

namespace apamd {

const std::vector<ConvKernelInfo>& registry() {
    static std::vector<ConvKernelInfo> v;
    static std::once_flag once;
    std::call_once(once, [] {
        register_s1k0(v);
        register_s1k3(v);
        register_s1k4(v);
        register_s1k7(v);
        register_s2k3(v);
        register_s2k4(v);
    });
    return v;
}

static const ConvKernelInfo* find_kernel(int CI, int S, int K, int CO_TILE) {
    for (const auto& k : registry())
        if (k.CI == CI && k.S == S && k.K == K && k.CO_TILE == CO_TILE) return &k;
    return nullptr;
}

// split-bf16 kernels (conv_bf16x3.h, conv_ph4.h): instantiated per tile family in conv_bf3_inst_*.hip / conv_ph4_inst.hip
const std::vector<Bf3Kernel>& bf3_registry() {
    static std::vector<Bf3Kernel> v;
    static std::once_flag once;
    std::call_once(once, [] {
        bf3_register_k3_short(v);
        bf3_register_k3_tall(v);
        bf3_register_s2k3(v);
        bf3_register_k4(v);
        bf3_register_row_tall(v);
        bf3_register_row_half(v);
        bf3_register_taps12(v);        // sub-pixel phases of ConvTranspose2d(s=2): 1, 2 or 4 taps (same tile geometry; the plan
        bf3_register_taps4(v);         // keeps the last)
        bf3_register_taps4_half(v);
    });
    return v;
}
// the kernel of one launch: K == 0 kernels are instantiated per tap count
const Bf3Kernel* bf3_for_taps(const Bf3Kernel* k, int ntaps) {
    if (k->K != 0) return k;
    for (const auto& e : bf3_registry())
        if (e.K == 0 && e.S == k->S && e.TMAX == ntaps && e.TH == k->TH) return &e;
    return nullptr;
}

// ------------------------------------------------------------------ make_plan, in steps
struct Geom {
    bool rowk;      // 1 x 7 over the row channels of a 7x7 stem (ap_split_prepass_rows): split-bf16 path only
    int K;          // taps along x
    int S, KT;      // kernel family: stride and dense tap count (0 = run-time taps)
};

// step 1: descriptor checks, kernel family, output size (pl.Hout, pl.Wout) and channel count (pl.Cin)
static int plan_geometry(const ap_conv_desc* d, Plan& pl, Geom& g) {
    if (!d) return fail(AP_ERR_INVALID, "null descriptor");
    if (d->nsrc < 1 || d->nsrc > kMaxSeg) return fail(AP_ERR_INVALID, "nsrc=%d out of range", d->nsrc);
    if (d->N < 1 || d->H < 1 || d->W < 1 || d->Cout < 1) return fail(AP_ERR_INVALID, "bad dims");
    g.rowk = d->KH == 1 && d->KW == 7;
    if (g.rowk) {
        if (d->transposed || d->stride != 1 || d->pad != 3 || d->nsrc != 1 || d->src[0].C != 32 ||
            d->precision == AP_PRECISION_FP32 || d->w_layout != AP_W_OIHW || d->w_flip)
            return fail(AP_ERR_UNSUPPORTED, "1x7 kernels exist only as the row form of a 7x7 stem (one 32-channel "
                                            "split source, stride 1, pad 3, split-bf16 precision)");
        if (d->pad_mode == AP_PAD_REFLECT && d->pad >= d->W) return fail(AP_ERR_INVALID, "reflection pad %d >= width", d->pad);
    } else if (d->KH != d->KW || d->KH < 1 || d->KH > 7) {
        return fail(AP_ERR_UNSUPPORTED, "kernel %dx%d", d->KH, d->KW);
    }
    const int K = g.K = d->KW;
    if (g.rowk) {
        g.S = 1; g.KT = K;
        pl.Hout = d->H; pl.Wout = d->W;
    } else if (!d->transposed) {
        if (d->stride != 1 && d->stride != 2) return fail(AP_ERR_UNSUPPORTED, "stride %d", d->stride);
        g.S = d->stride; g.KT = K;
        if (K == 2) {
            // the space-to-depth form of a 4x4 stride-2 layer (ap_split_prepass_s2d): 4 run-time taps, split-bf16 only
            if (d->stride != 1 || d->pad != 0 || d->precision == AP_PRECISION_FP32 || d->w_layout != AP_W_OIHW || d->w_flip)
                return fail(AP_ERR_UNSUPPORTED, "2x2 kernels exist only as the space-to-depth form of a 4x4 stride-2 layer "
                                                "(stride 1, pad 0, split-bf16 precision)");
            g.KT = 0;
        } else if (K == 1) {
            // 1x1 convolution (channel_mapping of the intrinsic-flow regressor, intrinsic_flow_models/networks.py:23-24):
            // one run-time tap at offset (0, 0)
            if (d->stride != 1 || d->pad != 0) return fail(AP_ERR_UNSUPPORTED, "1x1 kernels: stride 1, pad 0 only");
            g.KT = 0;
        } else if (K != 3 && K != 4 && K != 7) {
            return fail(AP_ERR_UNSUPPORTED, "kernel size %d (built: 1, 3, 4, 7)", K);
        }
        pl.Hout = (d->H + 2 * d->pad - K) / g.S + 1;
        pl.Wout = (d->W + 2 * d->pad - K) / g.S + 1;
        if (d->pad_mode == AP_PAD_REFLECT && (d->pad >= d->H || d->pad >= d->W))
            return fail(AP_ERR_INVALID, "reflection pad %d >= input size", d->pad);
    } else {
        if (d->stride != 2) return fail(AP_ERR_UNSUPPORTED, "transposed conv needs stride 2");
        if (d->pad_mode != AP_PAD_ZERO) return fail(AP_ERR_UNSUPPORTED, "transposed conv with reflection pad");
        g.S = 1; g.KT = 0;
        pl.Hout = (d->H - 1) * 2 - 2 * d->pad + K + d->output_padding;
        pl.Wout = (d->W - 1) * 2 - 2 * d->pad + K + d->output_padding;
    }
    if (pl.Hout < 1 || pl.Wout < 1) return fail(AP_ERR_INVALID, "empty output");
    pl.Cin = 0;
    for (int s = 0; s < d->nsrc; ++s) {
        if (d->src[s].C < 1) return fail(AP_ERR_INVALID, "segment %d has C=%d", s, d->src[s].C);
        pl.Cin += d->src[s].C;
    }
    return AP_OK;
}

// chunk layout: segment s starts at chunk chunk_begin[s] and takes ceil(C / ci) chunks of ci channels
static void layout_chunks(const ap_conv_desc* d, Plan& pl, int ci) {
    pl.nchunks = 0;
    for (int s = 0; s < d->nsrc; ++s) {
        pl.chunk_begin[s] = pl.nchunks;
        pl.nchunks += (d->src[s].C + ci - 1) / ci;
    }
    pl.cin_pad = pl.nchunks * ci;
}

// 1..4 output channels, 7x7 'same' convolution: vector-ALU direct kernel (conv_direct.h), no launch list
// (the PatchGAN's 4x4 pad-1 head, 512 -> 1 on 30 x 30 outputs, was tried here too: 160 workgroups of 128 chunks
// each run 0.60 ms against 0.39 ms on the MFMA kernel with a 1-of-32 filled tile)
static bool plan_direct(const ap_conv_desc* d, const Geom& g, Plan& pl) {
    if (g.rowk || d->transposed || d->stride != 1 || g.K != 7 || d->pad != 3 || d->Cout > 4) return false;
    pl.direct_cop = d->Cout == 1 ? 1 : 4;
    layout_chunks(d, pl, 4);
    pl.packed_floats = (long long)pl.cin_pad * g.K * g.K * pl.direct_cop;
    pl.stat_tiles = ((pl.Hout + 15) / 16) * ((pl.Wout + 63) / 64);
    return true;
}

// narrow 3x3 layers (landmark encoder): memory streams, one lane per output pixel (conv_small.h)
static bool plan_small(const ap_conv_desc* d, const Geom& g, Plan& pl) {
    if (g.rowk || d->transposed || g.K != 3 || d->nsrc != 1 || pl.Cin > 16 || (d->Cout != 8 && d->Cout != 16) ||
        d->w_layout != AP_W_OIHW || d->w_flip || sw(SW_NO_SMALL))
        return false;
    pl.small = true;
    pl.nchunks = 1;
    pl.cin_pad = pl.Cin;
    pl.packed_floats = (long long)d->Cout * pl.Cin * 9;       // the OIHW weights as they are
    pl.stat_tiles = ((pl.Hout + 7) / 8) * ((pl.Wout + 31) / 32);
    return true;
}

// The two layers that carry a plain copy of their weights behind the regular packed image (returns whether this one does).
// PatchGAN output layer (one output channel, 4x4 pad 1; conv_head.h): the weight image must not depend on the map size (weights
// are packed once per layer), so layers of this shape carry their OIHW weights, and maps narrow enough for the half-wave row
// kernel use those.  ConvTranspose2d(C, 1..4, 4, 2, 1): the data gradient of the PatchGAN's first layer w.r.t. the frame
// (conv_tsmall.h); same arrangement with the IOHW weights.
static bool plan_head_tsmall(const ap_conv_desc* d, const Geom& g, Plan& pl) {
    const bool head_w = !g.rowk && !d->transposed && d->stride == 1 && g.K == 4 && d->Cout == 1 && d->nsrc == 1 && pl.Cin >= 64 &&
                        d->w_layout == AP_W_OIHW && !d->w_flip && d->pad == 1;
    pl.head = head_w && d->W <= kHeadMaxW;
    pl.tsmall = !g.rowk && d->transposed && d->stride == 2 && g.K == 4 && d->pad == 1 && d->output_padding == 0 && d->Cout <= 4 &&
                d->nsrc == 1 && d->w_layout == AP_W_IOHW && !d->w_flip;
    return head_w || pl.tsmall;
}

// The split-bf16 matrix path (conv_bf16x3.h) and its kernel, pl.bk (left null: the layer stays on the fp32 kernel): the row form
// of a stem, and wide 3x3 / 4x4 / transposed layers when the caller allows ~1e-4 relative error (>= 48 outputs fill most of a
// 64-cout tile; with >= 128 inputs even a 16-output layer -- the data gradient of a ResnetBlock2 convolution w.r.t. its
// 16-channel landmark segments -- is 3x faster here than on the fp32 pipe)
static int pick_bf3(const ap_conv_desc* d, const Geom& g, Plan& pl) {
    const int K = g.K, KT = g.KT;
    if (g.rowk) {
        // the shortest row tile: two workgroups per CU
        for (const auto& k : bf3_registry())
            if (k.ROW && k.K == K && (!pl.bk || k.TH < pl.bk->TH)) pl.bk = &k;
        return pl.bk ? AP_OK : fail(AP_ERR_UNSUPPORTED, "no 1x%d row kernel", K);
    }
    if (d->precision == AP_PRECISION_FP32 || !(d->Cout >= 48 || (d->Cout >= 16 && pl.Cin >= 128)) || pl.Cin < 32 ||
        sw(SW_NO_BF16X3))
        return AP_OK;
    for (int s = 0; s < d->nsrc; ++s)
        if (d->src[s].C % 16 != 0) return AP_OK;
    if (!(KT == 0 ? K <= 4 : (K == 3 || (K == 4 && g.S == 1)))) return AP_OK;
    // several tile heights of a family: the tallest one (best operand reuse) unless its tile list leaves
    // most CUs idle (streaming inference at batch 1..4), then the shortest
    const Bf3Kernel *tall = nullptr, *small = nullptr;
    for (const auto& k : bf3_registry())
        if (k.S == g.S && k.K == KT && !k.ROW) {
            if (!tall || k.TH >= tall->TH) tall = &k;
            if (!small || k.TH < small->TH) small = &k;
        }
    pl.bk = tall;
    const bool even_out = pl.Hout % 2 == 0 && pl.Wout % 2 == 0;
    if (KT == 0) {
        // every launch of these plans has 4 taps (2x2 layers, 4x4 phases, fused 3x3 phases of an even output): half-height tile
        pl.k0_small = K == 2 || K == 4 || (d->transposed && K == 3 && even_out);
        if (pl.k0_small) pl.bk = small;
        // stride-2 transposed 3x3 / 4x4 with pad 1 and an even output: all four phases in one tile
        if (d->transposed && (K == 3 || K == 4) && d->pad == 1 && d->stride == 2 && even_out) {
            pl.ph4 = K;
            pl.bk = ph4_kernel(K);
        }
    } else if (tall && small != tall) {
        const long long tiles = (long long)d->N * ((pl.Hout + tall->TH - 1) / tall->TH) * ((pl.Wout + 31) / 32) *
                                ((d->Cout + tall->CO_TILE - 1) / tall->CO_TILE);
        // (also for maps no taller than the short tile: the column strip of a reflection-padded data gradient)
        if ((tiles * 2 <= num_cus() || pl.Hout <= small->TH) && !sw(SW_NO_SMALL_TILES)) pl.bk = small;
    }
    return AP_OK;
}

// The fp32 implicit-GEMM kernel (conv_igemm.h), pl.k: cout tile by output width, channel chunk by the segments and the LDS budget
static int pick_igemm(const ap_conv_desc* d, const Geom& g, Plan& pl) {
    int co_tile = d->Cout >= 96 ? 128 : (d->Cout >= 48 ? 64 : 32);
    if (const int forced = sw(SW_CONV_COTILE)) co_tile = forced;
    // channel chunk: largest of {8,4,2} that does not over-pad the narrowest segment, then shrink
    // until two workgroups fit a CU's LDS
    int minC = 1 << 30;
    for (int s = 0; s < d->nsrc; ++s) minC = std::min(minC, (int)d->src[s].C);
    int ci = minC <= 2 ? 2 : (minC <= 4 ? 4 : 8);
    for (int s = 0; s < d->nsrc; ++s)
        while (ci > 2 && d->src[s].C % ci != 0 && d->src[s].C > ci) ci >>= 1;
    const int ntaps_max = d->transposed ? ((g.K + 1) / 2) * ((g.K + 1) / 2) : g.K * g.K;
    const size_t lds_target = (size_t)sw(SW_CONV_LDS_TARGET);
    for (;;) {
        const ConvKernelInfo* k = find_kernel(ci, g.S, g.KT, co_tile);
        if (!k) return fail(AP_ERR_UNSUPPORTED, "no kernel for CI=%d S=%d K=%d CO_TILE=%d", ci, g.S, g.KT, co_tile);
        int nch = 0;
        for (int s = 0; s < d->nsrc; ++s) nch += (d->src[s].C + ci - 1) / ci;
        const size_t bytes = 4 * k->lds_floats(ntaps_max, nch > 1 ? 2 : 1, nch * ci);
        if (bytes <= lds_target || ci == 2) {
            if (bytes > 160 * 1024) return fail(AP_ERR_UNSUPPORTED, "LDS tile of %zu bytes does not fit", bytes);
            pl.k = k;
            break;
        }
        ci >>= 1;
    }
    if (const int forced = sw(SW_CONV_CI)) {
        if (const ConvKernelInfo* k = find_kernel(forced, g.S, g.KT, co_tile)) { pl.k = k; ci = forced; }
    }
    layout_chunks(d, pl, ci);
    pl.co_tiles = (d->Cout + co_tile - 1) / co_tile;
    return AP_OK;
}

// a finished launch takes its tile grid, its weight block and its statistics tiles
static void add_launch(Plan& pl, Launch& L) {
    const int ntaps = (int)L.taps.size();
    const int th = pl.bk ? pl.bk->TH : pl.k->TH;
    const int wf = pl.bk ? pl.bk->wfloats(ntaps) : pl.k->wfloats(ntaps);
    L.tiles_x = (L.OW + 31) / 32;
    L.tiles_y = (L.OH + th - 1) / th;
    L.wp_off = pl.packed_floats;
    L.stat_tile_off = pl.stat_tiles;
    pl.packed_floats += (long long)pl.co_tiles * pl.nchunks * wf;
    pl.stat_tiles += L.tiles_x * L.tiles_y;
    pl.launches.push_back(L);
}

static void dense_launch(const ap_conv_desc* d, const Geom& g, Plan& pl) {
    const int K = g.K;
    Launch L;
    for (int ky = 0; ky < (g.rowk ? 1 : K); ++ky)
        for (int kx = 0; kx < K; ++kx) L.taps.push_back(Tap{d->w_flip ? K - 1 - ky : ky, d->w_flip ? K - 1 - kx : kx, ky, kx});
    L.OH = pl.Hout; L.OW = pl.Wout;
    L.dy0 = g.rowk ? 0 : -d->pad; L.dx0 = -d->pad;
    L.osy = L.osx = 1; L.oy_off = L.ox_off = 0;
    add_launch(pl, L);
}

// ConvTranspose2d stride 2 as sub-pixel phases:
// y[co, 2q+ph] = sum over taps k with (ph + pad - k) even of x[ci, q + (ph + pad - k)/2] * w[ci,co,k]
// Split-bf16 path, even output size: the four phases share one pixel-tile grid and run as ONE launch whose
// cout tiles enumerate (phase, cout tile) -- the activation tile is fetched from HBM once instead of four
// times and the interleaved output lines of the phases meet in the XCD's L2 (conv_bf16x3.h, ConvKParams.nphase).
static int phase_launches(const ap_conv_desc* d, const Geom& g, Plan& pl) {
    const int K = g.K;
    const bool fuse = pl.bk != nullptr && pl.Hout % 2 == 0 && pl.Wout % 2 == 0;
    for (int phy = 0; phy < 2; ++phy)
        for (int phx = 0; phx < 2; ++phx) {
            Launch L;
            L.OH = (pl.Hout - phy + 1) / 2;
            L.OW = (pl.Wout - phx + 1) / 2;
            if (L.OH < 1 || L.OW < 1) continue;
            std::vector<std::pair<int, int>> ys, xs;  // (k, shift)
            for (int k = 0; k < K; ++k) {
                if (((phy + d->pad - k) % 2 + 2) % 2 == 0) ys.push_back({k, (phy + d->pad - k) / 2});
                if (((phx + d->pad - k) % 2 + 2) % 2 == 0) xs.push_back({k, (phx + d->pad - k) / 2});
            }
            int miny = 1 << 30, minx = 1 << 30, maxy = -(1 << 30), maxx = -(1 << 30);
            for (auto& a : ys) { miny = std::min(miny, a.second); maxy = std::max(maxy, a.second); }
            for (auto& a : xs) { minx = std::min(minx, a.second); maxx = std::max(maxx, a.second); }
            if (ys.empty() || xs.empty() || maxy - miny > 1 || maxx - minx > 1)
                return fail(AP_ERR_UNSUPPORTED, "transposed conv k=%d pad=%d not decomposable", K, d->pad);
            for (auto& a : ys)
                for (auto& b : xs)
                    L.taps.push_back(Tap{d->w_flip ? K - 1 - a.first : a.first, d->w_flip ? K - 1 - b.first : b.first,
                                         a.second - miny, b.second - minx});
            L.dy0 = miny; L.dx0 = minx;
            L.osy = L.osx = 2; L.oy_off = phy; L.ox_off = phx;
            if (fuse) {
                // one launch for the four phases: every phase carries the whole 2 x 2 window (positions it does
                // not have get zero weights), in the fixed order t = ly * 2 + lx
                std::vector<Tap> win(4, Tap{-1, -1, 0, 0});
                for (int t = 0; t < 4; ++t) { win[t].ly = t >> 1; win[t].lx = t & 1; }
                for (const auto& t : L.taps) { win[t.ly * 2 + t.lx].ky = t.ky; win[t.ly * 2 + t.lx].kx = t.kx; }
                L.taps = win;
            }
            add_launch(pl, L);
        }
    pl.fused_phases = fuse && pl.launches.size() == 4;
    return AP_OK;
}

int make_plan(const ap_conv_desc* d, Plan& pl) {
    Geom g;
    int rc = plan_geometry(d, pl, g);
    if (rc) return rc;
    if (plan_direct(d, g, pl) || plan_small(d, g, pl)) return AP_OK;
    const bool plain_w = plan_head_tsmall(d, g, pl);
    rc = pick_bf3(d, g, pl);
    if (rc) return rc;
    if (pl.bk) {
        // step 3, chunk layout: 16 channels of the split sources per chunk
        pl.bf3 = true;
        layout_chunks(d, pl, 16);                  // cin_pad: channels that exist in the sources
        pl.nchunks = (pl.nchunks + 1) & ~1;        // the kernel's pipeline runs chunk pairs: pad with an all-zero chunk
        pl.co_tiles = (d->Cout + pl.bk->CO_TILE - 1) / pl.bk->CO_TILE;
    } else {
        rc = pick_igemm(d, g, pl);
        if (rc) return rc;
    }
    // step 4: the launch list
    if (d->transposed) {
        rc = phase_launches(d, g, pl);
        if (rc) return rc;
    } else {
        dense_launch(d, g, pl);
    }
    if (plain_w) {
        pl.head_w_off = (pl.packed_floats + 3) & ~3LL;            // float4 loads
        pl.packed_floats = pl.head_w_off + (long long)pl.Cin * d->Cout * g.K * g.K;
    }
    return AP_OK;
}

// ------------------------------------------------------------------ which plans take which output form
// the channel-octet output form exists in the run-time-tap and row families of the split-bf16 kernel (conv_bf16x3.h epilogue)
bool octet_plan_ok(const ap_conv_desc* d, const Plan& pl) {
    if (!pl.bf3 || pl.fused_phases || pl.ph4 || pl.launches.size() != 1 || (d->Cout & 7)) return false;
    const Bf3Kernel* kern = bf3_for_taps(pl.bk, (int)pl.launches[0].taps.size());
    return kern && (kern->K == 0 || kern->ROW || (kern->K == 3 && kern->S == 1 && d->precision == AP_PRECISION_BF16X3));
}

// the bf16-output form exists for the plain-bf16 instantiations of the dense 3x3 stride-1 tiles (Bf3Cfg::OB16)
bool ob16_plan_ok(const ap_conv_desc* d, const Plan& pl) {
    if (!pl.bf3 || pl.fused_phases || pl.ph4 || pl.launches.size() != 1 || d->precision != AP_PRECISION_BF16) return false;
    return pl.bk && pl.bk->fn1_ob16 != nullptr;
}

// the answer of an ap_conv2d_*_ok query: the descriptor has a plan and the plan passes the predicate
static int32_t plan_passes(const ap_conv_desc* d, bool (*ok)(const ap_conv_desc*, const Plan&)) {
    Plan pl;
    return !make_plan(d, pl) && ok(d, pl) ? 1 : 0;
}

}  // namespace apamd

using namespace apamd;

extern "C" {

int ap_conv2d_out_size(const ap_conv_desc* d, int32_t* Hout, int32_t* Wout) {
    Plan pl;
    int rc = make_plan(d, pl);
    if (rc) return rc;
    if (Hout) *Hout = pl.Hout;
    if (Wout) *Wout = pl.Wout;
    return AP_OK;
}

int64_t ap_conv2d_packed_floats(const ap_conv_desc* d) {
    Plan pl;
    int rc = make_plan(d, pl);
    return rc ? rc : pl.packed_floats;
}

int32_t ap_conv2d_stat_tiles(const ap_conv_desc* d) {
    Plan pl;
    int rc = make_plan(d, pl);
    return rc ? rc : pl.stat_tiles;
}

int32_t ap_conv2d_wants_presplit(const ap_conv_desc* d) {
    Plan pl;
    int rc = make_plan(d, pl);
    return rc ? rc : (pl.bf3 ? 1 : 0);
}

int ap_conv2d_kernel_name(const ap_conv_desc* d, char* buf, int32_t buflen) {
    Plan pl;
    int rc = make_plan(d, pl);
    if (rc) return rc;
    if (!buf || buflen < 1) return fail(AP_ERR_INVALID, "kernel_name: bad buffer");
    if (pl.direct_cop) snprintf(buf, buflen, "DirectCfg<%d, %d>", d->KH, pl.direct_cop);
    else if (pl.small) snprintf(buf, buflen, "SmallCfg<%d, %d>", d->stride, d->Cout);
    else if (pl.head) snprintf(buf, buflen, "HeadCfg<%d>", d->KH);
    else if (pl.tsmall) snprintf(buf, buflen, "TSmallCfg<%d>", d->Cout);
    else if (pl.bf3) snprintf(buf, buflen, "%s%s", pl.bk->name, d->precision == AP_PRECISION_BF16 ? " bf16" : "");
    else snprintf(buf, buflen, "ConvCfg<%d, %d, %d, %d, %d, %d, %d>", pl.k->CI, pl.k->S, pl.k->K, pl.k->WCO, pl.k->MT, pl.k->WPX, pl.k->NT);
    return AP_OK;
}

int32_t ap_conv2d_octet_ok(const ap_conv_desc* d) { return plan_passes(d, octet_plan_ok); }
int32_t ap_conv2d_bf16out_ok(const ap_conv_desc* d) { return plan_passes(d, ob16_plan_ok); }

}  // extern "C"
