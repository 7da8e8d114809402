// conv_host.hip -- host-side planning and the C ABI of the convolution operator.
//
// A descriptor (ap_conv_desc) is turned into one launch (Conv2d) or four launches
// (ConvTranspose2d stride 2 as sub-pixel phases) of conv_igemm_f32; the same plan drives
// the weight packer so that the packed image and the kernel always agree.
#include "common.h"
#include "conv_registry.h"
#include "conv_direct.h"
#include "conv_tapgemm.h"
#include "conv_bf3_registry.h"
#include "conv_prepass.h"
#include "conv_small.h"
#include "conv_head.h"
#include "conv_tsmall.h"

#include <cstdlib>
#include <cstring>
#include <vector>

namespace apamd {

#ifdef APAMD_VARIANTS
const void* bf3_sb_kernel(size_t* lds_bytes);     // tools/variants/conv_bf3_sb.hip
#endif

static thread_local char g_err[512];
char* last_error_buf() { return g_err; }
int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

static const std::vector<ConvKernelInfo>& registry() {
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
static const std::vector<Bf3Kernel>& bf3_registry() {
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
static const Bf3Kernel* bf3_for_taps(const Bf3Kernel* k, int ntaps) {
    if (k->K != 0) return k;
    for (const auto& e : bf3_registry())
        if (e.K == 0 && e.S == k->S && e.TMAX == ntaps && e.TH == k->TH) return &e;
    return nullptr;
}

struct Tap { int ky, kx, ly, lx; };  // (ky,kx): index into the caller's weight; (ly,lx): LDS tile offset

struct Launch {
    std::vector<Tap> taps;
    int OH, OW, dy0, dx0;
    int osy, osx, oy_off, ox_off;
    int tiles_x, tiles_y;
    long long wp_off;      // float offset of this launch's weights in the packed buffer
    int stat_tile_off;
};

struct Plan {
    const ConvKernelInfo* k = nullptr;
    int direct_cop = 0;            // > 0: conv_direct_f32<K, direct_cop> instead of the implicit-GEMM kernel
    bool small = false;            // conv_small_f32: narrow 3x3 layers on the vector ALUs
    bool head = false;             // conv_head_fwd_kernel: one output channel, 4x4, narrow map
    bool tsmall = false;           // conv_tsmall_f32: transposed 4x4 stride 2 with 1..4 output channels
    long long head_w_off = -1;     // >= 0: plain copy of the caller's weights at this offset of the packed image
    bool bf3 = false;              // split-bf16 matrix path
    bool fused_phases = false;     // transposed, split-bf16: the four sub-pixel phases are one launch
    int ph4 = 0;                   // 3 / 4: ... and one TILE (conv_ph4.h)
    bool k0_small = false;         // run-time-tap family: the half-height 4-tap instantiation (two workgroups per CU)
    const Bf3Kernel* bk = nullptr;
    std::vector<Launch> launches;
    int Cin = 0, nchunks = 0, cin_pad = 0, co_tiles = 0;
    int chunk_begin[kMaxSeg] = {0, 0, 0};
    int Hout = 0, Wout = 0, stat_tiles = 0;
    long long packed_floats = 0;
};

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
        d->w_layout != AP_W_OIHW || d->w_flip || env_int("APAMD_NO_SMALL", 0))
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
        env_int("APAMD_NO_BF16X3", 0))
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
        if ((tiles * 2 <= num_cus() || pl.Hout <= small->TH) && !env_int("APAMD_NO_SMALL_TILES", 0)) pl.bk = small;
    }
    return AP_OK;
}

// The fp32 implicit-GEMM kernel (conv_igemm.h), pl.k: cout tile by output width, channel chunk by the segments and the LDS budget
static int pick_igemm(const ap_conv_desc* d, const Geom& g, Plan& pl) {
    int co_tile = d->Cout >= 96 ? 128 : (d->Cout >= 48 ? 64 : 32);
    co_tile = env_int("APAMD_CONV_COTILE", co_tile);
    // channel chunk: largest of {8,4,2} that does not over-pad the narrowest segment, then shrink
    // until two workgroups fit a CU's LDS
    int minC = 1 << 30;
    for (int s = 0; s < d->nsrc; ++s) minC = std::min(minC, (int)d->src[s].C);
    int ci = minC <= 2 ? 2 : (minC <= 4 ? 4 : 8);
    for (int s = 0; s < d->nsrc; ++s)
        while (ci > 2 && d->src[s].C % ci != 0 && d->src[s].C > ci) ci >>= 1;
    const int ntaps_max = d->transposed ? ((g.K + 1) / 2) * ((g.K + 1) / 2) : g.K * g.K;
    const size_t lds_target = (size_t)env_int("APAMD_CONV_LDS_TARGET", 72 * 1024);
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
    if (const int forced = env_int("APAMD_CONV_CI", 0)) {
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

static int make_plan(const ap_conv_desc* d, Plan& pl) {
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

// ------------------------------------------------------------------ weight packer
struct PackParams {
    const float* w;
    float* out;
    int Cin, Cout, K, layout;
    int nseg, segC[kMaxSeg], chunk_begin[kMaxSeg];
    int CI, CO_TILE, nchunks, co_tiles, ntaps, wfloats;
    int tap_ky[kMaxTaps], tap_kx[kMaxTaps];
};

__global__ void pack_weights_kernel(const PackParams p) {
    const long long total = (long long)p.co_tiles * p.nchunks * p.wfloats;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        const int within = (int)(idx % p.wfloats);
        const long long blk = idx / p.wfloats;
        const int chunk = (int)(blk % p.nchunks);
        const int cot = (int)(blk / p.nchunks);
        float v = 0.f;
        if (within < p.ntaps * p.CI * p.CO_TILE) {
            const int col = within % p.CO_TILE;
            const int ci = (within / p.CO_TILE) % p.CI;
            const int t = within / (p.CO_TILE * p.CI);
            const int co = cot * p.CO_TILE + col;
            int s = 0;
            if (p.nseg > 1 && chunk >= p.chunk_begin[1]) s = 1;
            if (p.nseg > 2 && chunk >= p.chunk_begin[2]) s = 2;
            const int cs = (chunk - p.chunk_begin[s]) * p.CI + ci;
            if (cs < p.segC[s] && co < p.Cout) {
                int cin = cs;
                for (int j = 0; j < s; ++j) cin += p.segC[j];
                const int ky = p.tap_ky[t], kx = p.tap_kx[t];
                const long long off = p.layout == AP_W_OIHW
                                          ? (((long long)co * p.Cin + cin) * p.K + ky) * p.K + kx
                                          : (((long long)cin * p.Cout + co) * p.K + ky) * p.K + kx;
                v = p.w[off];
            }
        }
        p.out[idx] = v;
    }
}

struct PackDirectParams {
    const float* w;
    float* out;
    int Cin, Cout, K, layout, flip, COP, CI, nchunks;
    int nseg, segC[kMaxSeg], chunk_begin[kMaxSeg];
};

// out[cin_pad][K][K][COP]
__global__ void pack_direct_kernel(const PackDirectParams p) {
    const int total = p.nchunks * p.CI * p.K * p.K * p.COP;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const int co = idx % p.COP;
        int t = idx / p.COP;
        int kx = t % p.K; t /= p.K;
        int ky = t % p.K; t /= p.K;
        const int ci = t % p.CI;
        const int chunk = t / p.CI;
        int s = 0;
        if (p.nseg > 1 && chunk >= p.chunk_begin[1]) s = 1;
        if (p.nseg > 2 && chunk >= p.chunk_begin[2]) s = 2;
        const int cs = (chunk - p.chunk_begin[s]) * p.CI + ci;
        float v = 0.f;
        if (cs < p.segC[s] && co < p.Cout) {
            int cin = cs;
            for (int j = 0; j < s; ++j) cin += p.segC[j];
            if (p.flip) { ky = p.K - 1 - ky; kx = p.K - 1 - kx; }
            const long long off = p.layout == AP_W_OIHW ? (((long long)co * p.Cin + cin) * p.K + ky) * p.K + kx
                                                        : (((long long)cin * p.Cout + co) * p.K + ky) * p.K + kx;
            v = p.w[off];
        }
        p.out[idx] = v;
    }
}

static const void* direct_fn(int K, int cop) {
    if (K == 7 && cop == 1) return reinterpret_cast<const void*>(&conv_direct_f32<DirectCfg<7, 1>>);
    if (K == 7 && cop == 4) return reinterpret_cast<const void*>(&conv_direct_f32<DirectCfg<7, 4>>);
    return nullptr;
}
static size_t direct_lds_bytes(int K, int cop, int nbuf, int cin_pad) {
    if (cop == 1) return 4 * DirectCfg<7, 1>::lds_floats(nbuf, cin_pad);
    return 4 * DirectCfg<7, 4>::lds_floats(nbuf, cin_pad);
}

// the packer's parameters for one launch of a split-bf16 plan; `v` (nullable): the weight as a strided / derived view
static PackBf3Params bf3_pack_params(const ap_conv_desc* d, const Plan& pl, const Launch& L, const float* weight,
                                     const ap_weight_view* v, float* packed) {
    PackBf3Params p;
    memset(&p, 0, sizeof(p));
    p.w = v ? v->w : weight;
    p.out = reinterpret_cast<unsigned short*>(packed + L.wp_off);
    p.Cin = pl.Cin; p.Cout = d->Cout; p.K = d->KW; p.layout = d->w_layout; p.flip = 0;
    p.KH = d->KH != d->KW ? d->KH : 0;
    p.nseg = d->nsrc;
    for (int s = 0; s < d->nsrc; ++s) { p.segC[s] = d->src[s].C; p.chunk_begin[s] = pl.chunk_begin[s]; }
    p.CO_TILE = pl.bk->CO_TILE; p.nchunks = pl.nchunks; p.co_tiles = pl.co_tiles;
    p.ntaps = (int)L.taps.size();
    for (int t = 0; t < p.ntaps; ++t) { p.tap_ky[t] = L.taps[t].ky; p.tap_kx[t] = L.taps[t].kx; }
    if (v) {
        p.view = 1;
        p.s_co = v->s_co; p.s_ci = v->s_ci; p.s_ky = v->s_ky; p.s_kx = v->s_kx;
        p.s2d_c = v->s2d_c; p.rows_c = v->rows_c; p.ksrc = v->ksrc;
    }
    return p;
}

}  // namespace apamd

using namespace apamd;

extern "C" {

const char* ap_version(void) { return "animateportrait_amd 0.3 (gfx950)"; }
int32_t ap_abi_version(void) { return AP_ABI_VERSION; }
const char* ap_last_error(void) { return last_error_buf(); }

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

int64_t ap_split_prepass_bytes(int32_t N, int32_t C, int32_t H, int32_t W) {
    if (N < 1 || C < 8 || (C & 7) || H < 1 || W < 1) return fail(AP_ERR_INVALID, "split_prepass: C=%d must be a multiple of 8", C);
    return (int64_t)N * 2 * (C / 8) * ((int64_t)H * W + 1) * 16;     // one all-zero slot closes every plane
}

int ap_norm_apply_split(const ap_src* src, const float* stat_partials, int32_t tiles, float eps, float* mean_out,
                        float* rstd_out, const ap_src* residual, int32_t N, int32_t H, int32_t W, float* y, void* xs,
                        ap_stream_t stream) {
    return ap_norm_apply_split_ex(src, stat_partials, tiles, eps, mean_out, rstd_out, residual, N, H, W, y, xs, 0, stream);
}

int ap_norm_apply_split_ex(const ap_src* src, const float* stat_partials, int32_t tiles, float eps, float* mean_out,
                           float* rstd_out, const ap_src* residual, int32_t N, int32_t H, int32_t W, float* y, void* xs,
                           int32_t flags, ap_stream_t stream) {
    if (!src || !src->data) return fail(AP_ERR_INVALID, "norm_apply_split: null source");
    if (!y && !xs && !stat_partials) return fail(AP_ERR_INVALID, "norm_apply_split: nothing to produce");
    if (N < 1 || src->C < 8 || (src->C & 7) || H < 1 || W < 1)
        return fail(AP_ERR_INVALID, "norm_apply_split: C=%d must be a multiple of 8", src->C);
    if ((src->mean == nullptr) != (src->rstd == nullptr)) return fail(AP_ERR_INVALID, "norm_apply_split: mean/rstd mismatch");
    if (src->act < 0 || src->act > 2) return fail(AP_ERR_INVALID, "norm_apply_split: act %d", src->act);
    if (stat_partials) {
        if (src->mean) return fail(AP_ERR_INVALID, "norm_apply_split: pass finished statistics OR partial tiles");
        if (tiles < 1 || !mean_out || !rstd_out) return fail(AP_ERR_INVALID, "norm_apply_split: partial tiles need tiles >= 1 and mean_out / rstd_out");
    }
    if (residual) {
        if (!residual->data || residual->C != src->C) return fail(AP_ERR_INVALID, "norm_apply_split: residual mismatch");
        if ((residual->mean == nullptr) != (residual->rstd == nullptr) || residual->act != AP_ACT_NONE)
            return fail(AP_ERR_INVALID, "norm_apply_split: a residual may be normalised but not activated");
    }
    if (N > 65535 || src->C / 8 > 65535) return fail(AP_ERR_UNSUPPORTED, "norm_apply_split: grid too large");
    NormSplitParams p;
    memset(&p, 0, sizeof(p));
    p.x = src->data; p.mean = src->mean; p.rstd = src->rstd;
    p.partials = stat_partials; p.tiles = tiles; p.inv_count = 1.0 / ((double)H * W); p.eps = eps;
    p.mean_out = mean_out; p.rstd_out = rstd_out;
    p.act = src->act;
    if (residual) { p.res = residual->data; p.res_mean = residual->mean; p.res_rstd = residual->rstd; }
    if (flags & 4) {            // the residual is handed over as its split copy (head + tail planes)
        if (!residual || residual->mean) return fail(AP_ERR_INVALID, "norm_apply_split: a split-copy residual must be a plain feature");
        p.res_xs = reinterpret_cast<const uint4*>(residual->data);
        p.res = nullptr;
    }
    p.y = y; p.xs = reinterpret_cast<uint4*>(xs);
    p.heads_only = (flags & 1) ? 1 : 0;
    p.xs_relu = (flags & 2) ? 1 : 0;
    p.N = N; p.C = src->C; p.HW = H * W;
    const bool xb16 = (flags & 8) != 0;       // src->data holds bf16 values (a raw output of ap_conv2d_fwd_bf16out)
    const int res_kind = p.res_xs ? 2 : (p.res ? 1 : 0);
    if (flags & 16) {           // src->data is the channel-octet raw output of ap_conv2d_fwd_octet; the only output is the split copy
        if (y || !xs || res_kind == 1 || xb16)
            return fail(AP_ERR_UNSUPPORTED, "norm_apply_split: a channel-octet source gives a split copy only, with no residual or a split-copy one");
        dim3 grid((p.HW + 511) / 512, src->C / 8, N);
        if (res_kind == 2) hipLaunchKernelGGL(norm_split_oct_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, p);
        else hipLaunchKernelGGL(norm_split_oct_kernel<0>, grid, dim3(256), 0, (hipStream_t)stream, p);
        return check_launch("norm_split_oct_kernel");
    }
    auto launch = [&](auto vt, auto xt, auto rt, dim3 grid) {
        hipLaunchKernelGGL((norm_split_kernel<decltype(vt)::value, decltype(xt)::value, decltype(rt)::value>), grid, dim3(256), 0, (hipStream_t)stream, p);
    };
    auto by_res = [&](auto vt, auto xt, dim3 grid) {
        if (res_kind == 0) launch(vt, xt, std::integral_constant<int, 0>{}, grid);
        else if (res_kind == 1) launch(vt, xt, std::integral_constant<int, 1>{}, grid);
        else launch(vt, xt, std::integral_constant<int, 2>{}, grid);
    };
    if ((p.HW & 3) == 0) {
        dim3 grid((p.HW / 4 + 255) / 256, src->C / 8, N);
        if (xb16) by_res(std::integral_constant<int, 4>{}, std::true_type{}, grid);
        else by_res(std::integral_constant<int, 4>{}, std::false_type{}, grid);
    } else {
        dim3 grid((p.HW + 255) / 256, src->C / 8, N);
        if (xb16) by_res(std::integral_constant<int, 1>{}, std::true_type{}, grid);
        else by_res(std::integral_constant<int, 1>{}, std::false_type{}, grid);
    }
    return check_launch("norm_split_kernel");
}

int ap_split_prepass_rows(const ap_src* src, int32_t N, int32_t H, int32_t W, int32_t K, int32_t pad, int32_t pad_mode,
                          void* out, ap_stream_t stream) {
    if (!src || !src->data || !out) return fail(AP_ERR_INVALID, "split_prepass_rows: null pointer");
    if (K != 7 || pad != 3 || src->C < 1 || src->C > 4)
        return fail(AP_ERR_UNSUPPORTED, "split_prepass_rows: built for 7x7 stems with 1..4 input channels (K=%d, C=%d)", K, src->C);
    if (N < 1 || N > 65535 || H < 1 || W < 1) return fail(AP_ERR_INVALID, "split_prepass_rows: bad sizes");
    if ((src->mean == nullptr) != (src->rstd == nullptr)) return fail(AP_ERR_INVALID, "split_prepass_rows: mean/rstd mismatch");
    if (pad_mode == AP_PAD_REFLECT && pad >= H) return fail(AP_ERR_INVALID, "split_prepass_rows: reflection pad %d >= height", pad);
    SplitRowsParams p;
    memset(&p, 0, sizeof(p));
    p.x = src->data; p.mean = src->mean; p.rstd = src->rstd; p.act = src->act;
    p.N = N; p.C = src->C; p.H = H; p.W = W; p.K = K; p.pad = pad; p.pad_mode = pad_mode;
    p.out = reinterpret_cast<uint4*>(out);
    const dim3 grid((H * W + 255) / 256, N);
    switch (src->C) {
        case 1: hipLaunchKernelGGL((split_rows_kernel<7, 1>), grid, dim3(256), 0, (hipStream_t)stream, p); break;
        case 2: hipLaunchKernelGGL((split_rows_kernel<7, 2>), grid, dim3(256), 0, (hipStream_t)stream, p); break;
        case 3: hipLaunchKernelGGL((split_rows_kernel<7, 3>), grid, dim3(256), 0, (hipStream_t)stream, p); break;
        default: hipLaunchKernelGGL((split_rows_kernel<7, 4>), grid, dim3(256), 0, (hipStream_t)stream, p); break;
    }
    return check_launch("split_rows_kernel");
}

int ap_split_prepass_s2d(const ap_src* src, int32_t N, int32_t H, int32_t W, void* out, ap_stream_t stream) {
    if (!src || !src->data || !out) return fail(AP_ERR_INVALID, "split_prepass_s2d: null pointer");
    if (src->C < 8 || src->C % 8 != 0 || H < 2 || W < 2 || (H & 1) || (W & 1))
        return fail(AP_ERR_UNSUPPORTED, "split_prepass_s2d: needs channels in multiples of 8 and an even map (C=%d, %dx%d)",
                    src->C, H, W);
    if (N < 1 || N > 65535 || src->C / 2 > 65535) return fail(AP_ERR_INVALID, "split_prepass_s2d: bad sizes");
    if ((src->mean == nullptr) != (src->rstd == nullptr)) return fail(AP_ERR_INVALID, "split_prepass_s2d: mean/rstd mismatch");
    if (src->act < 0 || src->act > 2) return fail(AP_ERR_INVALID, "split_prepass_s2d: act %d", src->act);
    SplitS2dParams p;
    memset(&p, 0, sizeof(p));
    p.x = src->data; p.mean = src->mean; p.rstd = src->rstd; p.act = src->act;
    p.N = N; p.C = src->C; p.H = H; p.W = W;
    p.out = reinterpret_cast<uint4*>(out);
    const int HW2 = (H / 2 + 1) * (W / 2 + 1);
    hipLaunchKernelGGL(split_s2d_kernel, dim3((HW2 + 255) / 256, src->C / 2, N), dim3(256), 0, (hipStream_t)stream, p);
    return check_launch("split_s2d_kernel");
}

int ap_split_prepass(const ap_src* src, int32_t N, int32_t H, int32_t W, void* out, ap_stream_t stream) {
    if (!src || !out) return fail(AP_ERR_INVALID, "split_prepass: null pointer");
    return ap_norm_apply_split(src, nullptr, 0, 0.f, nullptr, nullptr, nullptr, N, H, W, nullptr, out, stream);
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

int ap_conv2d_pack_weights(const ap_conv_desc* d, const float* weight, float* packed, ap_stream_t stream) {
    Plan pl;
    int rc = make_plan(d, pl);
    if (rc) return rc;
    if (!weight || !packed) return fail(AP_ERR_INVALID, "null weight/packed pointer");
    if (pl.small) {
        hipError_t e = hipMemcpyAsync(packed, weight, (size_t)pl.packed_floats * sizeof(float), hipMemcpyDeviceToDevice,
                                      (hipStream_t)stream);
        if (e != hipSuccess) return fail(AP_ERR_LAUNCH, "pack (copy) weights: %s", hipGetErrorString(e));
        return AP_OK;
    }
    if (pl.direct_cop) {
        PackDirectParams p;
        memset(&p, 0, sizeof(p));
        p.w = weight; p.out = packed;
        p.Cin = pl.Cin; p.Cout = d->Cout; p.K = d->KH; p.layout = d->w_layout; p.flip = d->w_flip;
        p.COP = pl.direct_cop; p.CI = 4; p.nchunks = pl.nchunks; p.nseg = d->nsrc;
        for (int s = 0; s < d->nsrc; ++s) { p.segC[s] = d->src[s].C; p.chunk_begin[s] = pl.chunk_begin[s]; }
        hipLaunchKernelGGL(pack_direct_kernel, dim3(64), dim3(256), 0, (hipStream_t)stream, p);
        return check_launch("pack_direct_kernel");
    }
    if (pl.bf3) {
        for (const auto& L : pl.launches) {
            const PackBf3Params p = bf3_pack_params(d, pl, L, weight, nullptr, packed);
            hipLaunchKernelGGL(pack_bf16x3_kernel, dim3(1024), dim3(256), 0, (hipStream_t)stream, p);
            rc = check_launch("pack_bf16x3_kernel");
            if (rc) return rc;
        }
        return AP_OK;
    }
    for (const auto& L : pl.launches) {
        PackParams p;
        memset(&p, 0, sizeof(p));
        p.w = weight;
        p.out = packed + L.wp_off;
        p.Cin = pl.Cin; p.Cout = d->Cout; p.K = d->KH; p.layout = d->w_layout;
        p.nseg = d->nsrc;
        for (int s = 0; s < d->nsrc; ++s) { p.segC[s] = d->src[s].C; p.chunk_begin[s] = pl.chunk_begin[s]; }
        p.CI = pl.k->CI; p.CO_TILE = pl.k->CO_TILE; p.nchunks = pl.nchunks; p.co_tiles = pl.co_tiles;
        p.ntaps = (int)L.taps.size();
        p.wfloats = pl.k->wfloats(p.ntaps);
        for (int t = 0; t < p.ntaps; ++t) { p.tap_ky[t] = L.taps[t].ky; p.tap_kx[t] = L.taps[t].kx; }
        const long long total = (long long)p.co_tiles * p.nchunks * p.wfloats;
        int blocks = (int)std::min<long long>((total + 255) / 256, 2048);
        hipLaunchKernelGGL(pack_weights_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p);
        rc = check_launch("pack_weights_kernel");
        if (rc) return rc;
    }
    if (pl.head_w_off >= 0) {
        hipError_t e = hipMemcpyAsync(packed + pl.head_w_off, weight, (size_t)pl.Cin * d->Cout * d->KH * d->KW * sizeof(float),
                                      hipMemcpyDeviceToDevice, (hipStream_t)stream);
        if (e != hipSuccess) return fail(AP_ERR_LAUNCH, "pack (head copy) weights: %s", hipGetErrorString(e));
    }
    return AP_OK;
}

int32_t ap_conv2d_pack_entry_bytes(void) { return (int32_t)sizeof(PackBf3Params); }

int32_t ap_conv2d_pack_entries(const ap_conv_desc* d, const ap_weight_view* v, float* packed, void* entries, int32_t max_entries) {
    Plan pl;
    int rc = make_plan(d, pl);
    if (rc) return rc;
    if (!v || !v->w || !packed) return fail(AP_ERR_INVALID, "pack_entries: null view / packed pointer");
    if (!pl.bf3) return 0;                                   // not a split-bf16 plan: use ap_conv2d_pack_weights
    if ((int)pl.launches.size() > max_entries || !entries) return fail(AP_ERR_INVALID, "pack_entries: room for %d entries, plan has %d", max_entries, (int)pl.launches.size());
    if ((v->s2d_c > 0 || v->rows_c > 0) && v->ksrc < 1) return fail(AP_ERR_INVALID, "pack_entries: derived views need ksrc");
    PackBf3Params* out = reinterpret_cast<PackBf3Params*>(entries);
    int n = 0;
    for (const auto& L : pl.launches) out[n++] = bf3_pack_params(d, pl, L, nullptr, v, packed);
    return n;
}

int ap_conv2d_pack_run(const void* entries_dev, int32_t count, ap_stream_t stream) {
    if (!entries_dev || count < 1 || count > 65535) return fail(AP_ERR_INVALID, "pack_run: bad table");
    hipLaunchKernelGGL(pack_bf16x3_table_kernel, dim3(48, count), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const PackBf3Params*>(entries_dev));
    return check_launch("pack_bf16x3_table_kernel");
}

}  // extern "C"

namespace apamd {

// ------------------------------------------------------------------ which plans take which output form
// the channel-octet output form exists in the run-time-tap and row families of the split-bf16 kernel (conv_bf16x3.h epilogue)
static bool octet_plan_ok(const ap_conv_desc* d, const Plan& pl) {
    if (!pl.bf3 || pl.fused_phases || pl.ph4 || pl.launches.size() != 1 || (d->Cout & 7)) return false;
    const Bf3Kernel* kern = bf3_for_taps(pl.bk, (int)pl.launches[0].taps.size());
    return kern && (kern->K == 0 || kern->ROW || (kern->K == 3 && kern->S == 1 && d->precision == AP_PRECISION_BF16X3));
}

// the bf16-output form exists for the plain-bf16 instantiations of the dense 3x3 stride-1 tiles (Bf3Cfg::OB16)
static bool ob16_plan_ok(const ap_conv_desc* d, const Plan& pl) {
    if (!pl.bf3 || pl.fused_phases || pl.ph4 || pl.launches.size() != 1 || d->precision != AP_PRECISION_BF16) return false;
    return pl.bk && pl.bk->fn1_ob16 != nullptr;
}

// the answer of an ap_conv2d_*_ok query: the descriptor has a plan and the plan passes the predicate
static int32_t plan_passes(const ap_conv_desc* d, bool (*ok)(const ap_conv_desc*, const Plan&)) {
    Plan pl;
    return !make_plan(d, pl) && ok(d, pl) ? 1 : 0;
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

// Every refusal that depends on the arguments, before anything is launched; callers tell the refusals apart, so the order stays
static int check_fwd_args(const ap_conv_desc* d, const Plan& pl, const OutForm& o, const FwdArgs& a) {
    if (o.bf16 && (!ob16_plan_ok(d, pl) || o.octet))
        return fail(AP_ERR_UNSUPPORTED, "conv2d_fwd_bf16out: only the plain-bf16 dense 3x3 stride-1 layers store bf16 (ap_conv2d_bf16out_ok)");
    if (!a.packed || !a.y) return fail(AP_ERR_INVALID, "null packed/y pointer");
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
        if (!d->src[s].data) return fail(AP_ERR_INVALID, "segment %d: null data", s);
        if ((d->src[s].mean == nullptr) != (d->src[s].rstd == nullptr))
            return fail(AP_ERR_INVALID, "segment %d: mean and rstd must be given together", s);
        if (d->src[s].act < 0 || d->src[s].act > 2) return fail(AP_ERR_INVALID, "segment %d: act %d", s, d->src[s].act);
    }
    return AP_OK;
}

static int launch_tsmall(const ap_conv_desc* d, const Plan& pl, const FwdArgs& a) {
    TSmallParams p;
    memset(&p, 0, sizeof(p));
    fill_seg(p.src, d->src[0], 0);
    p.N = d->N; p.C = pl.Cin; p.H = d->H; p.W = d->W; p.Cout = d->Cout;
    p.w = a.packed + pl.head_w_off; p.bias = a.bias; p.act = d->act; p.y = a.y;
    if (d->N > 65535 || (d->H + 7) / 8 > 65535) return fail(AP_ERR_UNSUPPORTED, "conv_tsmall: grid too large");
    const dim3 grid((d->W + 31) / 32, (d->H + 7) / 8, d->N);
    if (d->Cout == 1) hipLaunchKernelGGL((conv_tsmall_f32<1>), grid, dim3(256), 0, a.stream, p);
    else if (d->Cout == 2) hipLaunchKernelGGL((conv_tsmall_f32<2>), grid, dim3(256), 0, a.stream, p);
    else hipLaunchKernelGGL((conv_tsmall_f32<4>), grid, dim3(256), 0, a.stream, p);
    return check_launch("conv_tsmall_f32");
}

// Rows per workgroup of the head kernel.  The kernel is bound by its vector ALUs (normalisation, activation, three wave shifts and
// 16 FMAs per staged row element, on RB + 3 rows for RB outputs) and a launch is a few hundred 1024-thread workgroups: what counts
// is the number of workgroup ROUNDS on the CUs times the rows a workgroup stages.  (Round 6; before: 3-row bands unless taller
// ones still gave >= 200 workgroups -- 320 workgroups = two rounds at 2B = 32, 160 = 5/8 of the chip at B = 16.)
static int launch_head(const ap_conv_desc* d, const Plan& pl, const FwdArgs& a) {
    const int cus = num_cus();
    int rb = 3;
    long long best_cost = -1;
    for (int cand : {2, 3, 4, 5, 6, 10}) {
        const long long wgs = (long long)d->N * ((pl.Hout + cand - 1) / cand);
        const long long cost = ((wgs + cus - 1) / cus) * (cand + 3);
        if (best_cost < 0 || cost < best_cost) { rb = cand; best_cost = cost; }
    }
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
    if (d->stride == 1 && d->Cout == 8) hipLaunchKernelGGL((conv_small_f32<SmallCfg<1, 8>>), grid, dim3(256), 0, a.stream, p);
    else if (d->stride == 1) hipLaunchKernelGGL((conv_small_f32<SmallCfg<1, 16>>), grid, dim3(256), 0, a.stream, p);
    else if (d->Cout == 8) hipLaunchKernelGGL((conv_small_gather_f32<SmallCfg<2, 8>>), grid, dim3(256), 0, a.stream, p);
    else hipLaunchKernelGGL((conv_small_gather_f32<SmallCfg<2, 16>>), grid, dim3(256), 0, a.stream, p);
    return check_launch("conv_small_f32");
}

// The generator's output layer in split-bf16 arithmetic -- one reflection-padded 64-channel source, one output channel, no
// statistics epilogue -- multiplies on the matrix pipe (conv_tapgemm.h).  Same plan, same packed image: chosen here, at launch.
static bool tapgemm_serves(const ap_conv_desc* d, const Plan& pl, const FwdArgs& a) {
    return d->precision == AP_PRECISION_BF16X3 && d->Cout == 1 && d->KH == 7 && d->nsrc == 1 && d->src[0].C == TapGemmCfg::C &&
           d->pad_mode == AP_PAD_REFLECT && !a.stats && pl.cin_pad == TapGemmCfg::C;
}

// Tile height: the workgroups (two per CU) run in rounds, and a workgroup stages th + 6 rows for th output rows
static int launch_tapgemm(const ap_conv_desc* d, const Plan& pl, const FwdArgs& a) {
    const void* kfn = tapgemm_kernel();
    int rc = ensure_dyn_lds(kfn, 160 * 1024);
    if (rc) return rc;
    TapGemmParams p;
    memset(&p, 0, sizeof(p));
    fill_seg(p.seg, d->src[0], 0);
    p.N = d->N; p.H = d->H; p.W = d->W;
    p.y = a.y; p.wp = a.packed; p.bias = a.bias; p.act = d->act;
    p.tiles_x = (pl.Wout + TapGemmCfg::TW - 1) / TapGemmCfg::TW;
    const long long slots = 2LL * num_cus();
    long long best_cost = -1;
    for (int ty = 1; ty <= (pl.Hout + 7) / 8; ++ty) {
        const int th = (pl.Hout + ty - 1) / ty;
        const long long wgs = (long long)d->N * p.tiles_x * ((pl.Hout + th - 1) / th);
        const long long cost = ((wgs + slots - 1) / slots) * (th + 6);
        if (best_cost < 0 || cost < best_cost) { p.th = th; best_cost = cost; }
    }
    p.tiles_y = (pl.Hout + p.th - 1) / p.th;
    void* args[] = {&p};
    hipError_t e = hipLaunchKernel(kfn, dim3((unsigned)(d->N * p.tiles_y * p.tiles_x)), dim3(256), args, TapGemmCfg::lds_bytes(), a.stream);
    if (e != hipSuccess) return fail(AP_ERR_LAUNCH, "conv_tapgemm_bf16x3 launch: %s", hipGetErrorString(e));
    return AP_OK;
}

static int launch_direct(const ap_conv_desc* d, const Plan& pl, const FwdArgs& a) {
    if (tapgemm_serves(d, pl, a)) return launch_tapgemm(d, pl, a);
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
    p.ablate = env_int("APAMD_ABLATE", 0);
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

static int launch_igemm(const ap_conv_desc* d, const Plan& pl, const FwdArgs& a) {
    int rc = ensure_dyn_lds(pl.k->fn, 160 * 1024);
    if (rc) return rc;
    for (const auto& L : pl.launches) {
        ConvKParams p = conv_params(d, pl, L, a, true);
        p.wfloats = pl.k->wfloats(p.ntaps);
        if (pl.k->K == 0 && (rc = tap_bits(L, p.tap_bits))) return rc;
        const size_t lds = 4 * pl.k->lds_floats(p.ntaps, p.nchunks > 1 ? 2 : 1, p.cin_pad);
        const long long nblk = (long long)d->N * L.tiles_y * L.tiles_x * pl.co_tiles;
        if (nblk > 0x7fffffffLL) return fail(AP_ERR_UNSUPPORTED, "grid too large");
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
static void fused_phase_params(ConvKParams& p, const Plan& pl) {
    p.nphase = 4;
    p.co_tiles_phase = pl.co_tiles;
    p.co_tiles = pl.ph4 ? pl.co_tiles : 4 * pl.co_tiles;
    for (int ph = 0; ph < 4; ++ph) {
        const Launch& Lp = pl.launches[ph];
        p.ph_dy0[ph] = Lp.dy0; p.ph_dx0[ph] = Lp.dx0; p.ph_oy[ph] = Lp.oy_off; p.ph_ox[ph] = Lp.ox_off;
        p.ph_stat[ph] = Lp.stat_tile_off;
        p.ph_tapmask[ph] = phase_tapmask(Lp);
    }
}

// space-to-depth form of a 3x3 stride-2 layer: input phase (ry, rx) = 16-channel chunks [r C/16, (r+1) C/16)
static void s2d3_params(ConvKParams& p, const ap_conv_desc* d, const Plan& pl) {
    if (d->s2d_k != 3 || d->transposed || pl.bk->K != 0 || d->KW != 2 || d->nsrc != 1 || d->src[0].C % 64 != 0) return;
    p.s2d_div = d->src[0].C / 64;
    for (int r = 0; r < 4; ++r) {
        p.s2d_mask[r] = 0;
        for (int t = 0; t < 4; ++t)
            if (2 * (t >> 1) + (r >> 1) <= 2 && 2 * (t & 1) + (r & 1) <= 2) p.s2d_mask[r] |= 1u << t;
    }
}

// persistent workgroups, each walks its share of the tiles: one per CU, two when two stage sets fit its 160 KB of LDS
static unsigned bf3_workgroups(long long tiles, size_t lds, bool two_per_cu) {
    int cus = num_cus() * ((2 * lds <= 160 * 1024 || two_per_cu) ? 2 : 1);
    if (const int forced = env_int("APAMD_BF3_BLOCKS", 0)) {      // tuning / test knob: never silent
        static bool told = false;
        if (!told) fprintf(stderr, "libapamd: APAMD_BF3_BLOCKS=%d overrides the persistent workgroup count\n", forced);
        told = true;
        cus = forced;
    }
    return (unsigned)(tiles > cus ? cus : tiles);
}

static int launch_bf3(const ap_conv_desc* d, const Plan& pl, const OutForm& o, const FwdArgs& a) {
    if (!d->presplit)
        return fail(AP_ERR_INVALID, "this layer runs on the split-bf16 path: pass sources prepared by "
                                    "ap_split_prepass and set desc.presplit (see ap_conv2d_wants_presplit)");
    int rc = pl.ph4 ? check_ph4_plan(pl, o.view) : AP_OK;
    if (rc) return rc;
    for (const auto& L : pl.launches) {
        const Bf3Kernel* kern = pl.ph4 ? pl.bk : bf3_for_taps(pl.bk, (int)L.taps.size());
        if (!kern) return fail(AP_ERR_UNSUPPORTED, "no split-bf16 kernel for a phase with %d taps", (int)L.taps.size());
        ConvKParams p = conv_params(d, pl, L, a, false);
        p.wfloats = pl.bk->wfloats(p.ntaps);
        p.o_octet = o.octet ? 1 : 0;
        if (const ap_out_view* v = o.view) {
            // output window: a sub-grid of the output, stored with the caller's strides (ap_out_view)
            p.OH = v->OH; p.OW = v->OW;
            p.tiles_x = (v->OW + 31) / 32;
            p.tiles_y = (v->OH + pl.bk->TH - 1) / pl.bk->TH;
            p.o_nstride = v->nstride; p.o_cstride = v->cstride; p.o_rstride = v->rstride;
            p.osy = 1; p.oy_off = v->y_off;
            p.osx = v->xstride; p.ox_off = v->x_off * v->xstride;
        }
        if (pl.fused_phases) fused_phase_params(p, pl);
        s2d3_params(p, d, pl);
        if (pl.bk->K == 0 && (rc = tap_bits(L, p.tap_bits))) return rc;
        const void* kfn = o.bf16 ? kern->fn1_ob16 : kern->kernel(d->precision);
        // even chunk count per input phase: the instantiation with compile-time tap sets (no fragment reads for absent taps)
        if (p.s2d_div > 0 && (p.s2d_div & 1) == 0 && p.nchunks == 4 * p.s2d_div && kern->kernel_s2d3(d->precision))
            kfn = kern->kernel_s2d3(d->precision);
        rc = ensure_dyn_lds(kfn, 160 * 1024);
        if (rc) return rc;
        size_t lds = kern->lds(d->precision, p.ntaps);
        bool sb = false;
#ifdef APAMD_VARIANTS
        if (!o.view && !o.octet && kern->K == 3 && kern->S == 1 && kern->TH == 16 && !kern->ROW && d->precision != AP_PRECISION_BF16 &&
            p.osx == 1 && p.osy == 1 && p.oy_off == 0 && p.ox_off == 0 && env_int("APAMD_CONV_SB", 0)) {
            // rejected experiment kept for A/B (tools/variants/conv_bf16x3_sb.h, `make variants`): one LDS stage per
            // workgroup, two workgroups per CU
            kfn = bf3_sb_kernel(&lds);
            rc = ensure_dyn_lds(kfn, 160 * 1024);
            if (rc) return rc;
            p.sb_skew = env_int("APAMD_CONV_SB_SKEW", 0);
            sb = true;
        }
#endif
#ifdef APAMD_ABLATION
        // cycle account (tools/cycle_account.py): APAMD_STAMP_BUF = device address of the stamp buffer, APAMD_STAMP_WORDS =
        // dwords per wave; the stamps live in LDS behind the stage buffers, so only kernels that leave that room take them
        if (const char* sb_ = getenv("APAMD_STAMP_BUF")) {
            const int words = env_int("APAMD_STAMP_WORDS", 512);
            if (!pl.ph4 && lds + (size_t)16 * words <= 160 * 1024) {
                p.stamps = reinterpret_cast<unsigned*>(strtoull(sb_, nullptr, 0));
                p.stamp_lds_off = (int)lds;
                p.stamp_words = words;
                lds += (size_t)16 * words;
            }
        }
#endif
        if (lds > 160 * 1024) return fail(AP_ERR_UNSUPPORTED, "bf16x3 LDS tile of %zu bytes does not fit", lds);
        if (p.nchunks < 2) return fail(AP_ERR_UNSUPPORTED, "bf16x3 pipeline needs >= 32 input channels");
        if (((long long)d->H * d->W + 1) * 32 >= (1LL << 31))   // per-lane DMA offsets span two channel-group planes
            return fail(AP_ERR_UNSUPPORTED, "split-bf16 path: %d x %d planes are too large", d->H, d->W);
        const unsigned nblk = bf3_workgroups((long long)d->N * p.tiles_y * p.tiles_x * p.co_tiles, lds, sb);
        void* args[] = {&p};
        hipError_t e = hipLaunchKernel(kfn, dim3(nblk), dim3(256), args, lds, a.stream);
        if (e != hipSuccess) return fail(AP_ERR_LAUNCH, "conv_bf16x3 launch: %s", hipGetErrorString(e));
        if (pl.fused_phases) break;
    }
    return AP_OK;
}

// Every forward entry point: plan, refuse what the plan or the arguments rule out, then the family's launcher
static int conv2d_fwd_impl(const ap_conv_desc* d, const OutForm& o, const FwdArgs& a) {
    Plan pl;
    int rc = make_plan(d, pl);
    if (rc) return rc;
    rc = check_fwd_args(d, pl, o, a);
    if (rc) return rc;
    // (with a statistics epilogue wanted the two narrow-output layers stay on the general kernel)
    if (pl.tsmall && !a.stats) return launch_tsmall(d, pl, a);
    if (pl.head && !a.stats) return launch_head(d, pl, a);
    if (pl.small) return launch_small(d, pl, a);
    if (pl.bf3) return launch_bf3(d, pl, o, a);
    if (pl.direct_cop) return launch_direct(d, pl, a);
    return launch_igemm(d, pl, a);
}

}  // namespace apamd

extern "C" {

int32_t ap_conv2d_octet_ok(const ap_conv_desc* d) { return plan_passes(d, octet_plan_ok); }
int32_t ap_conv2d_bf16out_ok(const ap_conv_desc* d) { return plan_passes(d, ob16_plan_ok); }

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

int ap_conv2d_fwd_view_bf16out(const ap_conv_desc* d, const ap_out_view* view, const float* packed, const float* bias, void* y_bf16,
                               ap_stream_t stream) {
    if (!view) return fail(AP_ERR_INVALID, "conv2d_fwd_view_bf16out: null view");
    OutForm o;
    o.view = view;
    o.bf16 = true;
    return conv2d_fwd_impl(d, o, {packed, bias, reinterpret_cast<float*>(y_bf16), nullptr, (hipStream_t)stream});
}

}  // extern "C"
