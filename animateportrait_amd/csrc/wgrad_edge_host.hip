// wgrad_edge_host.hip -- C ABI of the weight gradients of the layers with kernels of their own: the PatchGAN's output layer
// (ap_conv_head_wgrad, conv_head.h), the 7x7 edge layers at full resolution on the bf16 matrix pipe (ap_wgrad_k7_bf16) and the
// PatchGAN's first layer (ap_wgrad_d0_bf16; both wgrad_k7.h).  None of them touches WgradPlan.  Their forward and data-gradient
// entry points are in edge_host.hip.  (The last layer's vector-ALU weight gradient, ap_conv_final_wgrad, is in wgrad_launch.hip.)
#include "common.h"
#include "conv_head.h"      // conv_head_wgrad_kernel, kHeadMaxW / kHeadMaxH (the forward kernel: conv_fwd.hip)
#include "wgrad_k7.h"

#include <algorithm>
#include <cstring>

namespace apamd {

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

}  // namespace apamd

using namespace apamd;

extern "C" {

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
