// edge_host.hip -- C ABI of the edge layers' forward and data-gradient kernels on the bf16 matrix pipe:
//   ap_conv_final_dgrad_bf16   data gradient of the generator's last 7x7 layer (dgrad_k7.h: dgrad_k7_final_kernel)
//   ap_conv_head_dgrad_bf16    data gradient of the PatchGAN's output layer (dgrad_k7.h: dgrad_head_kernel)
//   ap_conv_d0_fwd_bf16        the PatchGAN's first layer as an output stream (conv_d0.h)
// Their weight gradients are in wgrad_edge_host.hip (the last layer's vector-ALU one, ap_conv_final_wgrad, in wgrad_launch.hip).
#include "common.h"
#include "wgrad_k7.h"
#include "dgrad_k7.h"
#include "conv_d0.h"

#include <algorithm>
#include <cstring>

using namespace apamd;

extern "C" {

// ---- data gradient of the last layer on the bf16 matrix pipe (dgrad_k7.h)
int32_t ap_conv_final_dgrad_bf16_ok(int32_t N, int32_t C, int32_t H, int32_t W) {
    return (N >= 1 && (C == 32 || C == 64) && H >= 1 && W >= 16 && W <= 256 && (W & 15) == 0) ? 1 : 0;
}

int64_t ap_conv_final_dgrad_bf16_workspace_floats(int32_t N, int32_t C, int32_t H, int32_t W) {
    if (!ap_conv_final_dgrad_bf16_ok(N, C, H, W)) return fail(AP_ERR_UNSUPPORTED, "conv_final_dgrad_bf16: shape not served");
    return round4(((long long)N * (H + 12) * 2 * (W + 16) + 1) / 2);
}

int ap_conv_final_dgrad_bf16(const float* g, const float* w, int32_t N, int32_t C, int32_t H, int32_t W, float* workspace, float* gp,
                             ap_stream_t stream_) {
    if (!g || !w || !workspace || !gp) return fail(AP_ERR_INVALID, "conv_final_dgrad_bf16: null pointer");
    if (!ap_conv_final_dgrad_bf16_ok(N, C, H, W))
        return fail(AP_ERR_UNSUPPORTED, "conv_final_dgrad_bf16: N=%d C=%d %dx%d not served (C 32 / 64, W a multiple of 16 in 16..256)", N, C, H, W);
    hipStream_t stream = (hipStream_t)stream_;
    const int A = H + 12, NW = W + 16;
    K7NarrowParams np;
    np.src = g; np.dst = reinterpret_cast<unsigned*>(workspace);
    np.N = N; np.CN = 1; np.H = H; np.W = W; np.A = A; np.NW = NW; np.final_form = 1;
    const long long ndw = (long long)N * A * (NW / 2);
    hipLaunchKernelGGL(wgrad_k7_narrow_kernel, dim3((unsigned)std::min<long long>((ndw + 255) / 256, 4096)), dim3(256), 0, stream, np);
    int rc = check_launch("wgrad_k7_narrow_kernel");
    if (rc) return rc;
    DgradK7Params p;
    memset(&p, 0, sizeof(p));
    p.narrow = reinterpret_cast<const unsigned short*>(workspace);
    p.w = w; p.gp = gp; p.N = N; p.C = C; p.H = H; p.W = W; p.HP = H + 6; p.WP = W + 6; p.A = A; p.NW = NW;
    // one workgroup per CU (its LDS row buffers fill one): whole rounds of workgroups where the row count allows
    const RowSplit rs = split_rows(N, p.HP, false);
    p.RB = rs.RB;
    p.blocks_per_img = rs.bpi;
    const size_t lds = (size_t)2 * C * ((p.WP + 7) & ~7) * 4 + (size_t)(kDgradK7Rows + 7) * 2 * (NW + 8) * 2;
    const void* fn = C == 64 ? reinterpret_cast<const void*>(&dgrad_k7_final_kernel<2>) : reinterpret_cast<const void*>(&dgrad_k7_final_kernel<1>);
    rc = ensure_dyn_lds(fn, 160 * 1024);
    if (rc) return rc;
    void* args[] = {&p};
    hipError_t e = hipLaunchKernel(fn, dim3(rs.grid), dim3(512), args, lds, stream);
    if (e != hipSuccess) return fail(AP_ERR_LAUNCH, "dgrad_k7 launch: %s", hipGetErrorString(e));
    return AP_OK;
}

// ---- data gradient of the PatchGAN's output layer (dgrad_k7.h: dgrad_head_kernel)
int32_t ap_conv_head_dgrad_bf16_ok(int32_t N, int32_t C, int32_t H, int32_t W) {
    // H W <= 1156: the 32 output planes assembled in LDS; (H + 3) (W + 8) <= 7 * 256: the zero-framed gradient rows that
    // dgrad_head_kernel stages with NI = 7 loads per thread (a long thin map within the first bound needs more: 6 x 192, 4 x 289)
    return (N >= 1 && C >= 32 && (C & 31) == 0 && H >= 2 && W >= 2 && H <= 1156 && W <= 1156 && H * W <= 1156 &&
            (H + 3) * (W + 8) <= 7 * 256 && (long long)N * (C / 32) < 2147483647LL) ? 1 : 0;
}

int ap_conv_head_dgrad_bf16(const float* g, const float* w, int32_t N, int32_t C, int32_t H, int32_t W, float* gx, ap_stream_t stream_) {
    if (!g || !w || !gx) return fail(AP_ERR_INVALID, "conv_head_dgrad_bf16: null pointer");
    if (!ap_conv_head_dgrad_bf16_ok(N, C, H, W))
        return fail(AP_ERR_UNSUPPORTED, "conv_head_dgrad_bf16: N=%d C=%d %dx%d not served (C a multiple of 32, H W <= 1156, (H + 3) (W + 8) <= 1792)", N, C, H, W);
    DgradHeadParams p;
    p.g = g; p.w = w; p.gx = gx; p.N = N; p.C = C; p.H = H; p.W = W;
    const size_t lds = (size_t)32 * H * W * 4 + (size_t)(H + 3) * 2 * (W + 8) * 2;
    const void* fn = reinterpret_cast<const void*>(&dgrad_head_kernel);
    int rc = ensure_dyn_lds(fn, 160 * 1024);
    if (rc) return rc;
    void* args[] = {&p};
    hipError_t e = hipLaunchKernel(fn, dim3(N * (C / 32)), dim3(256), args, lds, (hipStream_t)stream_);
    if (e != hipSuccess) return fail(AP_ERR_LAUNCH, "dgrad_head launch: %s", hipGetErrorString(e));
    return AP_OK;
}

// ---- the PatchGAN's first layer as an output stream on the bf16 matrix pipe (conv_d0.h)
int32_t ap_conv_d0_fwd_bf16_ok(int32_t N, int32_t Cin, int32_t Cout, int32_t H, int32_t W) {
    return (N >= 1 && (Cin == 1 || Cin == 2) && Cout == 64 && H >= 2 && (H & 1) == 0 && W >= 8 && W <= 256 && (W & 3) == 0) ? 1 : 0;
}

int ap_conv_d0_fwd_bf16(const float* x, const float* w, const float* bias, int32_t N, int32_t Cin, int32_t Cout, int32_t H, int32_t W,
                        int32_t act, float* y, ap_stream_t stream_) {
    if (!x || !w || !y) return fail(AP_ERR_INVALID, "conv_d0_fwd_bf16: null pointer");
    if (!ap_conv_d0_fwd_bf16_ok(N, Cin, Cout, H, W))
        return fail(AP_ERR_UNSUPPORTED, "conv_d0_fwd_bf16: N=%d %d -> %d channels %dx%d not served (1 | 2 -> 64, even H, W %% 4 == 0, W <= 256)",
                    N, Cin, Cout, H, W);
    if (act < 0 || act > 2) return fail(AP_ERR_UNSUPPORTED, "conv_d0_fwd_bf16: act %d", act);
    ConvD0Params p;
    memset(&p, 0, sizeof(p));
    p.x = x; p.w = w; p.bias = bias; p.y = y; p.N = N; p.H = H; p.W = W; p.OH = H / 2; p.OW = W / 2; p.act = act;
    p.blocks_per_img = (p.OH + kConvD0Rows - 1) / kConvD0Rows;
    const size_t lds = (size_t)Cin * (2 * kConvD0Rows + 2) * (W + 8) * 2;
    hipStream_t stream = (hipStream_t)stream_;
    if (Cin == 1) hipLaunchKernelGGL(conv_d0_kernel<1>, dim3(N * p.blocks_per_img), dim3(512), lds, stream, p);
    else hipLaunchKernelGGL(conv_d0_kernel<2>, dim3(N * p.blocks_per_img), dim3(512), lds, stream, p);
    return check_launch("conv_d0_kernel");
}

}  // extern "C"
