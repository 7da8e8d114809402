// conv_prepass_host.hip -- C ABI of the streaming passes around the split-bf16 convolutions (conv_prepass.h): the split copies a
// layer stages (plain, row form, space-to-depth form) and the norm / residual / split pass between two convolutions.  No plan.
#include "common.h"
#include "conv_prepass.h"

#include <cstring>
#include <type_traits>

using namespace apamd;

extern "C" {

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
    if (src->act < 0 || src->act > 2) return fail(AP_ERR_INVALID, "split_prepass_rows: act %d", src->act);
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

}  // extern "C"
