// act_bwd.hip -- backward of the layers WITHOUT InstanceNorm: ap_act_bwd (dy = (fold(g1) + g2) * act'(out); with act NONE the
// residual stream's fold + add), ap_act_bwd_bias (the same with the layer's bias gradient from the same pass) and the bias
// gradient of an existing dy (ap_bias_grad, ap_bias_grad_ws).
#include "bwd_stream.h"

namespace apamd {

// dy = (fold(g1) + g2) * act'(out): act 1 relu / 2 lrelu (sign of the ACTIVATED output) / 3 tanh (1 - out^2)
// SUMS: the block's sum of dy goes to sums[(c * N + n) * gridDim.x + blockIdx.x] -- the partials bias_grad_final_kernel adds in fixed
// order: the bias gradient of a layer without InstanceNorm (the PatchGAN's first layer: 64 x 128 x 128 per image) costs no second pass
// over dy (round 6; bias_grad_partial_kernel re-read 1.1 GB per train step)
template <bool SUMS>
__global__ __launch_bounds__(256) void act_bwd_kernel(const float* __restrict__ g1, int p1, const float* __restrict__ g2,
                                                      const float* __restrict__ outv, int act, int H, int W,
                                                      float* __restrict__ dy, float* __restrict__ sums = nullptr, int C = 1) {
    __shared__ float sred[8];
    float ssum = 0.f;
    const int nc = blockIdx.y;
    const int HW = H * W;
    FoldReader fr{g1 + (long long)nc * (H + 2 * p1) * (W + 2 * p1), H, W, p1, W + 2 * p1};
    const float* op = outv ? outv + (long long)nc * HW : nullptr;
    const float* g2p = g2 ? g2 + (long long)nc * HW : nullptr;
    float* out = dy + (long long)nc * HW;
    if (p1 == 0 && (HW & 3) == 0) {
        const float4* ga = reinterpret_cast<const float4*>(g1 + (long long)nc * HW);
        const float4* gb = g2p ? reinterpret_cast<const float4*>(g2p) : nullptr;
        const float4* o4 = op ? reinterpret_cast<const float4*>(op) : nullptr;
        for (int i = blockIdx.x * 256 + threadIdx.x; i < HW / 4; i += gridDim.x * 256) {
            float4 gv = ga[i];
            if (gb) { const float4 t = gb[i]; gv.x += t.x; gv.y += t.y; gv.z += t.z; gv.w += t.w; }
            if (act != 0) {
                const float4 ov = o4[i];
                if (act == 1) {
                    gv.x = ov.x > 0.f ? gv.x : 0.f; gv.y = ov.y > 0.f ? gv.y : 0.f;
                    gv.z = ov.z > 0.f ? gv.z : 0.f; gv.w = ov.w > 0.f ? gv.w : 0.f;
                } else if (act == 2) {
                    gv.x = ov.x > 0.f ? gv.x : 0.2f * gv.x; gv.y = ov.y > 0.f ? gv.y : 0.2f * gv.y;
                    gv.z = ov.z > 0.f ? gv.z : 0.2f * gv.z; gv.w = ov.w > 0.f ? gv.w : 0.2f * gv.w;
                } else if (act == 3) {
                    gv.x *= tanh_grad(ov.x); gv.y *= tanh_grad(ov.y);
                    gv.z *= tanh_grad(ov.z); gv.w *= tanh_grad(ov.w);
                }
            }
            reinterpret_cast<float4*>(out)[i] = gv;
            if constexpr (SUMS) ssum += (gv.x + gv.y) + (gv.z + gv.w);
        }
    } else {
    // four elements per thread and trip, every load before the first store (one at a time this loop was four serial
    // memory round trips per thread: 150 us on the residual stream's 32 x 256 x 64 x 64 fold, 2.7 TB/s)
    for (int base = blockIdx.x * 1024; base < HW; base += gridDim.x * 1024) {
        float g[4], o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = base + k * 256 + threadIdx.x;
            g[k] = 0.f; o[k] = 0.f;
            if (i < HW) {
                const int yy = i / W, xx = i - yy * W;
                g[k] = fr.at(yy, xx);
                if (g2p) g[k] += g2p[i];
                if (act != 0) o[k] = op[i];
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = base + k * 256 + threadIdx.x;
            if (i < HW) {
                float v = g[k];
                if (act == 1) v = o[k] > 0.f ? v : 0.f;
                else if (act == 2) v = o[k] > 0.f ? v : 0.2f * v;
                else if (act == 3) v *= tanh_grad(o[k]);
                out[i] = v;
                if constexpr (SUMS) ssum += v;
            }
        }
    }
    }
    if constexpr (SUMS) {
        ssum = block_sum(ssum, sred);
        if (threadIdx.x == 0) {
            const int n = nc / C, c = nc - n * C, N = gridDim.y / C;
            sums[((long long)c * N + n) * gridDim.x + blockIdx.x] = ssum;
        }
    }
}

// act_bwd for the gradient of a pad-1 reflection-padded convolution (the residual stream's fold + add), W % 4 == 0:
// a thread produces four consecutive pixels of a row (fold1_at4).
// grid: (ceil(H * W / 4 / 512), N*C)
__global__ __launch_bounds__(256) void act_bwd_fold1_kernel(const float* __restrict__ g1, const float* __restrict__ g2,
                                                            const float* __restrict__ outv, int act, int H, int W,
                                                            float* __restrict__ dy) {
    const int nc = blockIdx.y;
    const int HW = H * W, W4 = W >> 2;
    const float* gp = g1 + (long long)nc * (H + 2) * (W + 2);
    const float4* gb = g2 ? reinterpret_cast<const float4*>(g2 + (long long)nc * HW) : nullptr;
    const float4* o4 = outv ? reinterpret_cast<const float4*>(outv + (long long)nc * HW) : nullptr;
    float4* out = reinterpret_cast<float4*>(dy + (long long)nc * HW);
    float4 acc[2], add[2], ov[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int i = (blockIdx.x * 2 + k) * 256 + threadIdx.x;
        acc[k] = add[k] = ov[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < HW / 4) {
            const int y = i / W4;
            acc[k] = fold1_at4(gp, H, W, y, (i - y * W4) * 4);
            if (gb) add[k] = gb[i];
            if (act != 0) ov[k] = o4[i];
        }
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int i = (blockIdx.x * 2 + k) * 256 + threadIdx.x;
        if (i < HW / 4) {
            float4 gv = make_float4(acc[k].x + add[k].x, acc[k].y + add[k].y, acc[k].z + add[k].z, acc[k].w + add[k].w);
            const float4 o = ov[k];
            if (act == 1) {
                gv.x = o.x > 0.f ? gv.x : 0.f; gv.y = o.y > 0.f ? gv.y : 0.f;
                gv.z = o.z > 0.f ? gv.z : 0.f; gv.w = o.w > 0.f ? gv.w : 0.f;
            } else if (act == 2) {
                gv.x = o.x > 0.f ? gv.x : 0.2f * gv.x; gv.y = o.y > 0.f ? gv.y : 0.2f * gv.y;
                gv.z = o.z > 0.f ? gv.z : 0.2f * gv.z; gv.w = o.w > 0.f ? gv.w : 0.2f * gv.w;
            } else if (act == 3) {
                gv.x *= tanh_grad(o.x); gv.y *= tanh_grad(o.y); gv.z *= tanh_grad(o.z); gv.w *= tanh_grad(o.w);
            }
            out[i] = gv;
        }
    }
}

// grid: (C).  db[c] = sum_{n, pix} dy[n, c, pix]
__global__ __launch_bounds__(256) void bias_grad_kernel(const float* __restrict__ dy, int N, int C, int HW,
                                                        float* __restrict__ db) {
    __shared__ float red[8];
    const int c = blockIdx.x;
    float s = 0.f;
    for (int n = 0; n < N; ++n) {
        const float* p = dy + ((long long)n * C + c) * HW;
        for (int i = threadIdx.x; i < HW; i += 256) s += p[i];
    }
    s = block_sum(s, red);
    if (threadIdx.x == 0) db[c] = s;
}

// Two-stage form for few channels (C = 1: the final layer of the generator and of every PatchGAN): stage 1 reduces
// SPLIT slices of every (n, c) plane in parallel, stage 2 adds the N * SPLIT partials of a channel in a fixed order.
__global__ __launch_bounds__(256) void bias_grad_partial_kernel(const float* __restrict__ dy, int C, int HW, int split,
                                                                float* __restrict__ ws) {
    __shared__ float red[8];
    const int c = blockIdx.x, n = blockIdx.y, sp = blockIdx.z;
    const int per = (HW + split - 1) / split;
    const int lo = sp * per, hi = lo + per < HW ? lo + per : HW;
    const float* p = dy + ((long long)n * C + c) * HW;
    float s = 0.f;
    for (int i = lo + threadIdx.x; i < hi; i += 256) s += p[i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) ws[((long long)c * gridDim.y + n) * split + sp] = s;
}

__global__ __launch_bounds__(64) void bias_grad_final_kernel(const float* __restrict__ ws, int count, float* __restrict__ db) {
    const int c = blockIdx.x;
    if (threadIdx.x != 0) return;
    float s = 0.f;
    for (int i = 0; i < count; ++i) s += ws[(long long)c * count + i];
    db[c] = s;
}

// db[c] = sum of the count block sums act_bwd_kernel<true> left for channel c: lane t adds elements t, t + 64, ..., then the
// lanes are added as a fixed tree
__global__ __launch_bounds__(64) void bias_sums_final_kernel(const float* __restrict__ ws, int count, float* __restrict__ db) {
    const int c = blockIdx.x;
    float s = 0.f;
    for (int i = threadIdx.x; i < count; i += 64) s += ws[(long long)c * count + i];
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) s += __shfl_xor(s, sh, 64);
    if (threadIdx.x == 0) db[c] = s;
}

}  // namespace apamd

using namespace apamd;

// Which kernel ap_act_bwd launches for a plane geometry: the one place that decides it (ap_act_bwd_route names the answer)
enum ActBwdRoute {
    ACTBWD_FOLD1,           // act_bwd_fold1_kernel: pad-1 fold, W % 4 == 0, H >= 3
    ACTBWD_GENERIC,         // act_bwd_kernel: 16-byte lanes for an unfolded gradient with H W % 4 == 0, else element-wise with FoldReader
};

static int act_bwd_route(int g1_pad, int H, int W, ActBwdRoute* route) {
    int rc = fold_pad_ok(g1_pad, H, W, "act_bwd");
    if (rc) return rc;
    *route = g1_pad == 1 && (W & 3) == 0 && H >= 3 && W >= 4 ? ACTBWD_FOLD1 : ACTBWD_GENERIC;
    return AP_OK;
}

extern "C" {

int ap_act_bwd(const float* g1, int32_t g1_pad, const float* g2, const float* out, int32_t act, int32_t NC,
               int32_t H, int32_t W, float* dy, ap_stream_t stream) {
    int rc = fold_args_ok(g1, g1_pad, H, W, "act_bwd");
    if (rc) return rc;
    if (!dy || (act != AP_ACT_NONE && !out)) return fail(AP_ERR_INVALID, "act_bwd: null pointer");
    if (act < 0 || act > 3) return fail(AP_ERR_INVALID, "act_bwd: act %d", act);
    if (NC < 1 || NC > 65535) return fail(AP_ERR_UNSUPPORTED, "act_bwd: N*C=%d", NC);
    ActBwdRoute route;
    rc = act_bwd_route(g1_pad, H, W, &route);
    if (rc) return rc;
    if (route == ACTBWD_FOLD1) {
        hipLaunchKernelGGL(act_bwd_fold1_kernel, dim3((H * W / 4 + 511) / 512, NC), dim3(256), 0, (hipStream_t)stream, g1,
                           g2, out, act, H, W, dy);
        return check_launch("act_bwd_fold1_kernel");
    }
    hipLaunchKernelGGL(act_bwd_kernel<false>, dim3(sweep_blocks(H, W), NC), dim3(256), 0, (hipStream_t)stream, g1, g1_pad, g2, out,
                       act, H, W, dy, (float*)nullptr, 1);
    return check_launch("act_bwd_kernel");
}

int ap_act_bwd_route(int32_t g1_pad, int32_t H, int32_t W, char* buf, int32_t buflen) {
    ActBwdRoute route;
    int rc = act_bwd_route(g1_pad, H, W, &route);
    if (rc) return rc;
    if (!buf || buflen < 1) return fail(AP_ERR_INVALID, "act_bwd_route: bad buffer");
    snprintf(buf, buflen, "%s", route == ACTBWD_FOLD1 ? "act_fold1" : "act_generic");
    return AP_OK;
}

// act_bwd + the bias gradient db[c] = sum_{n, y, x} dy of the same layer in one pass (workspace: ap_act_bwd_bias_workspace_floats)
int64_t ap_act_bwd_bias_workspace_floats(int32_t N, int32_t C, int32_t H, int32_t W) {
    if (N < 1 || C < 1 || H < 1 || W < 1) return fail(AP_ERR_INVALID, "act_bwd_bias: bad sizes");
    return (int64_t)N * C * sweep_blocks(H, W);
}

int ap_act_bwd_bias(const float* g1, int32_t g1_pad, const float* g2, const float* out, int32_t act, int32_t N, int32_t C,
                    int32_t H, int32_t W, float* dy, float* workspace, float* db, ap_stream_t stream) {
    int rc = fold_args_ok(g1, g1_pad, H, W, "act_bwd_bias");
    if (rc) return rc;
    if (!dy || !workspace || !db || (act != AP_ACT_NONE && !out)) return fail(AP_ERR_INVALID, "act_bwd_bias: null pointer");
    if (act < 0 || act > 3) return fail(AP_ERR_INVALID, "act_bwd_bias: act %d", act);
    if (N < 1 || C < 1 || (long long)N * C > 65535) return fail(AP_ERR_UNSUPPORTED, "act_bwd_bias: N*C=%lld", (long long)N * C);
    const int bx = sweep_blocks(H, W);
    hipLaunchKernelGGL(act_bwd_kernel<true>, dim3(bx, N * C), dim3(256), 0, (hipStream_t)stream, g1, g1_pad, g2, out, act, H, W, dy,
                       workspace, C);
    rc = check_launch("act_bwd_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(bias_sums_final_kernel, dim3(C), dim3(64), 0, (hipStream_t)stream, workspace, N * bx, db);
    return check_launch("bias_sums_final_kernel");
}

int ap_bias_grad(const float* dy, int32_t N, int32_t C, int32_t HW, float* db, ap_stream_t stream) {
    if (!dy || !db || N < 1 || C < 1 || HW < 1) return fail(AP_ERR_INVALID, "bias_grad: bad arguments");
    hipLaunchKernelGGL(bias_grad_kernel, dim3(C), dim3(256), 0, (hipStream_t)stream, dy, N, C, HW, db);
    return check_launch("bias_grad_kernel");
}

static int bias_grad_split(int N, int C, int HW) {
    // enough slices to put ~2 workgroups on every CU, each still streaming >= 4096 elements
    int split = 512 / (N * C > 0 ? N * C : 1);
    const int cap = HW / 4096;
    if (split > cap) split = cap;
    return split < 1 ? 1 : split;
}

int64_t ap_bias_grad_workspace_floats(int32_t N, int32_t C, int32_t HW) {
    if (N < 1 || C < 1 || HW < 1) return fail(AP_ERR_INVALID, "bias_grad: bad arguments");
    return (int64_t)N * C * bias_grad_split(N, C, HW);
}

int ap_bias_grad_ws(const float* dy, int32_t N, int32_t C, int32_t HW, float* workspace, float* db, ap_stream_t stream) {
    if (!dy || !db || !workspace || N < 1 || C < 1 || HW < 1) return fail(AP_ERR_INVALID, "bias_grad: bad arguments");
    if (N > 65535) return fail(AP_ERR_UNSUPPORTED, "bias_grad: N too large");
    const int split = bias_grad_split(N, C, HW);
    hipLaunchKernelGGL(bias_grad_partial_kernel, dim3(C, N, split), dim3(256), 0, (hipStream_t)stream, dy, C, HW, split,
                       workspace);
    int rc = check_launch("bias_grad_partial_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(bias_grad_final_kernel, dim3(C), dim3(64), 0, (hipStream_t)stream, workspace, N * split, db);
    return check_launch("bias_grad_final_kernel");
}

}  // extern "C"
