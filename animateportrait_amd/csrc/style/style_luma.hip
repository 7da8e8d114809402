// style_luma.hip -- luminance of a 3-channel cartoon frame and its backward (include/animateportrait_style.h: aps_luma_*),
// the one kernel cartoon TRAINING adds: the identity loss reads 0.299 R + 0.587 G + 0.114 B of the generated frame and of
// the static cartoon (Module2/models/geomgm_ifw_cartoon_fore_model.py:745-748), where the drawing model has one channel.
//
// HBM-bound: 4 planes moved per pixel each way, nothing reused.  Each lane moves one item per plane and round: a float4
// (global_load/store_dwordx4) when the plan found every plane start 16-byte aligned, a float otherwise.  Contraction is
// switched off for this file (the pragma below: HIP's __fmul_rn / __fadd_rn are plain operators and would still fuse), so
// every product and sum is rounded on its own: the result has the bits of the reference's ATen chain
// (0.299 * R + 0.587 * G) + 0.114 * B.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "style_checks.h"

#pragma clang fp contract(off)

namespace {

constexpr float kR = 0.299f, kG = 0.587f, kB = 0.114f;

template <int V> struct Item;
template <> struct Item<1> { using T = float; };
template <> struct Item<4> { using T = float4; };

__device__ __forceinline__ float luma(float r, float g, float b) {
    return (kR * r + kG * g) + kB * b;
}
__device__ __forceinline__ float4 luma(float4 r, float4 g, float4 b) {
    return make_float4(luma(r.x, g.x, b.x), luma(r.y, g.y, b.y), luma(r.z, g.z, b.z), luma(r.w, g.w, b.w));
}
__device__ __forceinline__ float scaled(float k, float v) { return k * v; }
__device__ __forceinline__ float4 scaled(float k, float4 v) {
    return make_float4(k * v.x, k * v.y, k * v.z, k * v.w);
}

// grid (blocks, N); x: N x 3 x items, y: N x items
template <int V>
__global__ __launch_bounds__(256) void luma_fwd_kernel(const typename Item<V>::T* __restrict__ x, long items,
                                                       typename Item<V>::T* __restrict__ y) {
    const long n = blockIdx.y;
    const typename Item<V>::T* xr = x + n * 3 * items;
    typename Item<V>::T* yr = y + n * items;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long)gridDim.x * 256)
        yr[i] = luma(xr[i], xr[items + i], xr[2 * items + i]);
}

// grid (blocks, N); g: N x items, gx: N x 3 x items
template <int V>
__global__ __launch_bounds__(256) void luma_bwd_kernel(const typename Item<V>::T* __restrict__ g, long items,
                                                       typename Item<V>::T* __restrict__ gx) {
    const long n = blockIdx.y;
    const typename Item<V>::T* gr = g + n * items;
    typename Item<V>::T* xr = gx + n * 3 * items;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long)gridDim.x * 256) {
        const typename Item<V>::T v = gr[i];
        xr[i] = scaled(kR, v);
        xr[items + i] = scaled(kG, v);
        xr[2 * items + i] = scaled(kB, v);
    }
}

int launched(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(aps::err_buf(), 256, "%s: launch failed: %s", what, hipGetErrorString(e));
        return APS_ERR_LAUNCH;
    }
    return APS_OK;
}

}  // namespace

extern "C" {

int32_t aps_luma_ok(const float* in, const float* out, int32_t N, int32_t H, int32_t W) {
    aps::LumaPlan pl;
    return aps::plan_luma("luma", in, out, N, H, W, &pl) == APS_OK ? 1 : 0;
}

int aps_luma_fwd(const float* x, int32_t N, int32_t H, int32_t W, float* y, void* stream) {
    aps::LumaPlan pl;
    const int rc = aps::plan_luma("luma_fwd", x, y, N, H, W, &pl);
    if (rc != APS_OK) return rc;
    (void)hipGetLastError();
    if (pl.vec == 4)
        hipLaunchKernelGGL(luma_fwd_kernel<4>, dim3(pl.blocks, N), dim3(256), 0, (hipStream_t)stream, (const float4*)x, pl.items,
                           (float4*)y);
    else
        hipLaunchKernelGGL(luma_fwd_kernel<1>, dim3(pl.blocks, N), dim3(256), 0, (hipStream_t)stream, x, pl.items, y);
    return launched("luma_fwd");
}

int aps_luma_bwd(const float* g, int32_t N, int32_t H, int32_t W, float* gx, void* stream) {
    aps::LumaPlan pl;
    const int rc = aps::plan_luma("luma_bwd", g, gx, N, H, W, &pl);
    if (rc != APS_OK) return rc;
    (void)hipGetLastError();
    if (pl.vec == 4)
        hipLaunchKernelGGL(luma_bwd_kernel<4>, dim3(pl.blocks, N), dim3(256), 0, (hipStream_t)stream, (const float4*)g, pl.items,
                           (float4*)gx);
    else
        hipLaunchKernelGGL(luma_bwd_kernel<1>, dim3(pl.blocks, N), dim3(256), 0, (hipStream_t)stream, g, pl.items, gx);
    return launched("luma_bwd");
}

}  // extern "C"
