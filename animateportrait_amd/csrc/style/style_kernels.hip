// libapstyle.so: aps_lin_coeffs, aps_affine_apply, aps_plane_combine (include/animateportrait_style.h) -- what the static
// cartoon generator (Photo2Cartoon, photo2cartoon.py:166-525) needs around its convolutions.
//
// Every kernel runs one workgroup per (output) plane: the planes are at most 256 x 256 and there are at most a few thousand
// of them, and a plane's statistics then need no second launch and no atomics.  A 256 x 256 plane (256 KiB) does not fit the
// LDS, so nothing is staged: a lane walks the plane with a stride of the workgroup size (coalesced), and a second walk -- for the
// sum of squared deviations from the mean, the two-pass safeguard -- re-reads what the SAME lane read or wrote in the first one
// (program order makes its own stores visible to it; the lines come back from L2).  Sums are kept in fp64: per lane at most
// 4096^2 / 256 terms, then a wave shuffle tree and one LDS round over the waves.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "style_checks.h"

namespace {

using aps::fail;
using aps::PlanePlan;

constexpr float IN_EPS = 1e-5f;       // nn.InstanceNorm2d's default, as ops.EPS
constexpr int MAX_WAVES = 16;         // 1024 lanes

// the sum of `v` over the workgroup, in every lane
__device__ __forceinline__ double block_sum(double v, double* lds) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    const int wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    __syncthreads();                  // (the previous round's readers are done with lds)
    if ((threadIdx.x & 63) == 0) lds[wave] = v;
    __syncthreads();
    double t = 0.0;
    for (int i = 0; i < nw; ++i) t += lds[i];
    return t;
}

// ---------------------------------------------------------------------------------------------- aps_lin_coeffs
__global__ __launch_bounds__(1024) void plane_moments_kernel(const float* __restrict__ x, int hw, float* __restrict__ planes) {
    __shared__ double lds[MAX_WAVES];
    const float* p = x + (size_t)blockIdx.x * hw;
    double s = 0.0;
    for (int i = threadIdx.x; i < hw; i += blockDim.x) s += (double)p[i];
    const double mean = block_sum(s, lds) / hw;
    double m2 = 0.0;
    for (int i = threadIdx.x; i < hw; i += blockDim.x) {
        const double d = (double)p[i] - mean;
        m2 += d * d;
    }
    m2 = block_sum(m2, lds);
    if (threadIdx.x == 0) {
        planes[2 * (size_t)blockIdx.x] = (float)mean;
        planes[2 * (size_t)blockIdx.x + 1] = (float)m2;
    }
}

// one workgroup per sample: the layer's moments from the planes' (count hw, mean, M2) by the parallel formula
//   mean = sum mean_c / C,   M2 = sum M2_c + hw sum (mean_c - mean)^2
__global__ __launch_bounds__(256) void lin_fold_kernel(const float* __restrict__ planes, const float* __restrict__ rho,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta, int C, int hw,
                                                       int per_sample, float eps, float* __restrict__ a, float* __restrict__ b) {
    __shared__ double lds[MAX_WAVES];
    const size_t base = (size_t)blockIdx.x * C;
    double s = 0.0;
    for (int c = threadIdx.x; c < C; c += blockDim.x) s += (double)planes[2 * (base + c)];
    const double mean_ln = block_sum(s, lds) / C;
    double m2 = 0.0;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        const double d = (double)planes[2 * (base + c)] - mean_ln;
        m2 += (double)planes[2 * (base + c) + 1] + (double)hw * d * d;
    }
    m2 = block_sum(m2, lds);
    const double rstd_ln = 1.0 / sqrt(m2 / ((double)C * hw - 1.0) + (double)eps);
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        const double mean_in = planes[2 * (base + c)];
        const double rstd_in = 1.0 / sqrt((double)planes[2 * (base + c) + 1] / (hw - 1.0) + (double)eps);
        const double r = rho[c];
        const double g = gamma[per_sample ? base + c : c], bt = beta[per_sample ? base + c : c];
        a[base + c] = (float)(g * (r * rstd_in + (1.0 - r) * rstd_ln));
        b[base + c] = (float)(bt - g * (r * mean_in * rstd_in + (1.0 - r) * mean_ln * rstd_ln));
    }
}

// ---------------------------------------------------------------------------------------------- statistics of a written plane
// biased InstanceNorm statistics of the plane `y` that this workgroup has just written with the same lane-to-element map
__device__ __forceinline__ void plane_instnorm_stats(const float* y, int hw, double sum, double* lds, float* mean_out, float* rstd_out) {
    const double mean = block_sum(sum, lds) / hw;
    double m2 = 0.0;
    for (int i = threadIdx.x; i < hw; i += blockDim.x) {
        const double d = (double)y[i] - mean;
        m2 += d * d;
    }
    m2 = block_sum(m2, lds);
    if (threadIdx.x == 0) {
        mean_out[blockIdx.x] = (float)mean;
        rstd_out[blockIdx.x] = (float)(1.0 / sqrt(m2 / hw + (double)IN_EPS));
    }
}

// ---------------------------------------------------------------------------------------------- aps_affine_apply
__global__ __launch_bounds__(1024) void affine_apply_kernel(const float* __restrict__ x, const float* __restrict__ a,
                                                            const float* __restrict__ b, int act, const float* __restrict__ residual,
                                                            int hw, float* y, float* __restrict__ mean_out, float* __restrict__ rstd_out) {
    __shared__ double lds[MAX_WAVES];
    const size_t off = (size_t)blockIdx.x * hw;
    const float av = a[blockIdx.x], bv = b[blockIdx.x];
    double s = 0.0;
    for (int i = threadIdx.x; i < hw; i += blockDim.x) {
        float v = fmaf(av, x[off + i], bv);
        if (act == APS_ACT_RELU) v = fmaxf(v, 0.f);
        if (residual) v += residual[off + i];
        y[off + i] = v;
        s += (double)v;
    }
    if (mean_out) plane_instnorm_stats(y + off, hw, s, lds, mean_out, rstd_out);
}

// ---------------------------------------------------------------------------------------------- aps_plane_combine
struct CombineParams {
    const float *s0, *s1, *s2, *s3;
    int mode, C, H, W, OH, OW, relu;
    float *y, *mean_out, *rstd_out;
};

__global__ __launch_bounds__(1024) void plane_combine_kernel(const CombineParams p) {
    __shared__ double lds[MAX_WAVES];
    const int plane = blockIdx.x, ohw = p.OH * p.OW, hw = p.H * p.W;
    const size_t in_off = (size_t)plane * hw, out_off = (size_t)plane * ohw;
    double s = 0.0;
    if (p.mode == APS_STAT) {
        for (int i = threadIdx.x; i < hw; i += blockDim.x) {
            const float v = p.s0[in_off + i];
            s += (double)(p.relu ? fmaxf(v, 0.f) : v);
        }
        s = block_sum(s, lds);
        if (threadIdx.x == 0) p.mean_out[plane] = (float)(s / hw);
        return;
    }
    if (p.mode == APS_JOIN) {
        // output channel c of sample n comes from the part that holds it: widths C/2, C/4, C/4
        const int n = plane / p.C, c = plane - n * p.C, h = p.C / 2, q = p.C / 4;
        const float* part = c < h ? p.s1 + ((size_t)n * h + c) * hw
                                  : (c < h + q ? p.s2 + ((size_t)n * q + (c - h)) * hw : p.s3 + ((size_t)n * q + (c - h - q)) * hw);
        for (int i = threadIdx.x; i < hw; i += blockDim.x) {
            const float v = p.s0[in_off + i] + part[i];
            p.y[out_off + i] = v;
            s += (double)v;
        }
    } else if (p.mode == APS_POOL2) {
        for (int i = threadIdx.x; i < ohw; i += blockDim.x) {
            const int oy = i / p.OW, ox = i - oy * p.OW;
            const float* r0 = p.s0 + in_off + (size_t)(2 * oy) * p.W + 2 * ox;
            const float v = (r0[0] + r0[1] + r0[p.W] + r0[p.W + 1]) * 0.25f;
            p.y[out_off + i] = v;
            s += (double)v;
        }
    } else if (p.mode == APS_UP2ADD) {
        for (int i = threadIdx.x; i < ohw; i += blockDim.x) {
            const int oy = i / p.OW, ox = i - oy * p.OW;
            float v = p.s0[in_off + (size_t)(oy >> 1) * p.W + (ox >> 1)];
            if (p.s1) v = p.s1[out_off + i] + v;
            p.y[out_off + i] = v;
            s += (double)v;
        }
    } else {  // APS_SUM3
        for (int i = threadIdx.x; i < hw; i += blockDim.x) {
            const float v = p.s0[in_off + i] + p.s1[in_off + i] + p.s2[in_off + i];
            p.y[out_off + i] = v;
            s += (double)v;
        }
    }
    if (p.mean_out) plane_instnorm_stats(p.y + out_off, ohw, s, lds, p.mean_out, p.rstd_out);
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

int32_t aps_abi_version(void) { return APS_ABI_VERSION; }
const char* aps_last_error(void) { return aps::err_buf(); }

int32_t aps_lin_coeffs_ok(const float* x, const float* rho, const float* gamma, const float* beta, const float* planes, const float* a,
                          const float* b, int32_t N, int32_t C, int32_t H, int32_t W, int32_t per_sample) {
    PlanePlan pl;
    return aps::plan_lin_coeffs(x, rho, gamma, beta, planes, a, b, N, C, H, W, per_sample, &pl) == APS_OK ? 1 : 0;
}

int aps_lin_coeffs(const float* x, int32_t N, int32_t C, int32_t H, int32_t W, const float* rho, const float* gamma, const float* beta,
                   int32_t per_sample, float eps, float* planes, float* a, float* b, void* stream) {
    PlanePlan pl;
    const int rc = aps::plan_lin_coeffs(x, rho, gamma, beta, planes, a, b, N, C, H, W, per_sample, &pl);
    if (rc != APS_OK) return rc;
    if (!(eps >= 0.f)) return fail(APS_ERR_INVALID, "lin_coeffs: eps must be >= 0");
    (void)hipGetLastError();
    hipLaunchKernelGGL(plane_moments_kernel, dim3(pl.planes), dim3(pl.threads), 0, (hipStream_t)stream, x, H * W, planes);
    hipLaunchKernelGGL(lin_fold_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, (const float*)planes, rho, gamma, beta, C, H * W,
                       per_sample, eps, a, b);
    return launched("lin_coeffs");
}

int32_t aps_affine_apply_ok(const float* x, const float* a, const float* b, const float* y, const float* mean_out, const float* rstd_out,
                            int32_t N, int32_t C, int32_t H, int32_t W, int32_t act) {
    PlanePlan pl;
    return aps::plan_affine_apply(x, a, b, y, mean_out, rstd_out, N, C, H, W, act, &pl) == APS_OK ? 1 : 0;
}

int aps_affine_apply(const float* x, const float* a, const float* b, int32_t act, const float* residual, int32_t N, int32_t C, int32_t H,
                     int32_t W, float* y, float* mean_out, float* rstd_out, void* stream) {
    PlanePlan pl;
    const int rc = aps::plan_affine_apply(x, a, b, y, mean_out, rstd_out, N, C, H, W, act, &pl);
    if (rc != APS_OK) return rc;
    (void)hipGetLastError();
    hipLaunchKernelGGL(affine_apply_kernel, dim3(pl.planes), dim3(pl.threads), 0, (hipStream_t)stream, x, a, b, act, residual, H * W, y,
                       mean_out, rstd_out);
    return launched("affine_apply");
}

int32_t aps_plane_combine_ok(int32_t mode, const float* s0, const float* s1, const float* s2, const float* s3, int32_t N, int32_t C,
                             int32_t H, int32_t W, int32_t Hs, int32_t Ws, int32_t flags, const float* y, const float* mean_out,
                             const float* rstd_out) {
    PlanePlan pl;
    return aps::plan_plane_combine(mode, s0, s1, s2, s3, N, C, H, W, Hs, Ws, flags, y, mean_out, rstd_out, &pl) == APS_OK ? 1 : 0;
}

int aps_plane_combine(int32_t mode, const float* s0, const float* s1, const float* s2, const float* s3, int32_t N, int32_t C, int32_t H,
                      int32_t W, int32_t Hs, int32_t Ws, int32_t flags, float* y, float* mean_out, float* rstd_out, void* stream) {
    PlanePlan pl;
    const int rc = aps::plan_plane_combine(mode, s0, s1, s2, s3, N, C, H, W, Hs, Ws, flags, y, mean_out, rstd_out, &pl);
    if (rc != APS_OK) return rc;
    CombineParams p;
    p.s0 = s0; p.s1 = s1; p.s2 = s2; p.s3 = s3;
    p.mode = mode; p.C = C; p.H = H; p.W = W; p.OH = pl.OH; p.OW = pl.OW; p.relu = flags & APS_STAT_RELU;
    p.y = y; p.mean_out = mean_out; p.rstd_out = rstd_out;
    (void)hipGetLastError();
    hipLaunchKernelGGL(plane_combine_kernel, dim3(pl.planes), dim3(pl.threads), 0, (hipStream_t)stream, p);
    return launched("plane_combine");
}

}  // extern "C"
