// seq_post.hip -- the clip-level post-processing of Module1's landmark sequence (include/animateportrait_seq.h:
// apq_savgol, apq_calib_baseline, apq_segment_assemble, apq_image_landmarks), so that the sequence stays on the device between
// the two landmark networks and the frame loop.  The reference does this work in numpy / scipy on the host
// (train_audio2landmark.py:101-141, 235-309, 594-617; util/utils.py:361-393; main_end2end_module2.py:262-272).
//
// The tensors are tiny (T <= 625 frames x 204 coordinates), so every kernel here is bound by launch and memory latency, not by
// bandwidth: each is one plain launch with a thread per output element wherever the operation allows it, no atomics, no
// workspace, no traffic between workgroups.  The one true recurrence, the inverted-lip fix, needs the frame before only for
// ten coordinates and only through runs of inverted frames: the sign tests and the inner-lip averaging of all frames run in
// parallel, and ten lanes of one wave then walk the frames with the mouth's columns staged in LDS.
//
// The numpy statements are restated in fp32 in their own operation order; nothing may be fused behind their back.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "seq_post_checks.h"

namespace {

constexpr int LMC = APQ_LM_C;
constexpr int NT = apq::kPostThreads;
constexpr int LIP0 = apq::kLipPoint0 * 3;            // first mouth column (144)
constexpr int LIPC = apq::kLipCols;
constexpr int LS = apq::kLipStride;

int launched(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(apq::err_buf(), 256, "%s: launch failed: %s", what, hipGetErrorString(e));
        return APQ_ERR_LAUNCH;
    }
    return APQ_OK;
}

// ------------------------------------------------------------------------------------------------------------ Savitzky-Golay
struct SgParams {
    const float *x, *taps0, *taps1;
    float* y;
    int T, C, c0, c1, c2, W0, W1;
};

// grid: (T, ceil((c2 - c0) / 256)) workgroups of 256 threads: a workgroup is one output row, so the taps' row is uniform
__global__ __launch_bounds__(256) void savgol_kernel(const SgParams p) {
    const int t = blockIdx.x;
    const int col = p.c0 + blockIdx.y * 256 + threadIdx.x;
    if (col >= p.c2) return;
    const bool first = col < p.c1;
    const int W = first ? p.W0 : p.W1, h = W >> 1;
    const float* taps = first ? p.taps0 : p.taps1;
    int row, start, step;
    if (t < h) {                       // the leading edge: the cubic through the first W samples, evaluated at t
        row = t; start = 0; step = 1;
    } else if (t >= p.T - h) {         // the trailing edge: the same rows, walked backwards from the last sample
        row = p.T - 1 - t; start = p.T - 1; step = -1;
    } else {
        row = h; start = t - h; step = 1;
    }
    const float* tp = taps + row * W;
    const float* xp = p.x + (long long)start * p.C + col;
    const long long stride = (long long)step * p.C;
    float acc = 0.f;
    for (int j = 0; j < W; ++j) acc = fmaf(tp[j], xp[j * stride], acc);
    p.y[(long long)t * p.C + col] = acc;
}

// ------------------------------------------------------------------------------------------------------------ calib_baseline
// grid: 204 workgroups (one column each) of 256 threads; a thread ranks two of the column's values by counting
__global__ __launch_bounds__(256) void calib_kernel(const float* __restrict__ x, float* __restrict__ y, int T, int k, float amp_x, float amp_y) {
    __shared__ float4 v4[APQ_SEG_MAX_T / 4];
    __shared__ double part[4];
    float* const v = reinterpret_cast<float*>(v4);
    const int c = blockIdx.x, tid = threadIdx.x;
    for (int i = tid; i < APQ_SEG_MAX_T; i += 256) v[i] = i < T ? x[i * LMC + c] : INFINITY;    // (the pad ranks behind everything)
    __syncthreads();
    const int i0 = tid, i1 = tid + 256;
    const float a0 = v[i0], a1 = v[i1];
    // rank = how many values come before this one in the order (value, index): a permutation of 0 .. T - 1 whatever the ties
    int r0 = 0, r1 = 0;
    for (int q = 0; q < (T + 3) / 4; ++q) {
        const float4 b4 = v4[q];
        const float b[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = 4 * q + e;
            r0 += (b[e] < a0 || (b[e] == a0 && j < i0)) ? 1 : 0;
            r1 += (b[e] < a1 || (b[e] == a1 && j < i1)) ? 1 : 0;
        }
    }
    double s = 0.0;
    if (i0 < T && r0 < k) s += (double)a0;
    if (i1 < T && r1 < k) s += (double)a1;
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
    if ((tid & 63) == 0) part[tid >> 6] = s;
    __syncthreads();
    const float mean = (float)((((part[0] + part[1]) + part[2]) + part[3]) / (double)k);
    const float amp = c < LIP0 ? 1.f : (c % 3 == 0 ? amp_x : (c % 3 == 1 ? amp_y : 1.f));
    if (i0 < T) y[i0 * LMC + c] = (a0 - mean) * amp;
    if (i1 < T) y[i1 * LMC + c] = (a1 - mean) * amp;
}

// ---------------------------------------------------------------------------------------------------------- segment assembly
struct SegParams {
    const float *in, *base, *fid;
    float* out;
    int T, flags;
    float r, q, amp;        // ratio and 1 - ratio (taken in double, then rounded: numpy's weak Python scalars), amp_pos
};

__device__ __forceinline__ float seg_value(const SegParams& p, int t, int c) {
    float v = p.in[t * LMC + c];
    if (p.flags & APQ_SEG_CLOSE) {
        v = v * p.amp;
        if (p.base) v = (v + p.base[t * LMC + c]) + p.fid[c];
    }
    return v;
}

// grid: 1 + ceil(144 T / 512) workgroups of 512 threads; dynamic LDS: T (61 floats + 1 flag).  Workgroup 0 owns the mouth
// (points 48 .. 67) of every frame, the others the 144 coordinates in front of it, an element per thread.
__global__ __launch_bounds__(NT) void segment_kernel(const SegParams p) {
    extern __shared__ float4 lds4[];
    const int tid = threadIdx.x, T = p.T;
    if (blockIdx.x > 0) {
        const int e = (blockIdx.x - 1) * NT + tid;
        if (e >= T * LIP0) return;
        const int t = e / LIP0, c = e - t * LIP0;
        float v;
        if ((p.flags & APQ_SEG_NOSE) && c >= 27 * 3 && c < 28 * 3) v = seg_value(p, t, c + 3) * 2.f - seg_value(p, t, c + 6);
        else v = seg_value(p, t, c);
        p.out[t * LMC + c] = v;
        return;
    }
    float* const L = reinterpret_cast<float*>(lds4);            // [T][LS]: the mouth's 60 coordinates of every frame
    int* const inverted = reinterpret_cast<int*>(L + T * LS);   // [T]
    auto at = [&](int t, int point, int comp) -> float& { return L[t * LS + (point - apq::kLipPoint0) * 3 + comp]; };

    for (int e = tid; e < T * LIPC; e += NT) {
        const int t = e / LIPC, c = e - t * LIPC;
        L[t * LS + c] = p.in[t * LMC + LIP0 + c];
    }
    __syncthreads();
    if (p.flags & APQ_SEG_CLOSE) {
        if (tid < T) {                                          // close_pose_branch_mouth on frame tid
#pragma unroll
            for (int i = 0; i < 5; ++i)
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    float &a = at(tid, 49 + i, k), &b = at(tid, 59 - i, k);
                    const float fa = a, fb = b, m = 0.5f * fa + 0.5f * fb;
                    a = m * p.r + fa * p.q;
                    b = m * p.r + fb * p.q;
                }
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    float &a = at(tid, 61 + i, k), &b = at(tid, 67 - i, k);
                    const float fa = a, fb = b, m = 0.5f * (fa + fb);
                    a = m * p.r + fa * p.q;
                    b = m * p.r + fb * p.q;
                }
        }
        __syncthreads();
        for (int e = tid; e < T * LIPC; e += NT) {
            const int t = e / LIPC, c = e - t * LIPC;
            float v = L[t * LS + c] * p.amp;
            if (p.base) v = (v + p.base[t * LMC + LIP0 + c]) + p.fid[LIP0 + c];
            L[t * LS + c] = v;
        }
        __syncthreads();
    }
    if (p.flags & APQ_SEG_LIP) {
        // a frame's sign test reads the frame as assembled: no earlier frame has written into it
        if (tid < T) {
            const float x0 = at(tid, 60, 0), y0 = at(tid, 60, 1);
            float sum = 0.f;
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                const float abx = at(tid, 61 + i, 0) - x0, aby = at(tid, 61 + i, 1) - y0;
                const float acx = at(tid, 62 + i, 0) - x0, acy = at(tid, 62 + i, 1) - y0;
                sum += abx * acy - aby * acx;
            }
            const int inv = 0.5f * sum < 0.f ? 1 : 0;
            if (inv) {
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        float &a = at(tid, 63 - i, k), &b = at(tid, 65 + i, k);
                        b = 0.5f * (a + b);
                        a = b;
                    }
            }
            inverted[tid] = inv;
        }
        __syncthreads();
        // the scan: y of the outer lip follows the inner lip's move since the frame before, which is final by then.  A lane
        // owns one (dst, src) column pair of the three slices (55..58 <- 64..67, 59 <- 60, 49..53 <- 60..64).
        if (tid < 10) {
            const int dst = tid < 4 ? 55 + tid : (tid == 4 ? 59 : 49 + (tid - 5));
            const int src = tid < 4 ? 64 + tid : (tid == 4 ? 60 : 60 + (tid - 5));
            float prev_d = at(0, dst, 1), prev_s = at(0, src, 1);          // frame 0 refers to itself
            for (int j = 0; j < T; ++j) {
                float d = at(j, dst, 1);
                const float s = at(j, src, 1);
                if (inverted[j]) {
                    d = s + prev_d - prev_s;
                    at(j, dst, 1) = d;
                }
                prev_d = d;
                prev_s = s;
            }
        }
        __syncthreads();
    }
    for (int e = tid; e < T * LIPC; e += NT) {
        const int t = e / LIPC, c = e - t * LIPC;
        p.out[t * LMC + LIP0 + c] = L[t * LS + c];
    }
}

// ----------------------------------------------------------------------------------------------------------- image landmarks
struct ImgParams {
    const float* in;
    float* out;
    const int32_t* stamps;
    int n_stamps, T, flags;
    double scale, shift_x, shift_y;
};

__device__ __forceinline__ float img_value(const ImgParams& p, int t, int c) {
    const float v = p.in[(long long)t * LMC + c];
    const int comp = c % 3;
    if (!(p.flags & APQ_IMG_TRANSFORM) || comp == 2) return v;
    return (float)(-(double)v / p.scale - (comp == 0 ? p.shift_x : p.shift_y));
}

// the lid mix of add_naive_eye at (frame, upper-lid point a, lower-lid point b): the pair's new values
__device__ __forceinline__ void lid_mix(const ImgParams& p, int t, int a, int b, int comp, float& na, float& nb) {
    const float fa = img_value(p, t, a * 3 + comp), fb = img_value(p, t, b * 3 + comp);
    na = 0.95f * fa + 0.05f * fb;
    nb = 0.05f * fa + 0.95f * fb;
}

// grid: ceil(204 T / 256) workgroups of 256 threads, an element per thread.  A blink touches the frames t - 9 .. t + 14 and
// reads t - 10, t and t + 15, which no blink writes: every element is a function of the input alone.
__global__ __launch_bounds__(256) void image_kernel(const ImgParams p) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)p.T * LMC) return;
    const int f = (int)(e / LMC), c = (int)(e - (long long)f * LMC);
    const int point = c / 3, comp = c - point * 3;
    int a = -1, b = -1;
    if (p.flags & APQ_IMG_EYES) {
        switch (point) {
            case 37: case 41: a = 37; b = 41; break;
            case 38: case 40: a = 38; b = 40; break;
            case 43: case 47: a = 43; b = 47; break;
            case 44: case 46: a = 44; b = 46; break;
            default: break;
        }
    }
    if (a < 0) {
        p.out[e] = img_value(p, f, c);
        return;
    }
    const bool upper = point == a;
    auto mixed = [&](int t) {
        float na, nb;
        lid_mix(p, min(max(t, 0), p.T - 1), a, b, comp, na, nb);
        return upper ? na : nb;
    };
    auto closed = [&](int t) {
        float na, nb;
        lid_mix(p, min(max(t, 0), p.T - 1), a, b, comp, na, nb);
        return 0.25f * na + 0.75f * nb;
    };
    float v = mixed(f);
    for (int n = 0; n < p.n_stamps; ++n) {
        const int t = p.stamps[n];
        if (f < t - 9 || f > t + 14) continue;
        if (f == t) {
            v = closed(t);
        } else if (f < t) {
            const float w = (float)(t - f) / 10.f;
            v = w * mixed(t - 10) + (1.f - w) * closed(t);
        } else {
            const float w = (float)(t + 14 - f) / 15.f;
            v = w * closed(t) + (1.f - w) * mixed(t + 15);
        }
        break;
    }
    p.out[e] = v;
}

}  // namespace

extern "C" {

int32_t apq_savgol_ok(const float* x, const float* y, const float* taps0, const float* taps1, int32_t T, int32_t C, int32_t c0,
                      int32_t c1, int32_t c2, int32_t W0, int32_t W1) {
    return apq::check_savgol(x, y, taps0, taps1, T, C, c0, c1, c2, W0, W1) == APQ_OK ? 1 : 0;
}

int apq_savgol(const float* x, float* y, const float* taps0, const float* taps1, int32_t T, int32_t C, int32_t c0, int32_t c1,
               int32_t c2, int32_t W0, int32_t W1, void* stream) {
    const int rc = apq::check_savgol(x, y, taps0, taps1, T, C, c0, c1, c2, W0, W1);
    if (rc != APQ_OK) return rc;
    if (c2 == c0) return APQ_OK;                     // nothing to filter
    SgParams p;
    p.x = x; p.y = y; p.taps0 = taps0; p.taps1 = taps1;
    p.T = T; p.C = C; p.c0 = c0; p.c1 = c1; p.c2 = c2; p.W0 = W0; p.W1 = W1;
    (void)hipGetLastError();
    hipLaunchKernelGGL(savgol_kernel, dim3(T, (c2 - c0 + 255) / 256), dim3(256), 0, (hipStream_t)stream, p);
    return launched("savgol");
}

int32_t apq_calib_baseline_ok(const float* x, const float* y, int32_t T, int32_t k, float amp_x, float amp_y) {
    (void)amp_x; (void)amp_y;
    return apq::check_calib_baseline(x, y, T, k) == APQ_OK ? 1 : 0;
}

int apq_calib_baseline(const float* x, float* y, int32_t T, int32_t k, float amp_x, float amp_y, void* stream) {
    const int rc = apq::check_calib_baseline(x, y, T, k);
    if (rc != APQ_OK) return rc;
    (void)hipGetLastError();
    hipLaunchKernelGGL(calib_kernel, dim3(LMC), dim3(256), 0, (hipStream_t)stream, x, y, T, k, amp_x, amp_y);
    return launched("calib_baseline");
}

int32_t apq_segment_assemble_ok(const float* in, const float* base, const float* fid, const float* out, int32_t T, double ratio,
                                float amp, int32_t flags) {
    (void)ratio; (void)amp;
    return apq::check_segment_assemble(in, base, fid, out, T, flags) == APQ_OK ? 1 : 0;
}

int apq_segment_assemble(const float* in, const float* base, const float* fid, float* out, int32_t T, double ratio, float amp,
                         int32_t flags, void* stream) {
    const int rc = apq::check_segment_assemble(in, base, fid, out, T, flags);
    if (rc != APQ_OK) return rc;
    // the longest segment's mouth needs more than the 64 KiB a kernel gets without asking
    constexpr int kMaxLds = APQ_SEG_MAX_T * (LS + 1) * (int)sizeof(float);
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&segment_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds);
    if (e != hipSuccess) {
        snprintf(apq::err_buf(), 256, "segment_assemble: hipFuncSetAttribute: %s", hipGetErrorString(e));
        return APQ_ERR_LAUNCH;
    }
    SegParams p;
    p.in = in; p.base = base; p.fid = fid; p.out = out; p.T = T; p.flags = flags;
    p.r = (float)ratio; p.q = (float)(1.0 - ratio); p.amp = amp;
    const size_t lds = ((size_t)T * (LS + 1) * sizeof(float) + 15) / 16 * 16;
    (void)hipGetLastError();
    hipLaunchKernelGGL(segment_kernel, dim3(1 + (T * LIP0 + NT - 1) / NT), dim3(NT), lds, (hipStream_t)stream, p);
    return launched("segment_assemble");
}

int32_t apq_image_landmarks_ok(const float* in, const float* out, const int32_t* stamps, int32_t n_stamps, int32_t T, double scale,
                               double shift_x, double shift_y, int32_t flags) {
    (void)shift_x; (void)shift_y;
    return apq::check_image_landmarks(in, out, stamps, n_stamps, T, scale, flags) == APQ_OK ? 1 : 0;
}

int apq_image_landmarks(const float* in, float* out, const int32_t* stamps, int32_t n_stamps, int32_t T, double scale, double shift_x,
                        double shift_y, int32_t flags, void* stream) {
    const int rc = apq::check_image_landmarks(in, out, stamps, n_stamps, T, scale, flags);
    if (rc != APQ_OK) return rc;
    ImgParams p;
    p.in = in; p.out = out; p.stamps = stamps; p.n_stamps = (flags & APQ_IMG_EYES) ? n_stamps : 0; p.T = T; p.flags = flags;
    p.scale = scale; p.shift_x = shift_x; p.shift_y = shift_y;
    (void)hipGetLastError();
    hipLaunchKernelGGL(image_kernel, dim3((unsigned)(((long long)T * LMC + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
    return launched("image_landmarks");
}

}  // extern "C"
