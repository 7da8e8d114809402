// Input and output side of the FAN landmark network (include/animateportrait_face.h, fan.py): the crop about a face box resized
// by OpenCV's 8-bit INTER_LINEAR rule (with its mirrored copy), and heat maps -> landmarks (flip sum, argmax, quarter-pixel step,
// inverse transform in float64).  The box arithmetic that fixes a window runs in the launcher (face_checks.h: fan_frame); the
// kernels are integer / comparison work, one thread per output pixel and one workgroup per (image, landmark).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "face_checks.h"

namespace {

using apf::fail;
constexpr int THREADS = 256;

struct CropParams {
    int H, W, ulx, uly, ww, wh, R, flip, order;
};

// OpenCV's linear taps of destination index d: first source index and the two 11-bit weights
__device__ __forceinline__ int linear_axis(int src, int dst, int d, int* w0, int* w1) {
    const double scale = (double)src / (double)dst;
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { s = 0; f = 0.f; }
    if (s >= src - 1) { s = src - 1; f = 0.f; }
    *w0 = (int)rintf((1.f - f) * 2048.f);
    *w1 = (int)rintf(f * 2048.f);
    return s;
}

__global__ __launch_bounds__(THREADS) void fan_crop_kernel(const uint8_t* __restrict__ img, CropParams p, float* __restrict__ out) {
    const int x = blockIdx.x * THREADS + threadIdx.x, y = blockIdx.y;
    if (x >= p.R || y >= p.R) return;
    int a0, a1, b0, b1;
    const int sx = linear_axis(p.ww, p.R, x, &a0, &a1), sy = linear_axis(p.wh, p.R, y, &b0, &b1);
    const int wx[2] = {sx, min(sx + 1, p.ww - 1)}, wy[2] = {sy, min(sy + 1, p.wh - 1)};
    int S[2][3];
    for (int r = 0; r < 2; ++r) {
        const int iy = wy[r] + p.uly;
        int t[2][3];
        for (int k = 0; k < 2; ++k) {
            const int ix = wx[k] + p.ulx;
            const bool inside = iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;           // zero where the window leaves the image
            const uint8_t* px = img + ((size_t)(inside ? iy : 0) * p.W + (inside ? ix : 0)) * 3;
            for (int c = 0; c < 3; ++c) t[k][c] = inside ? (int)px[c] : 0;
        }
        for (int c = 0; c < 3; ++c) S[r][c] = t[0][c] * a0 + t[1][c] * a1;
    }
    const size_t plane = (size_t)p.R * p.R;
    for (int c = 0; c < 3; ++c) {
        int v = (((b0 * (S[0][c] >> 4)) >> 16) + ((b1 * (S[1][c] >> 4)) >> 16) + 2) >> 2;
        v = v < 0 ? 0 : (v > 255 ? 255 : v);
        const float f = (float)v / 255.0f;
        const int pc = p.order == APF_FAN_BGR ? 2 - c : c;
        out[pc * plane + (size_t)y * p.R + x] = f;
        if (p.flip) out[(3 + pc) * plane + (size_t)y * p.R + (p.R - 1 - x)] = f;
    }
}

struct DecodeParams {
    int B, Hm, truncate;
    apf::FanFrame frame[APF_FAN_MAX_B];
};

// jaw i <-> 16 - i, brows 17 <-> 26 .. 21 <-> 22, nose 31 <-> 35, 32 <-> 34, eyes, mouth; everything else maps to itself
__constant__ int8_t kPair[APF_FAN_POINTS] = {16, 15, 14, 13, 12, 11, 10, 9,  8,  7,  6,  5,  4,  3,  2,  1,  0,  26, 25, 24, 23, 22, 21,
                                             20, 19, 18, 17, 27, 28, 29, 30, 35, 34, 33, 32, 31, 45, 44, 43, 42, 47, 46, 39, 38, 37, 36,
                                             41, 40, 54, 53, 52, 51, 50, 49, 48, 59, 58, 57, 56, 55, 64, 63, 62, 61, 60, 67, 66, 65};

// (value, index): the larger value wins, the lower index on equal values
__device__ __forceinline__ void take_better(float& v, int& i, float ov, int oi) {
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

__global__ __launch_bounds__(THREADS) void fan_decode_kernel(const float* __restrict__ hm, const float* __restrict__ hmf, DecodeParams p,
                                                              float* __restrict__ out) {
    const int j = blockIdx.x, b = blockIdx.y, Hm = p.Hm, n = Hm * Hm;
    const float* m0 = hm + ((size_t)b * APF_FAN_POINTS + j) * n;
    const float* m1 = hmf ? hmf + ((size_t)b * APF_FAN_POINTS + kPair[j]) * n : nullptr;
    auto value = [&](int y, int x) {
        float v = m0[y * Hm + x];
        if (m1) v = v + m1[y * Hm + (Hm - 1 - x)];
        return v;
    };
    float best = -INFINITY;
    int at = 0x7fffffff;
    for (int e = threadIdx.x; e < n; e += THREADS) take_better(best, at, value(e / Hm, e % Hm), e);       // ascending e per thread
    // fixed-order reduction: the wave by halving shuffles, then the four waves through LDS
    for (int off = 32; off >= 1; off >>= 1) {
        const float ov = __shfl_down(best, off, 64);
        const int oi = __shfl_down(at, off, 64);
        take_better(best, at, ov, oi);
    }
    __shared__ float s_v[THREADS / 64];
    __shared__ int s_i[THREADS / 64];
    if ((threadIdx.x & 63) == 0) { s_v[threadIdx.x >> 6] = best; s_i[threadIdx.x >> 6] = at; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < THREADS / 64; ++w) take_better(best, at, s_v[w], s_i[w]);
    if (at == 0x7fffffff) at = 0;                                   // a map of NaNs
    const int px = at % Hm, py = at / Hm;
    float fx = (float)(px + 1), fy = (float)(py + 1);
    if (px > 0 && px < Hm - 1 && py > 0 && py < Hm - 1) {
        const float dx = value(py, px + 1) - value(py, px - 1), dy = value(py + 1, px) - value(py - 1, px);
        fx += dx > 0.f ? 0.25f : (dx < 0.f ? -0.25f : 0.f);
        fy += dy > 0.f ? 0.25f : (dy < 0.f ? -0.25f : 0.f);
    }
    fx -= 0.5f;
    fy -= 0.5f;
    const apf::FanFrame f = p.frame[b];
    double X = f.i00 * (double)fx + f.i02x, Y = f.i00 * (double)fy + f.i02y;
    if (p.truncate) { X = trunc(X); Y = trunc(Y); }
    float* o = out + ((size_t)b * APF_FAN_POINTS + j) * 2;
    o[0] = (float)X;
    o[1] = (float)Y;
}

int launched(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return APF_OK;
    snprintf(apf::err_buf(), 256, "%s: launch failed: %s", what, hipGetErrorString(e));
    return APF_ERR_LAUNCH;
}

}  // namespace

extern "C" {

int32_t apf_fan_crop_ok(const uint8_t* img, int32_t H, int32_t W, double x0, double y0, double x1, double y1, int32_t R, int32_t flip,
                        int32_t order, const float* out) {
    return apf::check_fan_crop(img, H, W, x0, y0, x1, y1, R, flip, order, out) == APF_OK ? 1 : 0;
}

int apf_fan_crop(const uint8_t* img, int32_t H, int32_t W, double x0, double y0, double x1, double y1, int32_t R, int32_t flip,
                 int32_t order, float* out, void* stream) {
    const int rc = apf::check_fan_crop(img, H, W, x0, y0, x1, y1, R, flip, order, out);
    if (rc != APF_OK) return rc;
    const apf::FanWindow win = apf::fan_window(x0, y0, x1, y1, R);
    const CropParams p = {H, W, win.ulx, win.uly, win.w, win.h, R, flip, order};
    (void)hipGetLastError();
    hipLaunchKernelGGL(fan_crop_kernel, dim3((R + THREADS - 1) / THREADS, R), dim3(THREADS), 0, (hipStream_t)stream, img, p, out);
    return launched("fan_crop");
}

int32_t apf_fan_decode_ok(const float* hm, const float* hm_flipped, int32_t B, int32_t Hm, const double* boxes, const float* out) {
    (void)hm_flipped;
    return apf::check_fan_decode(hm, B, Hm, boxes, out) == APF_OK ? 1 : 0;
}

int apf_fan_decode(const float* hm, const float* hm_flipped, int32_t B, int32_t Hm, const double* boxes, int32_t truncate, float* out,
                   void* stream) {
    const int rc = apf::check_fan_decode(hm, B, Hm, boxes, out);
    if (rc != APF_OK) return rc;
    DecodeParams p = {};
    p.B = B;
    p.Hm = Hm;
    p.truncate = truncate != 0;
    for (int b = 0; b < B; ++b) p.frame[b] = apf::fan_frame(boxes[4 * b], boxes[4 * b + 1], boxes[4 * b + 2], boxes[4 * b + 3], Hm);
    (void)hipGetLastError();
    hipLaunchKernelGGL(fan_decode_kernel, dim3(APF_FAN_POINTS, B), dim3(THREADS), 0, (hipStream_t)stream, hm, hm_flipped, p, out);
    return launched("fan_decode");
}

}  // extern "C"
