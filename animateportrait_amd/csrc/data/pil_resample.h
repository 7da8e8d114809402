// Pillow's 8-bit resampler (Resample.c), the part every kernel that restates it shares: 22-bit integer weights, an int32
// accumulator that starts at one half, and a shift-and-clip to uint8 after EACH pass (the uint8 intermediate is part of the
// result).  image_prep.hip reads its weights from the caller's tables; the face library (face/face_resize.hip) computes the
// triangle filter's per output pixel with the functions below, in Pillow's double arithmetic and operation order
// (precompute_coeffs, normalize_coeffs_8bpc) -- compile with -ffp-contract=off.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pil {

constexpr int PRECISION_BITS = 32 - 8 - 2;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ int clip8(int acc) { return clampi(acc >> PRECISION_BITS, 0, 255); }

// the taps of one output index along one axis: source indices [lo, lo + n), weights tap(t) / ww before the integer rounding
struct BilinearAxis {
    double center, ss, ww;
    int lo, n;
};

__device__ __forceinline__ double triangle(double x) {
    if (x < 0.0) x = -x;
    return x < 1.0 ? 1.0 - x : 0.0;
}

__device__ __forceinline__ BilinearAxis bilinear_axis(int in_size, int out_size, int o) {
    BilinearAxis a;
    const double scale = (double)in_size / (double)out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * filterscale;
    a.center = (o + 0.5) * scale;
    a.ss = 1.0 / filterscale;
    int lo = (int)(a.center - support + 0.5);
    if (lo < 0) lo = 0;
    int hi = (int)(a.center + support + 0.5);
    if (hi > in_size) hi = in_size;
    a.lo = lo;
    a.n = hi - lo;
    double ww = 0.0;
    for (int t = 0; t < a.n; ++t) ww += triangle((t + lo - a.center + 0.5) * a.ss);
    a.ww = ww;
    return a;
}

__device__ __forceinline__ int bilinear_weight(const BilinearAxis& a, int t) {
    double w = triangle((t + a.lo - a.center + 0.5) * a.ss);
    if (a.ww != 0.0) w = w / a.ww;
    return w < 0.0 ? (int)(-0.5 + w * (double)(1 << PRECISION_BITS)) : (int)(0.5 + w * (double)(1 << PRECISION_BITS));
}

}  // namespace pil
