// warp_sample.h -- device helpers and constants shared by the feature-warp translation units (warp_fwd.hip, warp_bwd.hip).
// Sampling convention: the gathers are grid_sample with bilinear / zeros / align_corners=False; motion, flow and mask reach
// the feature resolution by align_corners=True bilinear resizes, evaluated per output pixel.
#pragma once
#include "common.h"

namespace apamd {

struct Taps {
    int off[4];     // offset inside a channel plane, or -1 when the tap is out of range (contributes 0)
    float w[4];
};

__device__ __forceinline__ Taps make_taps(float gx, float gy, int H, int W) {
    // grid_sampler_unnormalize, align_corners=False: ((g + 1) * size - 1) / 2
    float ix = ((gx + 1.f) * (float)W - 1.f) / 2.f;
    float iy = ((gy + 1.f) * (float)H - 1.f) / 2.f;
    ix = fminf(fmaxf(ix, -2.f), (float)W + 1.f);   // everything beyond is all-zero taps anyway
    iy = fminf(fmaxf(iy, -2.f), (float)H + 1.f);
    const float fx = floorf(ix), fy = floorf(iy);
    const int x0 = (int)fx, y0 = (int)fy, x1 = x0 + 1, y1 = y0 + 1;
    const float ex = fx + 1.f, ey = fy + 1.f;
    Taps t;
    t.w[0] = (ex - ix) * (ey - iy);   // nw
    t.w[1] = (ix - fx) * (ey - iy);   // ne
    t.w[2] = (ex - ix) * (iy - fy);   // sw
    t.w[3] = (ix - fx) * (iy - fy);   // se
    const bool xin0 = x0 >= 0 && x0 < W, xin1 = x1 >= 0 && x1 < W;
    const bool yin0 = y0 >= 0 && y0 < H, yin1 = y1 >= 0 && y1 < H;
    t.off[0] = (xin0 && yin0) ? y0 * W + x0 : -1;
    t.off[1] = (xin1 && yin0) ? y0 * W + x1 : -1;
    t.off[2] = (xin0 && yin1) ? y1 * W + x0 : -1;
    t.off[3] = (xin1 && yin1) ? y1 * W + x1 : -1;
    return t;
}

struct Lerp { int i0, i1; float l0, l1; };

// F.interpolate(mode='bilinear', align_corners=True): src = dst * (S-1)/(H-1)
__device__ __forceinline__ Lerp make_lerp(int dst, int S, int H) {
    const float scale = H > 1 ? (float)(S - 1) / (float)(H - 1) : 0.f;
    const float src = scale * (float)dst;
    Lerp l;
    l.i0 = (int)src;
    if (l.i0 > S - 1) l.i0 = S - 1;
    l.i1 = l.i0 + (l.i0 < S - 1 ? 1 : 0);
    l.l1 = src - (float)l.i0;
    l.l0 = 1.f - l.l1;
    return l;
}

__device__ __forceinline__ float bilerp(float v00, float v01, float v10, float v11, const Lerp& ly, const Lerp& lx) {
    return ly.l0 * (lx.l0 * v00 + lx.l1 * v01) + ly.l1 * (lx.l0 * v10 + lx.l1 * v11);
}

constexpr int kWarpCG = 8;   // channels per thread = one 16-byte slot of the split-bf16 layout

// launch grid of the warp kernels: `blocks` pixel blocks or tiles, then channel groups of kWarpCG, then images
inline dim3 warp_grid(int blocks, int C, int N) { return dim3(blocks, (C + kWarpCG - 1) / kWarpCG, N); }

}  // namespace apamd
