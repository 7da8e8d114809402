// bwd_stream.h -- what the HBM-bound kernels of the backward pass (instnorm_bwd.hip, instnorm_bwd_split.hip, act_bwd.hip) share:
// the readers of a gradient that is still in the PADDED coordinates of a reflection-padded convolution (the fold of
// nn.ReflectionPad2d's backward is done while reading), the activation derivatives, the block sum, the host's argument checks.
#pragma once
#include "common.h"

namespace apamd {

// gradient read with optional reflection fold: g has spatial (H+2p) x (W+2p)
struct FoldReader {
    const float* g;   // plane base
    int H, W, p, Wp;
    __device__ __forceinline__ float at(int y, int x) const {
        if (p == 0) return g[y * W + x];
        int ys[3], xs[3], ny = 0, nx = 0;
        ys[ny++] = y + p;
        if (y >= 1 && y <= p) ys[ny++] = p - y;
        if (y >= H - 1 - p && y <= H - 2) ys[ny++] = 2 * (H - 1) - y + p;
        xs[nx++] = x + p;
        if (x >= 1 && x <= p) xs[nx++] = p - x;
        if (x >= W - 1 - p && x <= W - 2) xs[nx++] = 2 * (W - 1) - x + p;
        float s = 0.f;
        for (int i = 0; i < ny; ++i)
            for (int j = 0; j < nx; ++j) s += g[ys[i] * Wp + xs[j]];
        return s;
    }
};

// Four consecutive pixels (x4 .. x4 + 3, x4 % 4 == 0, W % 4 == 0, H >= 3) of the fold of a pad-1 reflection-padded
// gradient plane gp[(H + 2) x (W + 2)]: one 16-byte load of the padded row (4-byte aligned: the hardware takes it)
// plus, on the first / last group of a row and on rows 1 and H - 2, the reflected border terms.
typedef float float4u __attribute__((ext_vector_type(4), aligned(4)));

__device__ __forceinline__ float4 fold1_row4(const float* __restrict__ gp, int W, int py, int x4) {
    const float* rp = gp + py * (W + 2);
    const float4u t = *reinterpret_cast<const float4u*>(rp + x4 + 1);
    float4 v = make_float4(t.x, t.y, t.z, t.w);
    if (x4 == 0) v.y += rp[0];                       // padded column 0 is the reflection of column 1
    if (x4 == W - 4) v.z += rp[W + 1];               // padded column W + 1 is the reflection of column W - 2
    return v;
}

// ... on bf16 gradients (2-byte elements, any 2-byte alignment: the padded rows start at odd elements)
__device__ __forceinline__ float bf16_val(unsigned short h) { return __uint_as_float((unsigned)h << 16); }
// four bf16 at an 8-byte-aligned address: one 8-byte load
__device__ __forceinline__ float4 ld4_bf16(const unsigned short* __restrict__ q) {
    const uint2 t = *reinterpret_cast<const uint2*>(q);
    return make_float4(__uint_as_float(t.x << 16), __uint_as_float(t.x & 0xffff0000u), __uint_as_float(t.y << 16), __uint_as_float(t.y & 0xffff0000u));
}
// four bf16 at an ODD element offset of a 4-byte-aligned row (the interior of a pad-1 row: element x + 1, x % 4 == 0, even row
// pitch): ONE 12-byte load of the three dwords around them -- q[-1] and q[4] lie inside the same padded row.  (As four 2-byte
// loads -- what a 2-byte-aligned vector type compiles to -- this read made instnorm_bwd_split<.., G16> half as fast as its
// fp32 form: 110-117 us against 56 for half the bytes.)
__device__ __forceinline__ float4 ld4_bf16_odd(const unsigned short* __restrict__ q) {
    typedef unsigned u32x3 __attribute__((ext_vector_type(3), aligned(4)));
    const u32x3 t = *reinterpret_cast<const u32x3*>(q - 1);
    return make_float4(__uint_as_float(t.x & 0xffff0000u), __uint_as_float(t.y << 16), __uint_as_float(t.y & 0xffff0000u), __uint_as_float(t.z << 16));
}
__device__ __forceinline__ float4 fold1_row4_bf16(const unsigned short* __restrict__ gp, int W, int py, int x4) {
    const unsigned short* rp = gp + py * (W + 2);
    float4 v = ld4_bf16_odd(rp + x4 + 1);
    if (x4 == 0) v.y += bf16_val(rp[0]);
    if (x4 == W - 4) v.z += bf16_val(rp[W + 1]);
    return v;
}

__device__ __forceinline__ float4 fold1_at4(const float* __restrict__ gp, int H, int W, int y, int x4) {
    float4 a = fold1_row4(gp, W, y + 1, x4);
    if (y == 1) { const float4 t = fold1_row4(gp, W, 0, x4); a.x += t.x; a.y += t.y; a.z += t.z; a.w += t.w; }
    if (y == H - 2) { const float4 t = fold1_row4(gp, W, H + 1, x4); a.x += t.x; a.y += t.y; a.z += t.z; a.w += t.w; }
    return a;
}

// The same for pad p = 2, 3 (the 7x7 layers: p = 3) with W % 4 == 0, W >= 4 + 2 p, H >= 2 p + 2: only the first and the last
// group of a row have reflected column partners (pixel x in [1, p] <- padded column p - x; x in [W - 1 - p, W - 2] <- padded
// column 2 (W - 1) - x + p), and only rows [1, p] / [H - 1 - p, H - 2] a partner row: no per-pixel loops (FoldReader::at walks
// up to 3 x 3 taps per pixel with data-dependent trip counts -- one memory round trip each).
__device__ __forceinline__ float4 foldp_row4(const float* __restrict__ gp, int W, int p, int py, int x4) {
    const float* rp = gp + py * (W + 2 * p);
    const float4u t = *reinterpret_cast<const float4u*>(rp + x4 + p);
    float4 v = make_float4(t.x, t.y, t.z, t.w);
    if (x4 == 0) {                                   // pixels 1 .. 3 <- padded columns p - 1, p - 2, p - 3
        v.y += rp[p - 1];
        if (p >= 2) v.z += rp[p - 2];
        if (p >= 3) v.w += rp[p - 3];
    }
    if (x4 == W - 4) {                               // pixels W - 4 .. W - 2 <- padded columns W + p + 2, W + p + 1, W + p
        v.z += rp[W + p];
        if (p >= 2) v.y += rp[W + p + 1];
        if (p >= 3) v.x += rp[W + p + 2];
    }
    return v;
}

__device__ __forceinline__ float4 foldp_at4(const float* __restrict__ gp, int H, int W, int p, int y, int x4) {
    float4 a = foldp_row4(gp, W, p, y + p, x4);
    int py2 = -1;
    if (y >= 1 && y <= p) py2 = p - y;
    else if (y >= H - 1 - p && y <= H - 2) py2 = 2 * (H - 1) - y + p;
    if (py2 >= 0) { const float4 t = foldp_row4(gp, W, p, py2, x4); a.x += t.x; a.y += t.y; a.z += t.z; a.w += t.w; }
    return a;
}

__device__ __forceinline__ float act_grad_from_xhat(float xh, int act) {
    if (act == 1) return xh > 0.f ? 1.f : 0.f;
    if (act == 2) return xh > 0.f ? 1.f : 0.2f;
    return 1.f;
}

// tanh'(pre) = 1 - out^2 as ONE fused operation, spelled out.  Left to the compiler's contraction, the 16-byte path of
// act_bwd_kernel<true> came out as multiply + subtract and every other form as a fused multiply-add, so ap_act_bwd_bias and
// ap_act_bwd disagreed in the last bit of dy on the generator's tanh layer.
__device__ __forceinline__ float tanh_grad(float o) { return __builtin_fmaf(-o, o, 1.f); }

__device__ __forceinline__ float block_sum(float v, float* red) {
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) v += __shfl_xor(v, sh, 64);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    float s = 0.f;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) s += red[i];
    __syncthreads();
    return s;
}

// (the bf16 stores of instnorm_bwd_split_kernel and of instnorm_bwd_fused_big_kernel<.., OB16>)
__device__ __forceinline__ unsigned pack_bf16x2(float a, float b) {
    const __bf16 ha = (__bf16)a, hb = (__bf16)b;
    return (unsigned)__builtin_bit_cast(unsigned short, ha) | ((unsigned)__builtin_bit_cast(unsigned short, hb) << 16);
}

inline int fold_pad_ok(int p1, int H, int W, const char* who) {
    if (p1 < 0 || (p1 > 0 && (p1 >= H || p1 >= W))) return fail(AP_ERR_INVALID, "%s: fold pad %d vs %dx%d", who, p1, H, W);
    return AP_OK;
}

inline int fold_args_ok(const float* g1, int p1, int H, int W, const char* who) {
    if (!g1) return fail(AP_ERR_INVALID, "%s: null gradient", who);
    return fold_pad_ok(p1, H, W, who);
}

// Workgroups per plane of the grid-stride sweeps (instnorm_bwd_apply_kernel, act_bwd_kernel): one per 1024 elements, at most 32.
// act_bwd_kernel<true> leaves one partial sum per workgroup, so ap_act_bwd_bias_workspace_floats sizes its answer by the same call.
inline int sweep_blocks(int H, int W) { return std::min((H * W + 1023) / 1024, 32); }

}  // namespace apamd
