// instnorm_bwd.hip -- ap_instnorm_bwd: backward of  a = act(IN(y))  w.r.t. y.  The incoming gradient may be (i) the data-gradient
// of a reflection-padded convolution, still in PADDED coordinates, plus (ii) a second plain gradient (residual branch).  One
// workgroup per (n, c) plane where the plane fits its registers (+ LDS), else the reduce / apply pair; instnorm_bwd_route decides.
#include "bwd_stream.h"

namespace apamd {

// grid: (N*C).  sums[nc] = (sum g', sum g' * xhat), g' = (fold(g1) + g2) * act'(xhat)
__global__ __launch_bounds__(256) void instnorm_bwd_reduce_kernel(const float* __restrict__ g1, int p1,
                                                                  const float* __restrict__ g2,
                                                                  const float* __restrict__ y,
                                                                  const float* __restrict__ mean,
                                                                  const float* __restrict__ rstd, int act, int H, int W,
                                                                  float* __restrict__ sums) {
    __shared__ float red[8];
    const int nc = blockIdx.x;
    const int HW = H * W;
    const float m = mean[nc], r = rstd[nc];
    FoldReader fr{g1 + (long long)nc * (H + 2 * p1) * (W + 2 * p1), H, W, p1, W + 2 * p1};
    const float* yp = y + (long long)nc * HW;
    const float* g2p = g2 ? g2 + (long long)nc * HW : nullptr;
    float s1 = 0.f, s2 = 0.f;
    if (p1 == 0 && (HW & 3) == 0) {
        // unfolded gradient: 16-byte lanes (same per-thread summation order is not required: block_sum is a tree)
        const float4* y4 = reinterpret_cast<const float4*>(yp);
        const float4* ga = reinterpret_cast<const float4*>(g1 + (long long)nc * HW);
        const float4* gb = g2p ? reinterpret_cast<const float4*>(g2p) : nullptr;
        for (int i = threadIdx.x; i < HW / 4; i += 256) {
            const float4 yv = y4[i];
            float4 gv = ga[i];
            if (gb) { const float4 t = gb[i]; gv.x += t.x; gv.y += t.y; gv.z += t.z; gv.w += t.w; }
            const float xh0 = (yv.x - m) * r, xh1 = (yv.y - m) * r, xh2 = (yv.z - m) * r, xh3 = (yv.w - m) * r;
            const float a0 = gv.x * act_grad_from_xhat(xh0, act), a1 = gv.y * act_grad_from_xhat(xh1, act);
            const float a2 = gv.z * act_grad_from_xhat(xh2, act), a3 = gv.w * act_grad_from_xhat(xh3, act);
            s1 += (a0 + a1) + (a2 + a3);
            s2 += (a0 * xh0 + a1 * xh1) + (a2 * xh2 + a3 * xh3);
        }
    } else
    for (int i = threadIdx.x; i < HW; i += 256) {
        const int yy = i / W, xx = i - yy * W;
        const float xh = (yp[i] - m) * r;
        float g = fr.at(yy, xx);
        if (g2p) g += g2p[i];
        g *= act_grad_from_xhat(xh, act);
        s1 += g;
        s2 += g * xh;
    }
    s1 = block_sum(s1, red);
    s2 = block_sum(s2, red);
    if (threadIdx.x == 0) {
        sums[nc * 2] = s1;
        sums[nc * 2 + 1] = s2;
    }
}

// grid: (ceil(HW/256/4), N*C).  dy = rstd * (g' - S1/HW - xhat * S2/HW)
__global__ __launch_bounds__(256) void instnorm_bwd_apply_kernel(const float* __restrict__ g1, int p1,
                                                                 const float* __restrict__ g2,
                                                                 const float* __restrict__ y,
                                                                 const float* __restrict__ mean,
                                                                 const float* __restrict__ rstd, int act, int H, int W,
                                                                 const float* __restrict__ sums,
                                                                 float* __restrict__ dy) {
    const int nc = blockIdx.y;
    const int HW = H * W;
    const float m = mean[nc], r = rstd[nc];
    const float inv = 1.f / (float)HW;
    const float a1 = sums[nc * 2] * inv, a2 = sums[nc * 2 + 1] * inv;
    FoldReader fr{g1 + (long long)nc * (H + 2 * p1) * (W + 2 * p1), H, W, p1, W + 2 * p1};
    const float* yp = y + (long long)nc * HW;
    const float* g2p = g2 ? g2 + (long long)nc * HW : nullptr;
    float* out = dy + (long long)nc * HW;
    if (p1 == 0 && (HW & 3) == 0) {
        const float4* y4 = reinterpret_cast<const float4*>(yp);
        const float4* ga = reinterpret_cast<const float4*>(g1 + (long long)nc * HW);
        const float4* gb = g2p ? reinterpret_cast<const float4*>(g2p) : nullptr;
        float4* o4 = reinterpret_cast<float4*>(out);
        for (int i = blockIdx.x * 256 + threadIdx.x; i < HW / 4; i += gridDim.x * 256) {
            const float4 yv = y4[i];
            float4 gv = ga[i];
            if (gb) { const float4 t = gb[i]; gv.x += t.x; gv.y += t.y; gv.z += t.z; gv.w += t.w; }
            float4 o;
            float xh = (yv.x - m) * r; o.x = r * (gv.x * act_grad_from_xhat(xh, act) - a1 - xh * a2);
            xh = (yv.y - m) * r; o.y = r * (gv.y * act_grad_from_xhat(xh, act) - a1 - xh * a2);
            xh = (yv.z - m) * r; o.z = r * (gv.z * act_grad_from_xhat(xh, act) - a1 - xh * a2);
            xh = (yv.w - m) * r; o.w = r * (gv.w * act_grad_from_xhat(xh, act) - a1 - xh * a2);
            o4[i] = o;
        }
        return;
    }
    for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += gridDim.x * 256) {
        const int yy = i / W, xx = i - yy * W;
        const float xh = (yp[i] - m) * r;
        float g = fr.at(yy, xx);
        if (g2p) g += g2p[i];
        g *= act_grad_from_xhat(xh, act);
        out[i] = r * (g - a1 - xh * a2);
    }
}

// One pass for planes that fit the registers of a workgroup (H*W <= NT * EPT): the gradient and the normalised
// activation of one (n, c) plane are loaded once, reduced in the block, and dy is written from the registers --
// 2 reads + 1 write per element instead of the 4 + 1 of the reduce / apply pair.  grid: (N*C)
template <int NT, int EPT>
__global__ __launch_bounds__(NT) void instnorm_bwd_fused_kernel(const float* __restrict__ g1, int p1,
                                                                const float* __restrict__ g2,
                                                                const float* __restrict__ y,
                                                                const float* __restrict__ mean,
                                                                const float* __restrict__ rstd, int act, int H, int W,
                                                                float* __restrict__ dy) {
    __shared__ float red[NT / 64];
    const int nc = blockIdx.x, tid = threadIdx.x;
    const int HW = H * W;
    const float m = mean[nc], r = rstd[nc];
    const float* yp = y + (long long)nc * HW;
    const float* g2p = g2 ? g2 + (long long)nc * HW : nullptr;
    float* out = dy + (long long)nc * HW;
    float gv[EPT], xh[EPT];
    float s1 = 0.f, s2 = 0.f;
    const bool fold1 = p1 == 1 && (W & 3) == 0 && H >= 3;
    const bool vec = (p1 == 0 && (HW & 3) == 0) || fold1;
    if (vec) {
        const float4* y4 = reinterpret_cast<const float4*>(yp);
        const float4* ga = reinterpret_cast<const float4*>(g1 + (long long)nc * HW);
        const float* gp = g1 + (long long)nc * (H + 2) * (W + 2);
        const float4* gb = g2p ? reinterpret_cast<const float4*>(g2p) : nullptr;
        const int W4 = W >> 2;
#pragma unroll
        for (int k = 0; k < EPT / 4; ++k) {
            const int i = k * NT + tid;
            float4 yv = make_float4(m, m, m, m), gq = make_float4(0.f, 0.f, 0.f, 0.f);
            if (i < HW / 4) {
                yv = y4[i];
                if (fold1) { const int yy = i / W4; gq = fold1_at4(gp, H, W, yy, (i - yy * W4) * 4); }
                else gq = ga[i];
                if (gb) { const float4 t = gb[i]; gq.x += t.x; gq.y += t.y; gq.z += t.z; gq.w += t.w; }
            }
            const float yy[4] = {yv.x, yv.y, yv.z, yv.w}, gg[4] = {gq.x, gq.y, gq.z, gq.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float x = (yy[j] - m) * r;
                const float g = gg[j] * act_grad_from_xhat(x, act);
                xh[k * 4 + j] = x;
                gv[k * 4 + j] = g;
                s1 += g;
                s2 += g * x;
            }
        }
    } else {
        FoldReader fr{g1 + (long long)nc * (H + 2 * p1) * (W + 2 * p1), H, W, p1, W + 2 * p1};
#pragma unroll
        for (int k = 0; k < EPT; ++k) {
            const int i = k * NT + tid;
            float x = 0.f, g = 0.f;
            if (i < HW) {
                const int yy = i / W, xx = i - yy * W;
                x = (yp[i] - m) * r;
                g = fr.at(yy, xx);
                if (g2p) g += g2p[i];
                g *= act_grad_from_xhat(x, act);
            }
            xh[k] = x;
            gv[k] = g;
            s1 += g;
            s2 += g * x;
        }
    }
    s1 = block_sum(s1, red);
    s2 = block_sum(s2, red);
    const float inv = 1.f / (float)HW;
    const float a1 = s1 * inv, a2 = s2 * inv;
    if (vec) {
        float4* o4 = reinterpret_cast<float4*>(out);
#pragma unroll
        for (int k = 0; k < EPT / 4; ++k) {
            const int i = k * NT + tid;
            if (i < HW / 4)
                o4[i] = make_float4(r * (gv[k * 4] - a1 - xh[k * 4] * a2), r * (gv[k * 4 + 1] - a1 - xh[k * 4 + 1] * a2),
                                    r * (gv[k * 4 + 2] - a1 - xh[k * 4 + 2] * a2), r * (gv[k * 4 + 3] - a1 - xh[k * 4 + 3] * a2));
        }
    } else {
#pragma unroll
        for (int k = 0; k < EPT; ++k) {
            const int i = k * NT + tid;
            if (i < HW) out[i] = r * (gv[k] - a1 - xh[k] * a2);
        }
    }
}

// The same for an unfolded gradient with H W % 4 == 0 (every launch of the train step that is not on the operand-writing route),
// with the load-phase rule applied (section 3.5 of DESIGN.md): all 16-byte loads of a thread -- y, g1 and, as a template parameter,
// g2 -- are issued from clamped indices before any arithmetic.  (In the general kernel above the `i < HW / 4` test, the fold test and
// the `g2 != nullptr` test sit between the loads: 8-12 dependent round trips per thread, 3.9 TB/s.)
template <int NT, int EPT, bool G2>
__global__ __launch_bounds__(NT) void instnorm_bwd_fused_vec_kernel(const float* __restrict__ g1, const float* __restrict__ g2,
                                                                    const float* __restrict__ y, const float* __restrict__ mean,
                                                                    const float* __restrict__ rstd, int act, int HW,
                                                                    float* __restrict__ dy) {
    __shared__ float red[NT / 64];
    constexpr int NG = EPT / 4;
    const int nc = blockIdx.x, tid = threadIdx.x, Q = HW >> 2;
    const float4* y4 = reinterpret_cast<const float4*>(y + (long long)nc * HW);
    const float4* ga = reinterpret_cast<const float4*>(g1 + (long long)nc * HW);
    const float4* gb = reinterpret_cast<const float4*>((G2 ? g2 : g1) + (long long)nc * HW);
    float4 yv[NG], gq[NG], gr[NG];
#pragma unroll
    for (int k = 0; k < NG; ++k) {
        const int i = k * NT + tid, ic = i < Q ? i : Q - 1;
        yv[k] = y4[ic];
        gq[k] = ga[ic];
        if constexpr (G2) gr[k] = gb[ic];
    }
    const float m = mean[nc], r = rstd[nc];
    float gv[EPT], xh[EPT];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < NG; ++k) {
        const bool in = k * NT + tid < Q;
        const float yy[4] = {yv[k].x, yv[k].y, yv[k].z, yv[k].w};
        float gg[4] = {gq[k].x, gq[k].y, gq[k].z, gq[k].w};
        if constexpr (G2) { gg[0] += gr[k].x; gg[1] += gr[k].y; gg[2] += gr[k].z; gg[3] += gr[k].w; }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float x = in ? (yy[j] - m) * r : 0.f;
            const float g = in ? gg[j] * act_grad_from_xhat(x, act) : 0.f;
            xh[k * 4 + j] = x;
            gv[k * 4 + j] = g;
            s1 += g;
            s2 += g * x;
        }
    }
    s1 = block_sum(s1, red);
    s2 = block_sum(s2, red);
    const float inv = 1.f / (float)HW;
    const float a1 = s1 * inv, a2 = s2 * inv;
    float4* o4 = reinterpret_cast<float4*>(dy + (long long)nc * HW);
#pragma unroll
    for (int k = 0; k < NG; ++k) {
        const int i = k * NT + tid;
        if (i < Q)
            o4[i] = make_float4(r * (gv[k * 4] - a1 - xh[k * 4] * a2), r * (gv[k * 4 + 1] - a1 - xh[k * 4 + 1] * a2),
                                r * (gv[k * 4 + 2] - a1 - xh[k * 4 + 2] * a2), r * (gv[k * 4 + 3] - a1 - xh[k * 4 + 3] * a2));
    }
}

// ... and for the gradient of a pad-1 reflection-padded consumer (g1: (H + 2) x (W + 2) planes, W % 4 == 0, H >= 3): the padded row's
// 16 bytes and ONE edge dword (padded column 0 or W + 1, whichever this group could need) are loaded unconditionally with y and g2; the
// reflected ROWS 0 and H + 1 belong to the groups of rows 1 and H - 2 only and are added in a second phase that a wave enters only if
// it holds such a group (as instnorm_bwd_split_kernel does).
template <int NT, int EPT, bool G2>
__global__ __launch_bounds__(NT) void instnorm_bwd_fused_fold1_kernel(const float* __restrict__ g1, const float* __restrict__ g2,
                                                                      const float* __restrict__ y, const float* __restrict__ mean,
                                                                      const float* __restrict__ rstd, int act, int H, int W,
                                                                      float* __restrict__ dy) {
    __shared__ float red[NT / 64];
    constexpr int NG = EPT / 4;
    const int nc = blockIdx.x, tid = threadIdx.x, HW = H * W, Q = HW >> 2, W4 = W >> 2;
    const float4* y4 = reinterpret_cast<const float4*>(y + (long long)nc * HW);
    const float* gp = g1 + (long long)nc * (H + 2) * (W + 2);
    const float4* gb = reinterpret_cast<const float4*>((G2 ? g2 : y) + (long long)nc * HW);
    float4 yv[NG], gr[NG];
    float4u gm[NG];
    float ge[NG];
    int gy[NG], gx[NG];
#pragma unroll
    for (int k = 0; k < NG; ++k) {
        const int i = k * NT + tid, ic = i < Q ? i : Q - 1;
        gy[k] = ic / W4;
        gx[k] = (ic - gy[k] * W4) * 4;
        const float* rp = gp + (gy[k] + 1) * (W + 2);
        gm[k] = *reinterpret_cast<const float4u*>(rp + gx[k] + 1);
        ge[k] = rp[gx[k] == 0 ? 0 : W + 1];
        yv[k] = y4[ic];
        if constexpr (G2) gr[k] = gb[ic];
    }
    const float m = mean[nc], r = rstd[nc];
    float4 gq[NG];
    bool border = false;
#pragma unroll
    for (int k = 0; k < NG; ++k) {
        gq[k] = make_float4(gm[k].x, gm[k].y, gm[k].z, gm[k].w);
        if (gx[k] == 0) gq[k].y += ge[k];                 // padded column 0 is the reflection of column 1
        if (gx[k] == W - 4) gq[k].z += ge[k];             // padded column W + 1 is the reflection of column W - 2
        border = border || gy[k] == 1 || gy[k] == H - 2;
    }
    if (__builtin_amdgcn_ballot_w64(border) != 0) {       // wave-uniform: this wave holds groups of row 1 or row H - 2
#pragma unroll
        for (int k = 0; k < NG; ++k) {
            if (gy[k] == 1) { const float4 t = fold1_row4(gp, W, 0, gx[k]); gq[k].x += t.x; gq[k].y += t.y; gq[k].z += t.z; gq[k].w += t.w; }
            if (gy[k] == H - 2) { const float4 t = fold1_row4(gp, W, H + 1, gx[k]); gq[k].x += t.x; gq[k].y += t.y; gq[k].z += t.z; gq[k].w += t.w; }
        }
    }
    float gv[EPT], xh[EPT];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < NG; ++k) {
        const bool in = k * NT + tid < Q;
        const float yy[4] = {yv[k].x, yv[k].y, yv[k].z, yv[k].w};
        float gg[4] = {gq[k].x, gq[k].y, gq[k].z, gq[k].w};
        if constexpr (G2) { gg[0] += gr[k].x; gg[1] += gr[k].y; gg[2] += gr[k].z; gg[3] += gr[k].w; }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float x = in ? (yy[j] - m) * r : 0.f;
            const float g = in ? gg[j] * act_grad_from_xhat(x, act) : 0.f;
            xh[k * 4 + j] = x;
            gv[k * 4 + j] = g;
            s1 += g;
            s2 += g * x;
        }
    }
    s1 = block_sum(s1, red);
    s2 = block_sum(s2, red);
    const float inv = 1.f / (float)HW;
    const float a1 = s1 * inv, a2 = s2 * inv;
    float4* o4 = reinterpret_cast<float4*>(dy + (long long)nc * HW);
#pragma unroll
    for (int k = 0; k < NG; ++k) {
        const int i = k * NT + tid;
        if (i < Q)
            o4[i] = make_float4(r * (gv[k * 4] - a1 - xh[k * 4] * a2), r * (gv[k * 4 + 1] - a1 - xh[k * 4 + 1] * a2),
                                r * (gv[k * 4 + 2] - a1 - xh[k * 4 + 2] * a2), r * (gv[k * 4 + 3] - a1 - xh[k * 4 + 3] * a2));
    }
}

// ... and for small planes of any size with an unfolded gradient (the PatchGAN's 31 x 31 maps: H W = 961 is odd, so the general
// kernel took its element-wise path -- 16 predicated iterations with the loads behind their tests): four elements per thread, every
// load from a clamped index first.
template <bool G2>
__global__ __launch_bounds__(256) void instnorm_bwd_fused_small_kernel(const float* __restrict__ g1, const float* __restrict__ g2,
                                                                       const float* __restrict__ y, const float* __restrict__ mean,
                                                                       const float* __restrict__ rstd, int act, int HW,
                                                                       float* __restrict__ dy) {
    __shared__ float red[4];
    constexpr int EPT = 4;
    const int nc = blockIdx.x, tid = threadIdx.x;
    const float* yp = y + (long long)nc * HW;
    const float* ga = g1 + (long long)nc * HW;
    const float* gb = (G2 ? g2 : g1) + (long long)nc * HW;
    float yv[EPT], gq[EPT], gr[EPT];
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
        const int i = k * 256 + tid, ic = i < HW ? i : HW - 1;
        yv[k] = yp[ic];
        gq[k] = ga[ic];
        if constexpr (G2) gr[k] = gb[ic];
    }
    const float m = mean[nc], r = rstd[nc];
    float gv[EPT], xh[EPT];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
        const bool in = k * 256 + tid < HW;
        const float x = in ? (yv[k] - m) * r : 0.f;
        float g = gq[k];
        if constexpr (G2) g += gr[k];
        g = in ? g * act_grad_from_xhat(x, act) : 0.f;
        xh[k] = x;
        gv[k] = g;
        s1 += g;
        s2 += g * x;
    }
    s1 = block_sum(s1, red);
    s2 = block_sum(s2, red);
    const float inv = 1.f / (float)HW;
    const float a1 = s1 * inv, a2 = s2 * inv;
    float* out = dy + (long long)nc * HW;
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
        const int i = k * 256 + tid;
        if (i < HW) out[i] = r * (gv[k] - a1 - xh[k] * a2);
    }
}

// The same for 256 x 256 planes (unfolded gradient, HW % 4 == 0, HW <= 65536): 1024 threads x 16 float4 groups.  The
// activated gradient of the first 8 groups stays in registers, the other 8 are parked in LDS (128 KiB); the normalised
// activation is recomputed from a second read of y, which the plane's first pass left in the memory-side cache --
// 2 + (1 cached) reads + 1 write per element instead of the 4 + 1 of the reduce / apply pair.  grid: (N*C)
// OB16: dy is stored as bf16 values (its one reader is the stems' weight gradient on the bf16 matrix pipe, wgrad_k7.h, which rounds
// it to bf16 anyway: half the bytes written here and read there)
template <bool FOLD, bool OB16 = false>
__global__ __launch_bounds__(1024) void instnorm_bwd_fused_big_kernel(const float* __restrict__ g1, int p1,
                                                                     const float* __restrict__ g2,
                                                                     const float* __restrict__ y,
                                                                     const float* __restrict__ mean,
                                                                     const float* __restrict__ rstd, int act, int H, int W,
                                                                     float* __restrict__ dy) {
    extern __shared__ float4 park[];                 // [8][1024]
    __shared__ float red[16];
    const int nc = blockIdx.x, tid = threadIdx.x, HW = H * W, Q = HW >> 2, W4 = W >> 2;
    // p1 > 0: the gradient of a reflection-padded convolution, still in padded coordinates (W % 4 == 0: a group of four
    // pixels stays in one row)
    const FoldReader fr{g1 + (long long)nc * (H + 2 * p1) * (W + 2 * p1), H, W, p1, W + 2 * p1};
    const float m = mean[nc], r = rstd[nc];
    const float4* y4 = reinterpret_cast<const float4*>(y + (long long)nc * HW);
    const float4* ga = reinterpret_cast<const float4*>(g1 + (long long)nc * HW);
    const float4* gb = g2 ? reinterpret_cast<const float4*>(g2 + (long long)nc * HW) : nullptr;
    float4* o4 = reinterpret_cast<float4*>(dy + (long long)nc * HW);
    float4 keep[8];
    float s1 = 0.f, s2 = 0.f;
    auto take = [&](int k) -> float4 {
        const int i = k * 1024 + tid;
        float4 yv = make_float4(m, m, m, m), gq = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < Q) {
            yv = y4[i];
            if constexpr (!FOLD) {
                gq = ga[i];
            } else {
                const int yy = i / W4, xx = (i - yy * W4) * 4;
                if (p1 == 1 && H >= 3) gq = fold1_at4(fr.g, H, W, yy, xx);
                else if (p1 <= 3 && W >= 4 + 2 * p1 && H >= 2 * p1 + 2) gq = foldp_at4(fr.g, H, W, p1, yy, xx);
                else gq = make_float4(fr.at(yy, xx), fr.at(yy, xx + 1), fr.at(yy, xx + 2), fr.at(yy, xx + 3));
            }
            if (gb) { const float4 t = gb[i]; gq.x += t.x; gq.y += t.y; gq.z += t.z; gq.w += t.w; }
        }
        const float x0 = (yv.x - m) * r, x1 = (yv.y - m) * r, x2 = (yv.z - m) * r, x3 = (yv.w - m) * r;
        gq.x *= act_grad_from_xhat(x0, act); gq.y *= act_grad_from_xhat(x1, act);
        gq.z *= act_grad_from_xhat(x2, act); gq.w *= act_grad_from_xhat(x3, act);
        s1 += (gq.x + gq.y) + (gq.z + gq.w);
        s2 += (gq.x * x0 + gq.y * x1) + (gq.z * x2 + gq.w * x3);
        return gq;
    };
    // (at most four groups' loads in flight: hoisted all at once they would take the registers `keep` needs)
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        keep[k] = take(k);
        if ((k & 3) == 3) asm volatile("" ::: "memory");
    }
#pragma unroll 4
    for (int k = 8; k < 16; ++k) park[(k - 8) * 1024 + tid] = take(k);
    s1 = block_sum(s1, red);
    s2 = block_sum(s2, red);
    const float inv = 1.f / (float)HW;
    const float a1 = s1 * inv, a2 = s2 * inv;
    auto put = [&](int k, float4 g) {
        const int i = k * 1024 + tid;
        if (i < Q) {
            const float4 yv = y4[i];
            const float4 o = make_float4(r * (g.x - a1 - (yv.x - m) * r * a2), r * (g.y - a1 - (yv.y - m) * r * a2),
                                         r * (g.z - a1 - (yv.z - m) * r * a2), r * (g.w - a1 - (yv.w - m) * r * a2));
            if constexpr (OB16) reinterpret_cast<uint2*>(reinterpret_cast<unsigned short*>(dy) + (long long)nc * HW)[i] = make_uint2(pack_bf16x2(o.x, o.y), pack_bf16x2(o.z, o.w));
            else o4[i] = o;
        }
    };
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        put(k, keep[k]);
        if ((k & 3) == 3) asm volatile("" ::: "memory");
    }
#pragma unroll 4
    for (int k = 8; k < 16; ++k) put(k, park[(k - 8) * 1024 + tid]);
}

}  // namespace apamd

using namespace apamd;

// Which kernel ap_instnorm_bwd launches for a plane geometry: instnorm_bwd_route is the one place that decides it, the launcher
// switches on the answer, and ap_instnorm_bwd_route reports its name from the table below.  The forms with a `g2` template
// parameter (small, vec, fold1) are further split by the presence of a second gradient at the launch.
enum InBwdRoute {
    INBWD_SMALL,            // instnorm_bwd_fused_small_kernel: unfolded, H W <= 1024 and not a multiple of 4
    INBWD_VEC_256,          // instnorm_bwd_fused_vec_kernel<256>: unfolded, H W % 4 == 0, H W <= 4096
    INBWD_VEC_1024,         //                              <1024>: ... H W <= 16384
    INBWD_FOLD1_256,        // instnorm_bwd_fused_fold1_kernel<256>: pad-1 fold, W % 4 == 0, W >= 8, H >= 3
    INBWD_FOLD1_1024,
    INBWD_GENERAL_256,      // instnorm_bwd_fused_kernel<256>: everything else up to 4096 pixels
    INBWD_GENERAL_1024,     //                          <1024>: ... up to 16384
    INBWD_BIG,              // instnorm_bwd_fused_big_kernel<false>: 16384 < H W <= 65536, W % 4 == 0, unfolded
    INBWD_BIG_FOLD,         //                              <true>: ... any fold
    INBWD_BIG_BF16,         //                              <false, true>: unfolded, dy stored as bf16
    INBWD_REDUCE_APPLY,     // the reduce / apply pair: all other planes
};
// kInBwdRouteName[route][second gradient present], in the enum's order
static const char* const kInBwdRouteName[][2] = {
    {"small", "small<g2>"},
    {"vec<256>", "vec<256,g2>"},         {"vec<1024>", "vec<1024,g2>"},
    {"fold1<256>", "fold1<256,g2>"},     {"fold1<1024>", "fold1<1024,g2>"},
    {"general<256>", "general<256>"},    {"general<1024>", "general<1024>"},
    {"big", "big"},                      {"big<fold>", "big<fold>"},          {"big<bf16>", "big<bf16>"},
    {"reduce_apply", "reduce_apply"},
};
static_assert(sizeof(kInBwdRouteName) / sizeof(kInBwdRouteName[0]) == INBWD_REDUCE_APPLY + 1, "one name pair per InBwdRoute");

// act_bits: the launcher's `act` argument (activation in the low byte, bit 8 = dy stored as bf16)
static int instnorm_bwd_route(int g1_pad, int act_bits, int H, int W, InBwdRoute* route) {
    int rc = fold_pad_ok(g1_pad, H, W, "instnorm_bwd");
    if (rc) return rc;
    const bool ob16 = (act_bits & 0x100) != 0;  // bit 8: dy is stored as bf16 values (256 x 256-class planes without a fold only)
    const int act = act_bits & 0xff;
    if (act < 0 || act > 2) return fail(AP_ERR_INVALID, "instnorm_bwd: act %d", act);
    if (ob16 && !(g1_pad == 0 && H * W > 16384 && H * W <= 65536 && (W % 4) == 0))
        return fail(AP_ERR_UNSUPPORTED, "instnorm_bwd: a bf16 dy is written by the big-plane kernel only (%dx%d, fold %d)", H, W, g1_pad);
    const bool plain_vec = g1_pad == 0 && ((H * W) & 3) == 0;     // unfolded gradient, whole 16-byte groups: the load-phase form
    const bool fold1_vec = g1_pad == 1 && (W & 3) == 0 && H >= 3 && W >= 8;   // pad-1 fold, the same
    if (g1_pad == 0 && H * W <= 1024 && ((H * W) & 3) != 0) *route = INBWD_SMALL;      // small planes that are not whole 16-byte groups
    else if (H * W <= 4096) *route = plain_vec ? INBWD_VEC_256 : (fold1_vec ? INBWD_FOLD1_256 : INBWD_GENERAL_256);
    else if (H * W <= 16384) *route = plain_vec ? INBWD_VEC_1024 : (fold1_vec ? INBWD_FOLD1_1024 : INBWD_GENERAL_1024);
    else if (H * W <= 65536 && (W % 4) == 0 && W >= 4) *route = ob16 ? INBWD_BIG_BF16 : (g1_pad == 0 ? INBWD_BIG : INBWD_BIG_FOLD);
    else *route = INBWD_REDUCE_APPLY;
    return AP_OK;
}

// the one-workgroup-per-plane InstanceNorm backward with NT threads: the load-phase forms where the gradient comes in whole
// 16-byte groups (unfolded / pad-1 fold, with or without a second contribution), else the general one
template <int NT>
static int launch_instnorm_bwd_fused(bool plain_vec, bool fold1_vec, const float* g1, int g1_pad, const float* g2, const float* y,
                                      const float* mean, const float* rstd, int act, int NC, int H, int W, float* dy, ap_stream_t stream) {
    const dim3 grid(NC), block(NT);
    hipStream_t st = (hipStream_t)stream;
    if (plain_vec && g2) hipLaunchKernelGGL((instnorm_bwd_fused_vec_kernel<NT, 16, true>), grid, block, 0, st, g1, g2, y, mean, rstd, act, H * W, dy);
    else if (plain_vec) hipLaunchKernelGGL((instnorm_bwd_fused_vec_kernel<NT, 16, false>), grid, block, 0, st, g1, g2, y, mean, rstd, act, H * W, dy);
    else if (fold1_vec && g2) hipLaunchKernelGGL((instnorm_bwd_fused_fold1_kernel<NT, 16, true>), grid, block, 0, st, g1, g2, y, mean, rstd, act, H, W, dy);
    else if (fold1_vec) hipLaunchKernelGGL((instnorm_bwd_fused_fold1_kernel<NT, 16, false>), grid, block, 0, st, g1, g2, y, mean, rstd, act, H, W, dy);
    else hipLaunchKernelGGL((instnorm_bwd_fused_kernel<NT, 16>), grid, block, 0, st, g1, g1_pad, g2, y, mean, rstd, act, H, W, dy);
    return check_launch("instnorm_bwd_fused_kernel");
}

extern "C" {

int ap_instnorm_bwd(const float* g1, int32_t g1_pad, const float* g2, const float* y, const float* mean,
                    const float* rstd, int32_t act, int32_t NC, int32_t H, int32_t W, float* sums_ws, float* dy,
                    ap_stream_t stream) {
    int rc = fold_args_ok(g1, g1_pad, H, W, "instnorm_bwd");
    if (rc) return rc;
    if (!y || !mean || !rstd || !sums_ws || !dy) return fail(AP_ERR_INVALID, "instnorm_bwd: null pointer");
    InBwdRoute route;
    rc = instnorm_bwd_route(g1_pad, act, H, W, &route);
    if (rc) return rc;
    act &= 0xff;
    if (NC < 1 || NC > 65535) return fail(AP_ERR_UNSUPPORTED, "instnorm_bwd: N*C=%d", NC);
    switch (route) {
    case INBWD_SMALL:
        if (g2) hipLaunchKernelGGL(instnorm_bwd_fused_small_kernel<true>, dim3(NC), dim3(256), 0, (hipStream_t)stream, g1, g2, y, mean, rstd, act, H * W, dy);
        else hipLaunchKernelGGL(instnorm_bwd_fused_small_kernel<false>, dim3(NC), dim3(256), 0, (hipStream_t)stream, g1, g2, y, mean, rstd, act, H * W, dy);
        return check_launch("instnorm_bwd_fused_small_kernel");
    case INBWD_VEC_256:
    case INBWD_FOLD1_256:
    case INBWD_GENERAL_256:
        return launch_instnorm_bwd_fused<256>(route == INBWD_VEC_256, route == INBWD_FOLD1_256, g1, g1_pad, g2, y, mean, rstd, act, NC, H, W, dy, stream);
    case INBWD_VEC_1024:
    case INBWD_FOLD1_1024:
    case INBWD_GENERAL_1024:
        return launch_instnorm_bwd_fused<1024>(route == INBWD_VEC_1024, route == INBWD_FOLD1_1024, g1, g1_pad, g2, y, mean, rstd, act, NC, H, W, dy, stream);
    case INBWD_BIG:
    case INBWD_BIG_FOLD:
    case INBWD_BIG_BF16: {
        // (the three instantiations have one signature: the launch raises the dynamic-LDS limit of the one it takes)
        const auto kernel = route == INBWD_BIG_BF16 ? &instnorm_bwd_fused_big_kernel<false, true>
                                                    : (route == INBWD_BIG ? &instnorm_bwd_fused_big_kernel<false> : &instnorm_bwd_fused_big_kernel<true>);
        const size_t lds = 8 * 1024 * sizeof(float4);
        rc = ensure_dyn_lds(reinterpret_cast<const void*>(kernel), (int)lds);
        if (rc) return rc;
        hipLaunchKernelGGL(kernel, dim3(NC), dim3(1024), lds, (hipStream_t)stream, g1, g1_pad, g2, y, mean, rstd, act, H, W, dy);
        return check_launch("instnorm_bwd_fused_big_kernel");
    }
    case INBWD_REDUCE_APPLY:
        break;
    }
    hipLaunchKernelGGL(instnorm_bwd_reduce_kernel, dim3(NC), dim3(256), 0, (hipStream_t)stream, g1, g1_pad, g2, y,
                       mean, rstd, act, H, W, sums_ws);
    rc = check_launch("instnorm_bwd_reduce_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(instnorm_bwd_apply_kernel, dim3(sweep_blocks(H, W), NC), dim3(256), 0, (hipStream_t)stream, g1, g1_pad, g2, y,
                       mean, rstd, act, H, W, sums_ws, dy);
    return check_launch("instnorm_bwd_apply_kernel");
}

int ap_instnorm_bwd_route(int32_t g1_pad, int32_t has_g2, int32_t act_bits, int32_t H, int32_t W, char* buf, int32_t buflen) {
    InBwdRoute route;
    int rc = instnorm_bwd_route(g1_pad, act_bits, H, W, &route);
    if (rc) return rc;
    if (!buf || buflen < 1) return fail(AP_ERR_INVALID, "instnorm_bwd_route: bad buffer");
    snprintf(buf, buflen, "%s", kInBwdRouteName[route][has_g2 ? 1 : 0]);
    return AP_OK;
}

}  // extern "C"
