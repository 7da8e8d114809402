// seq_encoder.hip -- the self-attention encoder of Module1's pose network at inference, two launches per layer
// (include/animateportrait_seq.h: apq_enc_qkv, apq_enc_attn_ff; Module1/src/models/model_audio2landmark_speaker_aware.py:195-209).
// d_model = 64, two heads of 32, d_ff hidden units, one sequence of up to 512 rows: through the library that is a chain of tiny
// launches (the hand-written Norm alone is seven of them).
//
// Every product runs on the fp32 matrix pipe as v_mfma_f32_16x16x4_f32, in the orientation of seq_lstm.hip:
//   A (16 x 4)  = 16 rows of the LEFT matrix (weights [out][in], keys, or V transposed)   lane l: row l & 15, k-slot l >> 4
//   B (4 x 16)  = 16 rows of activations (the workgroup's 16 query rows)                  lane l: query row l & 15, k-slot l >> 4
//   D (16 x 16) : lane l holds query row l & 15 and the four outputs 4 (l >> 4) + reg of the tile
// K is walked in chunks of 16: k-slot s of matrix instruction m of a chunk is k = 16 chunk + 4 s + m, so a lane's four A values
// and its four B values of a chunk are 16 contiguous bytes each.  With that order an accumulator tile is the next product's B
// operand as it stands (register m of slot s IS k = 4 s + m): the feed-forward's hidden activations go from linear_1 to linear_2
// in registers.
//
// apq_enc_qkv:      256 threads own 16 of the B T rows: Norm_1 into LDS, then wave w makes columns 16 w .. 16 w + 15 of q, k, v.
// apq_enc_attn_ff:  512 threads own 16 query rows of ONE sequence:
//   scores [2][16][T] into LDS (K tiles straight from L2), softmax in place (16 lanes per row, maximum first), p V with the keys
//   split over two waves per output tile, out-projection + residual, Norm_2, the feed-forward with each wave on its own 32 hidden
//   units of every 256-unit chunk (W1 and W2 fragments straight from L2), the eight partial outputs added in wave order through
//   LDS, residual, the optional closing Norm, store.
// A workgroup reads q, k, v and the weights, and writes its own 16 rows: no traffic between workgroups, no atomics, no spin.  Rows
// and keys past the end of the sequence are never read: their index is clamped, their probability is zero.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "seq_encoder_checks.h"

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int D = APQ_ENC_D;
constexpr int DK = apq::kEncDk;
constexpr int DS = apq::kEncStride;
constexpr int ROWS = apq::kEncRows;
constexpr int NW = apq::kAttnWaves;

struct QkvParams {
    const float *x, *alpha, *bias, *w[3], *b[3];
    float* out[3];
    float eps;
    long long rows;      // B T
};

struct AttnParams {
    const float *x, *q, *k, *v, *wo, *bo, *alpha2, *bias2, *w1, *b1, *w2, *b2, *alpha_f, *bias_f;
    float* y;
    float eps2, eps_f;
    int T, tiles, ss, region0, d_ff;
};

__device__ inline const float4& ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ inline float4& at4(float* p) { return *reinterpret_cast<float4*>(p); }
__device__ inline f32x4 vec(const float4& a) { return f32x4{a.x, a.y, a.z, a.w}; }
__device__ inline float4 flt4(const f32x4& a) { return make_float4(a[0], a[1], a[2], a[3]); }

// one K chunk of 16: four matrix instructions, k-slot s of instruction m is k = 4 s + m
__device__ inline f32x4 mma16(const float4& a, const float4& b, f32x4 acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
    return acc;
}

// the sum over the 16 lanes that share a row (lanes 16 i .. 16 i + 15 of a wave): every lane gets the same bits
__device__ inline float row_sum(float s) {
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) s += __shfl_xor(s, m);
    return s;
}

__device__ inline float row_max(float s) {
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) s = fmaxf(s, __shfl_xor(s, m));
    return s;
}

// module1.Norm on a row of 64 held four values a lane by 16 lanes: alpha (x - mean) / (std_unbiased + eps) + bias
__device__ inline float4 norm_row(const float4& v, const float4& alpha, const float4& bias, float eps) {
    const float mean = row_sum((v.x + v.y) + (v.z + v.w)) * (1.f / D);
    const float4 d = make_float4(v.x - mean, v.y - mean, v.z - mean, v.w - mean);
    const float var = row_sum((d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w)) / (float)(D - 1);
    const float den = sqrtf(var) + eps;
    return make_float4(alpha.x * d.x / den + bias.x, alpha.y * d.y / den + bias.y, alpha.z * d.z / den + bias.z,
                       alpha.w * d.w / den + bias.w);
}

// grid: ceil(B T / 16) workgroups of 256 threads
__global__ __launch_bounds__(apq::kQkvThreads) void enc_qkv_kernel(const QkvParams p) {
    __shared__ float4 xs4[ROWS * DS / 4];
    float* const xs = reinterpret_cast<float*>(xs4);                    // [16][DS]: Norm_1 of the tile
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const long long row0 = (long long)blockIdx.x * ROWS;
    {
        const int row = tid >> 4, j = tid & 15;                         // 16 lanes per row, four values each
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);                     // (a row past the end: zeros, never stored)
        if (row0 + row < p.rows) v = ld4(p.x + (row0 + row) * D + 4 * j);
        at4(xs + row * DS + 4 * j) = norm_row(v, ld4(p.alpha + 4 * j), ld4(p.bias + 4 * j), p.eps);
    }
    __syncthreads();
    const int u0 = wave * 16;                                           // this wave's 16 output columns of q, k and v
    f32x4 acc[3];
#pragma unroll
    for (int m = 0; m < 3; ++m) acc[m] = vec(ld4(p.b[m] + u0 + 4 * g));
#pragma unroll
    for (int c = 0; c < D / 16; ++c) {
        const float4 xb = ld4(xs + r * DS + 16 * c + 4 * g);
#pragma unroll
        for (int m = 0; m < 3; ++m) acc[m] = mma16(ld4(p.w[m] + (u0 + r) * D + 16 * c + 4 * g), xb, acc[m]);
    }
    if (row0 + r < p.rows) {
#pragma unroll
        for (int m = 0; m < 3; ++m) at4(p.out[m] + (row0 + r) * D + u0 + 4 * g) = flt4(acc[m]);
    }
}

// grid: B ceil(T / 16) workgroups of 512 threads; dynamic LDS: plan.lds_bytes
__global__ __launch_bounds__(apq::kAttnThreads) void enc_attn_ff_kernel(const AttnParams p) {
    extern __shared__ float4 lds4[];
    float* const sc = reinterpret_cast<float*>(lds4);       // [2][16][ss] scores, then probabilities; at the end the partial outputs [8][16][DS]
    float* const qs = sc + p.region0;                       // [16][DS] the query tile
    float* const cs = qs + ROWS * DS;                       // [16][DS] the heads' outputs side by side
    float* const x1s = cs + ROWS * DS;                      // [16][DS] x, then x + attention
    float* const xns = x1s + ROWS * DS;                     // [16][DS] the second half of p V, then Norm_2 of x1
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int row = tid >> 4, j = tid & 15;                 // the 16-lanes-per-row view; rows 0 .. 15 are threads 0 .. 255
    const int T = p.T, ss = p.ss, nkt = (T + 15) / 16;
    const int t0 = (int)(blockIdx.x % p.tiles) * ROWS;
    const long long seq = (long long)(blockIdx.x / p.tiles) * T;        // first row of this workgroup's sequence

    if (tid < ROWS * 16) {
        float4 q4 = make_float4(0.f, 0.f, 0.f, 0.f), x4 = q4;           // (rows past the end: zeros, never stored)
        if (t0 + row < T) {
            q4 = ld4(p.q + (seq + t0 + row) * D + 4 * j);
            x4 = ld4(p.x + (seq + t0 + row) * D + 4 * j);
        }
        at4(qs + row * DS + 4 * j) = q4;
        at4(x1s + row * DS + 4 * j) = x4;
    }
    __syncthreads();

    // scores: wave w takes the key tiles w, w + 8, ..., both heads of a tile side by side (two independent accumulators)
    const float sqrt_dk = sqrtf((float)DK);
    for (int kt = wave; kt < nkt; kt += NW) {
        const float* krow = p.k + (seq + min(16 * kt + r, T - 1)) * D + 4 * g;
        f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int c = 0; c < DK / 16; ++c)
#pragma unroll
            for (int h = 0; h < 2; ++h) acc[h] = mma16(ld4(krow + h * DK + 16 * c), ld4(qs + r * DS + h * DK + 16 * c + 4 * g), acc[h]);
#pragma unroll
        for (int h = 0; h < 2; ++h)                                     // (the entries of keys past T - 1 are never read back)
            at4(sc + (h * ROWS + r) * ss + 16 * kt + 4 * g) =
                make_float4(acc[h][0] / sqrt_dk, acc[h][1] / sqrt_dk, acc[h][2] / sqrt_dk, acc[h][3] / sqrt_dk);
    }
    __syncthreads();

    // softmax over the T keys of each of the 32 (head, row) pairs, 16 lanes a pair; keys T .. 16 nkt - 1 get probability 0
    {
        float* const srow = sc + row * ss;                              // row = 16 head + query row here
        float mx = -INFINITY;
        for (int key = j; key < T; key += 16) mx = fmaxf(mx, srow[key]);
        mx = row_max(mx);
        float sum = 0.f;
        for (int key = j; key < T; key += 16) {
            const float e = expf(srow[key] - mx);
            srow[key] = e;
            sum += e;
        }
        sum = row_sum(sum);
        for (int key = j; key < 16 * nkt; key += 16) srow[key] = key < T ? srow[key] / sum : 0.f;
    }
    __syncthreads();

    // p V: output tile (head, 16 of its 32 columns) = wave & 3, the key chunks of even / odd index by wave >> 2
    {
        const int tile = wave & 3, half = wave >> 2, h = tile >> 1, col = h * DK + (tile & 1) * 16;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const float* vcol = p.v + seq * D + col + r;
        for (int c = half; c < nkt; c += 2) {
            const int k0 = 16 * c + 4 * g;
            const float4 va = make_float4(vcol[min(k0, T - 1) * D], vcol[min(k0 + 1, T - 1) * D], vcol[min(k0 + 2, T - 1) * D],
                                          vcol[min(k0 + 3, T - 1) * D]);
            acc = mma16(va, ld4(sc + (h * ROWS + r) * ss + k0), acc);
        }
        at4((half ? xns : cs) + r * DS + col + 4 * g) = flt4(acc);
    }
    __syncthreads();
    if (tid < ROWS * 16) {
        const float4 a = ld4(cs + row * DS + 4 * j), b = ld4(xns + row * DS + 4 * j);
        at4(cs + row * DS + 4 * j) = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
    }
    __syncthreads();

    // x1 = x + (c wo^T + bo): waves 0 .. 3, 16 output columns each
    if (wave < D / 16) {
        const int u0 = wave * 16;
        f32x4 acc = vec(ld4(p.bo + u0 + 4 * g));
#pragma unroll
        for (int c = 0; c < D / 16; ++c) acc = mma16(ld4(p.wo + (u0 + r) * D + 16 * c + 4 * g), ld4(cs + r * DS + 16 * c + 4 * g), acc);
        float4& x1 = at4(x1s + r * DS + u0 + 4 * g);
        x1 = make_float4(x1.x + acc[0], x1.y + acc[1], x1.z + acc[2], x1.w + acc[3]);
    }
    __syncthreads();
    if (tid < ROWS * 16)
        at4(xns + row * DS + 4 * j) = norm_row(ld4(x1s + row * DS + 4 * j), ld4(p.alpha2 + 4 * j), ld4(p.bias2 + 4 * j), p.eps2);
    __syncthreads();

    // feed-forward: of every chunk of 256 hidden units wave w takes 32 w .. 32 w + 31 as two tiles of 16.  A tile's relu output
    // is the B operand of linear_2 as it stands: register m of k-slot g is hidden unit 4 g + m of the tile.
    float4 xb[D / 16];
#pragma unroll
    for (int c = 0; c < D / 16; ++c) xb[c] = ld4(xns + r * DS + 16 * c + 4 * g);
    f32x4 yacc[D / 16];
#pragma unroll
    for (int o = 0; o < D / 16; ++o) yacc[o] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int hid0 = wave * 32; hid0 < p.d_ff; hid0 += APQ_ENC_FF_CHUNK) {
        f32x4 hacc[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) hacc[t] = vec(ld4(p.b1 + hid0 + 16 * t + 4 * g));
#pragma unroll
        for (int c = 0; c < D / 16; ++c)
#pragma unroll
            for (int t = 0; t < 2; ++t) hacc[t] = mma16(ld4(p.w1 + (hid0 + 16 * t + r) * D + 16 * c + 4 * g), xb[c], hacc[t]);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const float4 hb = make_float4(fmaxf(hacc[t][0], 0.f), fmaxf(hacc[t][1], 0.f), fmaxf(hacc[t][2], 0.f), fmaxf(hacc[t][3], 0.f));
#pragma unroll
            for (int o = 0; o < D / 16; ++o)
                yacc[o] = mma16(ld4(p.w2 + (long long)(16 * o + r) * p.d_ff + hid0 + 16 * t + 4 * g), hb, yacc[o]);
        }
    }
    // (the probabilities were last read before the barriers above: their region now takes the eight partial outputs)
    float* const part = sc + wave * ROWS * DS;
#pragma unroll
    for (int o = 0; o < D / 16; ++o) at4(part + r * DS + 16 * o + 4 * g) = flt4(yacc[o]);
    __syncthreads();

    // y = x1 + (sum of the partial outputs in wave order + b2), the closing Norm where asked for
    if (tid < ROWS * 16) {
        float4 s = ld4(sc + row * DS + 4 * j);
#pragma unroll
        for (int w = 1; w < NW; ++w) {
            const float4 a = ld4(sc + (w * ROWS + row) * DS + 4 * j);
            s = make_float4(s.x + a.x, s.y + a.y, s.z + a.z, s.w + a.w);
        }
        const float4 b2 = ld4(p.b2 + 4 * j), x1 = ld4(x1s + row * DS + 4 * j);
        float4 y = make_float4(x1.x + (s.x + b2.x), x1.y + (s.y + b2.y), x1.z + (s.z + b2.z), x1.w + (s.w + b2.w));
        if (p.alpha_f) y = norm_row(y, ld4(p.alpha_f + 4 * j), ld4(p.bias_f + 4 * j), p.eps_f);     // (uniform: whole waves)
        if (t0 + row < T) at4(p.y + (seq + t0 + row) * D + 4 * j) = y;
    }
}

int launched(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(apq::err_buf(), 256, "%s: launch failed: %s", what, hipGetErrorString(e));
        return APQ_ERR_LAUNCH;
    }
    return APQ_OK;
}

}  // namespace

extern "C" {

int32_t apq_enc_qkv_ok(const float* x, const float* alpha, const float* bias, float eps, const float* wq, const float* bq,
                       const float* wk, const float* bk, const float* wv, const float* bv, const float* q, const float* k,
                       const float* v, int32_t B, int32_t T, int32_t d_model) {
    (void)eps;
    return apq::check_enc_qkv(x, alpha, bias, wq, bq, wk, bk, wv, bv, q, k, v, B, T, d_model) == APQ_OK ? 1 : 0;
}

int apq_enc_qkv(const float* x, const float* alpha, const float* bias, float eps, const float* wq, const float* bq, const float* wk,
                const float* bk, const float* wv, const float* bv, float* q, float* k, float* v, int32_t B, int32_t T,
                int32_t d_model, void* stream) {
    const int rc = apq::check_enc_qkv(x, alpha, bias, wq, bq, wk, bk, wv, bv, q, k, v, B, T, d_model);
    if (rc != APQ_OK) return rc;
    QkvParams p;
    p.x = x; p.alpha = alpha; p.bias = bias; p.eps = eps;
    p.w[0] = wq; p.w[1] = wk; p.w[2] = wv; p.b[0] = bq; p.b[1] = bk; p.b[2] = bv;
    p.out[0] = q; p.out[1] = k; p.out[2] = v;
    p.rows = (long long)B * T;
    (void)hipGetLastError();
    hipLaunchKernelGGL(enc_qkv_kernel, dim3((unsigned)((p.rows + ROWS - 1) / ROWS)), dim3(apq::kQkvThreads), 0, (hipStream_t)stream, p);
    return launched("enc_qkv");
}

int32_t apq_enc_attn_ff_ok(const float* x, const float* q, const float* k, const float* v, const float* wo, const float* bo,
                           const float* alpha2, const float* bias2, float eps2, const float* w1, const float* b1, const float* w2,
                           const float* b2, const float* alpha_f, const float* bias_f, float eps_f, const float* y, int32_t B,
                           int32_t T, int32_t d_model, int32_t heads, int32_t d_ff) {
    (void)eps2;
    (void)eps_f;
    apq::EncAttnPlan pl;
    return apq::check_enc_attn_ff(x, q, k, v, wo, bo, alpha2, bias2, w1, b1, w2, b2, alpha_f, bias_f, y, B, T, d_model, heads, d_ff,
                                  &pl) == APQ_OK ? 1 : 0;
}

int apq_enc_attn_ff(const float* x, const float* q, const float* k, const float* v, const float* wo, const float* bo,
                    const float* alpha2, const float* bias2, float eps2, const float* w1, const float* b1, const float* w2,
                    const float* b2, const float* alpha_f, const float* bias_f, float eps_f, float* y, int32_t B, int32_t T,
                    int32_t d_model, int32_t heads, int32_t d_ff, void* stream) {
    apq::EncAttnPlan pl;
    const int rc = apq::check_enc_attn_ff(x, q, k, v, wo, bo, alpha2, bias2, w1, b1, w2, b2, alpha_f, bias_f, y, B, T, d_model, heads,
                                          d_ff, &pl);
    if (rc != APQ_OK) return rc;
    // the scores of a long sequence need more than the 64 KiB a kernel gets without asking
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&enc_attn_ff_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)apq::kEncMaxLds);
    if (e != hipSuccess) {
        snprintf(apq::err_buf(), 256, "enc_attn_ff: hipFuncSetAttribute: %s", hipGetErrorString(e));
        return APQ_ERR_LAUNCH;
    }
    AttnParams p;
    p.x = x; p.q = q; p.k = k; p.v = v; p.wo = wo; p.bo = bo; p.alpha2 = alpha2; p.bias2 = bias2; p.eps2 = eps2;
    p.w1 = w1; p.b1 = b1; p.w2 = w2; p.b2 = b2; p.alpha_f = alpha_f; p.bias_f = bias_f; p.eps_f = eps_f; p.y = y;
    p.T = T; p.tiles = pl.tiles; p.ss = pl.ss; p.region0 = pl.region0; p.d_ff = d_ff;
    (void)hipGetLastError();
    hipLaunchKernelGGL(enc_attn_ff_kernel, dim3((unsigned)pl.blocks), dim3(apq::kAttnThreads), pl.lds_bytes, (hipStream_t)stream, p);
    return launched("enc_attn_ff");
}

}  // extern "C"
