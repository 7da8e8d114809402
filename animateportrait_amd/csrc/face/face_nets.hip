// The detector's three nets (include/animateportrait_face.h), fp32 FMA with fp32 accumulation: their layers are 3..128
// channels wide, too narrow for the matrix pipe, and the thresholds want fp32-class scores.
//
// P-Net is one fused launch per level: a workgroup owns an 8 x 8 tile of the output map, stages the 26 x 26 x 3 patch of the
// level it depends on in LDS (preprocessed on load), and runs conv1+PReLU -> ceil-mode pool -> conv2+PReLU -> conv3+PReLU ->
// the two 1x1 heads -> softmax from LDS to LDS; the epilogue writes the maps (when asked) and appends the positions above the
// threshold to the candidate list with a vector atomic.
// R-Net and O-Net run layer by layer over the batch of cut-outs through two ping-pong buffers of the caller's workspace;
// rows at or beyond the device-side count return at once.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "face_checks.h"

namespace {

using apf::fail;
constexpr int THREADS = 256;

__device__ __forceinline__ float prep(uint8_t v) { return ((float)v - 127.5f) * 0.0078125f; }
__device__ __forceinline__ float prelu(float v, float a) { return v > 0.f ? v : a * v; }

// ---- P-Net ---------------------------------------------------------------------------------------------------------------
constexpr int T = 8, IN_T = 2 * T + 10, C1_T = 2 * T + 8, P_T = T + 4, C2_T = T + 2;
// offsets into the packed parameters
constexpr int P_W1 = 0, P_B1 = 270, P_A1 = 280, P_W2 = 290, P_B2 = 1730, P_A2 = 1746, P_W3 = 1762, P_B3 = 6370, P_A3 = 6402,
              P_W41 = 6434, P_B41 = 6498, P_W42 = 6500, P_B42 = 6628;
static_assert(P_B42 + 4 == APF_PNET_PARAMS, "P-Net's parameter count");

// valid k3 convolution + PReLU from LDS to LDS, G output channels per work item
template <int CIN, int COUT, int G, int IN_S, int OUT_S>
__device__ __forceinline__ void conv3_lds(const float* in, float* out, const float* w, const float* b, const float* a) {
    for (int e = threadIdx.x; e < (COUT / G) * OUT_S * OUT_S; e += THREADS) {
        const int pos = e % (OUT_S * OUT_S), co = (e / (OUT_S * OUT_S)) * G, y = pos / OUT_S, x = pos % OUT_S;
        float acc[G];
        for (int g = 0; g < G; ++g) acc[g] = b[co + g];
        for (int ci = 0; ci < CIN; ++ci)
            for (int ky = 0; ky < 3; ++ky)
                for (int kx = 0; kx < 3; ++kx) {
                    const float v = in[(ci * IN_S + y + ky) * IN_S + x + kx];
                    for (int g = 0; g < G; ++g) acc[g] = fmaf(v, w[((co + g) * CIN + ci) * 9 + ky * 3 + kx], acc[g]);
                }
        for (int g = 0; g < G; ++g) out[((co + g) * OUT_S + y) * OUT_S + x] = prelu(acc[g], a[co + g]);
    }
}

__global__ __launch_bounds__(THREADS) void pnet_kernel(const uint8_t* level, int h, int w, const float* par, float threshold, float* prob,
                                                        float* off, int32_t* cand_idx, float* cand_score, float* cand_off,
                                                        int32_t* cand_count) {
    __shared__ float s_in[3 * IN_T * IN_T];        // later conv2's output (16 x 10 x 10)
    __shared__ float s_c1[10 * C1_T * C1_T];       // later conv3's output (32 x 8 x 8)
    __shared__ float s_p[10 * P_T * P_T];
    static_assert(16 * C2_T * C2_T <= 3 * IN_T * IN_T && 32 * T * T <= 10 * C1_T * C1_T, "aliased buffers fit");
    const int ph = (h - 2 + 1) / 2, pw = (w - 2 + 1) / 2, mh = ph - 4, mw = pw - 4;
    const int oy0 = blockIdx.y * T, ox0 = blockIdx.x * T;

    for (int e = threadIdx.x; e < 3 * IN_T * IN_T; e += THREADS) {
        const int c = e / (IN_T * IN_T), y = (e / IN_T) % IN_T, x = e % IN_T, gy = 2 * oy0 + y, gx = 2 * ox0 + x;
        s_in[e] = (gy < h && gx < w) ? prep(level[((size_t)gy * w + gx) * 3 + c]) : 0.f;
    }
    __syncthreads();
    conv3_lds<3, 10, 10, IN_T, C1_T>(s_in, s_c1, par + P_W1, par + P_B1, par + P_A1);
    __syncthreads();
    // ceil-mode 2/2 pool: a window that crosses the edge of conv1's (h-2) x (w-2) output takes what lies inside
    for (int e = threadIdx.x; e < 10 * P_T * P_T; e += THREADS) {
        const int c = e / (P_T * P_T), y = (e / P_T) % P_T, x = e % P_T, gy = oy0 + y, gx = ox0 + x;
        float m = 0.f;
        if (gy < ph && gx < pw) {
            const float* p = s_c1 + (c * C1_T + 2 * y) * C1_T + 2 * x;
            const bool down = 2 * gy + 1 < h - 2, right = 2 * gx + 1 < w - 2;
            m = p[0];
            if (right) m = fmaxf(m, p[1]);
            if (down) m = fmaxf(m, p[C1_T]);
            if (down && right) m = fmaxf(m, p[C1_T + 1]);
        }
        s_p[e] = m;
    }
    __syncthreads();
    float* s_c2 = s_in;
    float* s_c3 = s_c1;
    conv3_lds<10, 16, 4, P_T, C2_T>(s_p, s_c2, par + P_W2, par + P_B2, par + P_A2);
    __syncthreads();
    conv3_lds<16, 32, 4, C2_T, T>(s_c2, s_c3, par + P_W3, par + P_B3, par + P_A3);
    __syncthreads();
    if (threadIdx.x < T * T) {
        const int y = threadIdx.x / T, x = threadIdx.x % T, gy = oy0 + y, gx = ox0 + x;
        if (gy < mh && gx < mw) {
            float o[6];
            for (int j = 0; j < 2; ++j) o[j] = par[P_B41 + j];
            for (int j = 0; j < 4; ++j) o[2 + j] = par[P_B42 + j];
            for (int c = 0; c < 32; ++c) {
                const float v = s_c3[(c * T + y) * T + x];
                for (int j = 0; j < 2; ++j) o[j] = fmaf(v, par[P_W41 + j * 32 + c], o[j]);
                for (int j = 0; j < 4; ++j) o[2 + j] = fmaf(v, par[P_W42 + j * 32 + c], o[2 + j]);
            }
            const float m = fmaxf(o[0], o[1]), e0 = expf(o[0] - m), e1 = expf(o[1] - m), p1 = e1 / (e0 + e1);
            const int idx = gy * mw + gx;
            if (prob) prob[idx] = p1;
            if (off)
                for (int j = 0; j < 4; ++j) off[(size_t)j * mh * mw + idx] = o[2 + j];
            if (p1 > threshold) {
                const int slot = atomicAdd(cand_count, 1);
                if (slot < APF_CAP_LEVEL) {
                    cand_idx[slot] = idx;
                    cand_score[slot] = p1;
                    for (int j = 0; j < 4; ++j) cand_off[(size_t)slot * 4 + j] = o[2 + j];
                }
            }
        }
    }
}

// ---- R-Net, O-Net ----------------------------------------------------------------------------------------------------------
// valid convolution + PReLU, NCHW fp32 (or the uint8 NHWC cut-outs, preprocessed on load); 4 output channels per thread
template <bool U8>
__global__ __launch_bounds__(THREADS) void conv_prelu_kernel(const void* in_, float* out, const float* w, const float* b, const float* a,
                                                              const int32_t* count, int cap, int cin, int cout, int k, int is, int os) {
    const long e = (long)blockIdx.x * THREADS + threadIdx.x;
    const int per = (cout / 4) * os * os;
    const int n = (int)(e / per);
    if (n >= min(*count, cap)) return;
    const int r = (int)(e % per), co = (r / (os * os)) * 4, y = (r / os) % os, x = r % os;
    float acc[4];
    for (int g = 0; g < 4; ++g) acc[g] = b[co + g];
    for (int ci = 0; ci < cin; ++ci)
        for (int ky = 0; ky < k; ++ky)
            for (int kx = 0; kx < k; ++kx) {
                float v;
                if (U8) v = prep(((const uint8_t*)in_)[(((size_t)n * is + y + ky) * is + x + kx) * 3 + ci]);
                else v = ((const float*)in_)[(((size_t)n * cin + ci) * is + y + ky) * is + x + kx];
                for (int g = 0; g < 4; ++g) acc[g] = fmaf(v, w[(((co + g) * cin + ci) * k + ky) * k + kx], acc[g]);
            }
    for (int g = 0; g < 4; ++g) out[(((size_t)n * cout + co + g) * os + y) * os + x] = prelu(acc[g], a[co + g]);
}

// ceil-mode max-pool, window k, stride 2: a window that crosses the edge takes what lies inside
__global__ __launch_bounds__(THREADS) void maxpool_kernel(const float* in, float* out, const int32_t* count, int cap, int c, int k, int is,
                                                           int os) {
    const long e = (long)blockIdx.x * THREADS + threadIdx.x;
    const int per = c * os * os;
    const int n = (int)(e / per);
    if (n >= min(*count, cap)) return;
    const int r = (int)(e % per), ch = r / (os * os), y = (r / os) % os, x = r % os;
    const float* p = in + ((size_t)n * c + ch) * is * is;
    float m = -INFINITY;
    for (int ky = 0; ky < k && 2 * y + ky < is; ++ky)
        for (int kx = 0; kx < k && 2 * x + kx < is; ++kx) m = fmaxf(m, p[(2 * y + ky) * is + 2 * x + kx]);
    out[e] = m;
}

// hidden = PReLU(in (n, fin) @ wt (fin, fout) + b)
__global__ __launch_bounds__(THREADS) void fc_prelu_kernel(const float* in, float* out, const float* wt, const float* b, const float* a,
                                                            const int32_t* count, int cap, int fin, int fout) {
    const long e = (long)blockIdx.x * THREADS + threadIdx.x;
    const int n = (int)(e / fout), j = (int)(e % fout);
    if (n >= min(*count, cap)) return;
    const float* x = in + (size_t)n * fin;
    float acc = b[j];
    for (int i = 0; i < fin; ++i) acc = fmaf(x[i], wt[(size_t)i * fout + j], acc);
    out[e] = prelu(acc, a[j]);
}

// the heads: 2 logits -> softmax, 4 offsets, n_lm landmarks; weights (out, in) followed by their bias, head after head
__global__ __launch_bounds__(THREADS) void heads_kernel(const float* hidden, const float* w, const int32_t* count, int cap, int fin, int n_lm,
                                                         float* probs, float* offsets, float* landmarks) {
    const int e = blockIdx.x * THREADS + threadIdx.x;
    const int outs = 6 + n_lm, n = e / outs, j = e % outs;
    if (n >= min(*count, cap)) return;
    const float* x = hidden + (size_t)n * fin;
    const float* w1 = w;                              // (2, fin), bias 2
    const float* w2 = w1 + 2 * fin + 2;               // (4, fin), bias 4
    const float* w3 = w2 + 4 * fin + 4;               // (10, fin), bias 10
    auto dot = [&](const float* row, float bias) {
        float acc = bias;
        for (int i = 0; i < fin; ++i) acc = fmaf(x[i], row[i], acc);
        return acc;
    };
    if (j < 2) {
        const float o0 = dot(w1, w1[2 * fin]), o1 = dot(w1 + fin, w1[2 * fin + 1]);
        const float m = fmaxf(o0, o1), e0 = expf(o0 - m), e1 = expf(o1 - m);
        probs[(size_t)n * 2 + j] = (j == 0 ? e0 : e1) / (e0 + e1);
    } else if (j < 6) {
        offsets[(size_t)n * 4 + j - 2] = dot(w2 + (size_t)(j - 2) * fin, w2[4 * fin + j - 2]);
    } else {
        landmarks[(size_t)n * 10 + j - 6] = dot(w3 + (size_t)(j - 6) * fin, w3[10 * fin + j - 6]);
    }
}

int launched(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return APF_OK;
    snprintf(apf::err_buf(), 256, "%s: launch failed: %s", what, hipGetErrorString(e));
    return APF_ERR_LAUNCH;
}

unsigned blocks(long items) { return (unsigned)((items + THREADS - 1) / THREADS); }

}  // namespace

extern "C" {

int32_t apf_pnet_ok(const uint8_t* level, int32_t h, int32_t w, const float* params, const int32_t* cand_count) {
    return apf::check_pnet(level, h, w, params, cand_count) == APF_OK ? 1 : 0;
}

int apf_pnet(const uint8_t* level, int32_t h, int32_t w, const float* params, float threshold, float* prob, float* off, int32_t* cand_idx,
             float* cand_score, float* cand_off, int32_t* cand_count, void* stream) {
    const int rc = apf::check_pnet(level, h, w, params, cand_count);
    if (rc != APF_OK) return rc;
    if (!cand_idx || !cand_score || !cand_off) return fail(APF_ERR_INVALID, "pnet: null candidate arrays");
    const int mh = apf::pnet_map(h), mw = apf::pnet_map(w);
    (void)hipGetLastError();
    hipLaunchKernelGGL(pnet_kernel, dim3((mw + T - 1) / T, (mh + T - 1) / T), dim3(THREADS), 0, (hipStream_t)stream, level, h, w, params,
                       threshold, prob, off, cand_idx, cand_score, cand_off, cand_count);
    return launched("pnet");
}

int64_t apf_net_ws_bytes(int32_t net, int32_t cap) { return apf::net_ws_bytes(net, cap); }

int32_t apf_net_ok(int32_t net, const uint8_t* cuts, const int32_t* count, int32_t cap, const float* params, const void* ws,
                   const float* probs, const float* offsets, const float* landmarks) {
    return apf::check_net(net, cuts, count, cap, params, ws, probs, offsets, landmarks) == APF_OK ? 1 : 0;
}

int apf_net(int32_t net, const uint8_t* cuts, const int32_t* count, int32_t cap, const float* params, void* ws, float* probs,
            float* offsets, float* landmarks, void* stream) {
    const int rc = apf::check_net(net, cuts, count, cap, params, ws, probs, offsets, landmarks);
    if (rc != APF_OK) return rc;
    const apf::NetPlan p = apf::net_plan(net);
    float* buf[2] = {(float*)ws, (float*)ws + (size_t)cap * p.a_elems};
    hipStream_t st = (hipStream_t)stream;
    const float* par = params;
    const void* cur = cuts;
    (void)hipGetLastError();
    for (int i = 0; i < p.n_layers; ++i) {
        const apf::Layer& l = p.layers[i];
        float* dst = buf[i % 2];
        const long items = (long)cap * (l.pool ? l.cout : l.cout / 4) * l.out_side * l.out_side;
        if (l.pool) {
            hipLaunchKernelGGL(maxpool_kernel, dim3(blocks(items)), dim3(THREADS), 0, st, (const float*)cur, dst, count, cap, l.cout, l.k,
                               l.in_side, l.out_side);
        } else {
            const float* w = par;
            const float* b = w + (size_t)l.cout * l.cin * l.k * l.k;
            const float* a = b + l.cout;
            par = a + l.cout;
            if (i == 0)
                hipLaunchKernelGGL(conv_prelu_kernel<true>, dim3(blocks(items)), dim3(THREADS), 0, st, cur, dst, w, b, a, count, cap, l.cin,
                                   l.cout, l.k, l.in_side, l.out_side);
            else
                hipLaunchKernelGGL(conv_prelu_kernel<false>, dim3(blocks(items)), dim3(THREADS), 0, st, cur, dst, w, b, a, count, cap, l.cin,
                                   l.cout, l.k, l.in_side, l.out_side);
        }
        cur = dst;
    }
    const float* wt = par;
    const float* b = wt + (size_t)p.fc_in * p.fc_out;
    const float* a = b + p.fc_out;
    par = a + p.fc_out;
    hipLaunchKernelGGL(fc_prelu_kernel, dim3(blocks((long)cap * p.fc_out)), dim3(THREADS), 0, st, (const float*)cur, buf[1], wt, b, a, count,
                       cap, p.fc_in, p.fc_out);
    hipLaunchKernelGGL(heads_kernel, dim3(blocks((long)cap * (6 + p.n_lm))), dim3(THREADS), 0, st, (const float*)buf[1], par, count, cap,
                       p.fc_out, p.n_lm, probs, offsets, landmarks);
    return launched(net == APF_NET_R ? "rnet" : "onet");
}

}  // extern "C"
