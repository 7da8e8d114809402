// seq_lstm.hip -- one LSTM layer (256 hidden units) over a whole BATCH of sequences as one launch
// (include/animateportrait_seq.h: apq_lstm_layer_fwd).  Module1's two landmark networks run 3-layer LSTMs over up to 512
// windows of 18 frames (Module1/src/models/model_audio2landmark.py:41-55, :312-318); through the library that is a few small
// kernels per time step and layer.
//
//   gates_t = [W_ih | W_hh] [x_t ; h_{t-1}] + b_ih + b_hh        one product over K = I + H per step, nothing precomputed
//   i, f, g, o = sigmoid, sigmoid, tanh, sigmoid of the four H-row blocks (PyTorch's gate order)
//   c_t = f c_{t-1} + i g,   h_t = o tanh(c_t)
//
// The batch rows are independent, so a workgroup owns 16 of them for the entire sequence and talks to no other workgroup:
// no atomics, no workspace, no spin.  The products run on the fp32 matrix pipe as v_mfma_f32_16x16x4_f32 with
//   A (16 x 4)  = 16 gate rows of W            lane l: row l & 15, k-slot l >> 4, straight from global memory (L2-resident)
//   B (4 x 16)  = [x_t ; h_{t-1}] of 16 rows   lane l: batch row l & 15, k-slot l >> 4, from LDS
//   D (16 x 16) : lane l holds batch row l & 15 and the four units 4 (l >> 4) + reg of the tile
// A wave owns 32 hidden units (two 16-unit tiles) for all four gates, so a lane finds i, f, g and o of one (unit, row) in
// the same slot of four accumulators and the gate math needs no exchange.  c lives in registers, h in LDS (two tiles, one
// barrier per step), x_{t+1} is fetched into registers under step t's products.
// K is walked in chunks of 16: k-slot s of matrix instruction m of a chunk is k = 16 chunk + 4 s + m, so that a lane's four
// A values (and its four B values) of a chunk are 16 contiguous bytes -- one 128-bit load each.  The order is the same for
// every row and every launch: a row's result does not depend on its place in the batch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "seq_checks.h"
#include "seq_math.h"

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int H = APQ_LSTM_H;
constexpr int HS = H + apq::kPad;                    // floats of an h row in LDS
constexpr int ROWS = apq::kRows;
constexpr int NT = apq::kThreads;
constexpr int XR = ROWS * APQ_MAX_I / NT;            // x values a thread carries from one step to the next (16)
static_assert(XR == 2 * (APQ_MAX_I / 64), "a wave moves two rows of the x tile");
constexpr int HCHUNKS = H / 16;

struct Params {
    const float *x, *w_ih, *w_hh, *b_ih, *b_hh;
    float* out;
    int B, T, I, xs, last_only;
};

// grid: ceil(B / 16) workgroups of 512 threads; dynamic LDS: plan.lds_bytes
template <bool VEC>
__global__ __launch_bounds__(NT) void lstm_batched_kernel(const Params p) {
    extern __shared__ float4 lds4[];
    float* const hs = reinterpret_cast<float*>(lds4);       // [2][16][HS]
    float* const xsb = hs + 2 * ROWS * HS;                  // [2][16][xs]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);          // (tells the compiler that it is uniform)
    const int r = lane & 15, g = lane >> 4;
    const int u0 = wave * 32;
    const long long b0 = (long long)blockIdx.x * ROWS;
    const int I = p.I, xs = p.xs, T = p.T;
    const int nci = (I + 15) / 16, nq = nci + HCHUNKS;
    const bool row_ok = b0 + r < p.B;

    // h_{-1} = 0, and the columns I .. 16 nci - 1 of both x tiles stay zero for the whole launch
    for (int e = tid; e < 2 * ROWS * (HS + xs); e += NT) hs[e] = 0.f;

    // x_t of the tile: wave w moves rows 2 w and 2 w + 1, a lane the columns lane + 64 j
    float xr[XR];
    auto load_x = [&](int t) {
#pragma unroll
        for (int j = 0; j < XR; ++j) {
            const int row = 2 * wave + j / (XR / 2), col = lane + 64 * (j % (XR / 2));
            const float* xrow = p.x + ((b0 + row) * T + t) * I;         // (uniform; dereferenced only for rows of the batch)
            xr[j] = (col < I && b0 + row < p.B) ? xrow[col] : 0.f;
        }
    };
    auto store_x = [&](int buf) {
#pragma unroll
        for (int j = 0; j < XR; ++j) {
            const int row = 2 * wave + j / (XR / 2), col = lane + 64 * (j % (XR / 2));
            if (col < I) xsb[(buf * ROWS + row) * xs + col] = xr[j];
        }
    };
    load_x(0);
    __syncthreads();
    store_x(0);

    // this lane's units: u0 + 16 ut + 4 g + reg
    float bias[2][4][4], c[2][4];
#pragma unroll
    for (int ut = 0; ut < 2; ++ut)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            c[ut][reg] = 0.f;
#pragma unroll
            for (int gate = 0; gate < 4; ++gate) {
                const int n = gate * H + u0 + 16 * ut + 4 * g + reg;
                bias[ut][gate][reg] = p.b_ih[n] + p.b_hh[n];
            }
        }
    __syncthreads();

    // A fragments of K chunk q: chunks 0 .. nci - 1 walk w_ih, the rest w_hh.  A tile's first row is uniform, the lane adds
    // (its row, its k): one set of offsets per chunk for all eight tiles.  Past the end of a w_ih row (the tail of the last
    // chunk) a lane re-reads the row's last element(s) instead: the x tile holds zeros there, so the product adds nothing.
    const unsigned off_hh = (unsigned)(r * H + 4 * g);
    auto load_a = [&](int q, float4 (&a)[2][4]) {
        if (q < nci) {
            const int k0 = 16 * q + 4 * g;
            unsigned o[4];
            if constexpr (VEC) {
                o[0] = (unsigned)(r * I + min(k0, I - 4));
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = (unsigned)(r * I + min(k0 + j, I - 1));
            }
#pragma unroll
            for (int ut = 0; ut < 2; ++ut)
#pragma unroll
                for (int gate = 0; gate < 4; ++gate) {
                    const float* w = p.w_ih + (long long)(gate * H + u0 + 16 * ut) * I;
                    if constexpr (VEC) a[ut][gate] = *reinterpret_cast<const float4*>(w + o[0]);
                    else a[ut][gate] = make_float4(w[o[0]], w[o[1]], w[o[2]], w[o[3]]);
                }
        } else {
#pragma unroll
            for (int ut = 0; ut < 2; ++ut)
#pragma unroll
                for (int gate = 0; gate < 4; ++gate) {
                    const float* w = p.w_hh + ((gate * H + u0 + 16 * ut) * H + 16 * (q - nci));
                    a[ut][gate] = *reinterpret_cast<const float4*>(w + off_hh);
                }
        }
    };

    for (int t = 0; t < T; ++t) {
        const int cur = t & 1, nxt = cur ^ 1;
        if (t + 1 < T) load_x(t + 1);                                   // (lands under the products)
        f32x4 acc[2][4];
#pragma unroll
        for (int ut = 0; ut < 2; ++ut)
#pragma unroll
            for (int gate = 0; gate < 4; ++gate)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) acc[ut][gate][reg] = bias[ut][gate][reg];
        const float* xb = xsb + (cur * ROWS + r) * xs + 4 * g;
        const float* hb = hs + (cur * ROWS + r) * HS + 4 * g;
        auto mma = [&](int q, const float4 (&a)[2][4]) {
            const float4 b = *reinterpret_cast<const float4*>(q < nci ? xb + 16 * q : hb + 16 * (q - nci));
            const float bm[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int ut = 0; ut < 2; ++ut)
#pragma unroll
                    for (int gate = 0; gate < 4; ++gate) {
                        const float am = m == 0 ? a[ut][gate].x : m == 1 ? a[ut][gate].y : m == 2 ? a[ut][gate].z : a[ut][gate].w;
                        acc[ut][gate] = __builtin_amdgcn_mfma_f32_16x16x4f32(am, bm[m], acc[ut][gate], 0, 0, 0);
                    }
        };
        // the fragments of chunk q + 1 are in flight while chunk q multiplies
        float4 a0[2][4], a1[2][4];
        load_a(0, a0);
        for (int q = 0; q < nq; q += 2) {
            if (q + 1 < nq) load_a(q + 1, a1);
            mma(q, a0);
            if (q + 1 < nq) {
                if (q + 2 < nq) load_a(q + 2, a0);
                mma(q + 1, a1);
            }
        }
        const bool write_out = row_ok && (!p.last_only || t + 1 == T);
#pragma unroll
        for (int ut = 0; ut < 2; ++ut) {
            float hv[4];
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const float gi = apq::sigmoidf_(acc[ut][0][reg]), gf = apq::sigmoidf_(acc[ut][1][reg]);
                const float gg = apq::tanhf_(acc[ut][2][reg]), go = apq::sigmoidf_(acc[ut][3][reg]);
                c[ut][reg] = gf * c[ut][reg] + gi * gg;
                hv[reg] = go * apq::tanhf_(c[ut][reg]);
            }
            const int unit = u0 + 16 * ut + 4 * g;
            const float4 h4 = make_float4(hv[0], hv[1], hv[2], hv[3]);
            *reinterpret_cast<float4*>(hs + (nxt * ROWS + r) * HS + unit) = h4;
            if (write_out) {
                const long long row = p.last_only ? b0 + r : (b0 + r) * T + t;
                *reinterpret_cast<float4*>(p.out + row * H + unit) = h4;
            }
        }
        if (t + 1 < T) store_x(nxt);
        __syncthreads();            // h_t and x_{t+1} are complete; the tiles of step t may be overwritten in step t + 1
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

template <bool VEC>
int launch(const Params& p, const apq::LstmPlan& pl, hipStream_t stream) {
    // the largest plan needs more than the 64 KiB a kernel gets without asking
    constexpr int kMaxLds = 2 * ROWS * (HS + (APQ_MAX_I + apq::kPad)) * (int)sizeof(float);
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&lstm_batched_kernel<VEC>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds);
    if (e != hipSuccess) {
        snprintf(apq::err_buf(), 256, "lstm_layer_fwd: hipFuncSetAttribute: %s", hipGetErrorString(e));
        return APQ_ERR_LAUNCH;
    }
    (void)hipGetLastError();
    hipLaunchKernelGGL(lstm_batched_kernel<VEC>, dim3(pl.blocks), dim3(NT), pl.lds_bytes, stream, p);
    return launched("lstm_layer_fwd");
}

}  // namespace

extern "C" {

int32_t apq_abi_version(void) { return APQ_ABI_VERSION; }
const char* apq_last_error(void) { return apq::err_buf(); }

int32_t apq_lstm_layer_fwd_ok(const float* x, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                              const float* out, int32_t B, int32_t T, int32_t I, int32_t H_, int32_t last_only) {
    (void)last_only;
    apq::LstmPlan pl;
    return apq::plan_lstm_layer_fwd(x, w_ih, w_hh, b_ih, b_hh, out, B, T, I, H_, &pl) == APQ_OK ? 1 : 0;
}

int apq_lstm_layer_fwd(const float* x, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, float* out,
                       int32_t B, int32_t T, int32_t I, int32_t H_, int32_t last_only, void* stream) {
    apq::LstmPlan pl;
    const int rc = apq::plan_lstm_layer_fwd(x, w_ih, w_hh, b_ih, b_hh, out, B, T, I, H_, &pl);
    if (rc != APQ_OK) return rc;
    Params p;
    p.x = x; p.w_ih = w_ih; p.w_hh = w_hh; p.b_ih = b_ih; p.b_hh = b_hh; p.out = out;
    p.B = B; p.T = T; p.I = I; p.xs = pl.xs; p.last_only = last_only ? 1 : 0;
    return pl.vec_ih ? launch<true>(p, pl, (hipStream_t)stream) : launch<false>(p, pl, (hipStream_t)stream);
}

}  // extern "C"
