// seq_lstm_train.hip -- the two training launches of one batched LSTM layer (include/animateportrait_seq.h:
// apq_lstm_layer_fwd_train, apq_lstm_layer_bwd), for Module1's content branch (Module1/src/approaches/train_content.py).
//
// Forward: the walk of seq_lstm.hip (seq_lstm_body.h) that also stores the activated gates and c_t of every step.
//
// Backward: the reverse-time recurrence, whose one output are the pre-activation gate gradients dG [B][T][4H]:
//   dh = dout_t + dh_rec,   do = dh tanh(c_t) o (1 - o),   dc = dh o (1 - tanh^2 c_t) + dc_carry
//   di = dc g i (1 - i),    df = dc c_{t-1} f (1 - f),     dg = dc i (1 - g^2),   dc_carry = dc f,   dh_rec = dG_t W_hh
// As in the forward a workgroup owns 16 batch rows for the entire sequence and talks to no other workgroup: no atomics, no
// workspace, no spin.  dh_rec is a product over K = 4H = 1024 on v_mfma_f32_16x16x4_f32 with
//   A (16 x 4)  = 16 rows of w_hh_t [H][4H] (the transposed W_hh)   lane l: unit l & 15, k-slot l >> 4, from global memory
//   B (4 x 16)  = dG_t of the 16 batch rows                        lane l: batch row l & 15, k-slot l >> 4, from LDS
//   D (16 x 16) : lane l holds batch row l & 15 and the four units 4 (l >> 4) + reg of the tile
// A wave owns 32 hidden units (two tiles), so dh_rec arrives in the lane that holds the same (row, units) of the saved
// gates: dh_rec and dc_carry live in registers and the gate math needs no exchange.  The dG tile [16][4H + pad] is staged in
// LDS (64.25 KiB) between the gate math and the product; the gates, cell rows and dout of step t - 1 are fetched into
// registers under step t's products.  K is walked in chunks of 16 as in the forward (k = 16 chunk + 4 slot + m: one 128-bit
// load per operand and chunk); even and odd chunks go to two accumulators per tile, added once at the end, so the order of
// every sum is fixed: a row's result does not depend on its place in the batch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "seq_lstm_body.h"
#include "seq_lstm_train_checks.h"

namespace {

constexpr int G4 = 4 * H;                            // gate values of a (row, step)
constexpr int DS = apq::kDgStride;                   // floats of a dG row in LDS
constexpr int KCHUNKS = G4 / 16;

struct TrainParams {
    Params p;
    float *gates, *cell;
};

template <bool VEC>
__global__ __launch_bounds__(NT) void lstm_batched_train_kernel(const TrainParams tp) {
    constexpr bool TRAIN = true;
    const Params& p = tp.p;
    float* const gates_out = tp.gates;
    float* const cell_out = tp.cell;
#include "seq_lstm_body_inl.h"
}

struct BwdParams {
    const float *dout, *gates, *cell, *w_hh_t;
    float* dgates;
    int B, T, last_only;
};

__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float at(const float4& v, int j) { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }

// grid: ceil(B / 16) workgroups of 512 threads; dynamic LDS: 16 (4H + pad) floats
__global__ __launch_bounds__(NT) void lstm_batched_bwd_kernel(const BwdParams p) {
    extern __shared__ float4 lds4[];
    float* const dgs = reinterpret_cast<float*>(lds4);      // [16][DS]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int u0 = wave * 32;
    const long long b0 = (long long)blockIdx.x * ROWS;
    const int T = p.T;
    const bool row_ok = b0 + r < p.B;
    const long long brow = b0 + r;                   // (dereferenced only where row_ok)

    // what the gate math of one step reads, for this lane's (row, units u0 + 16 ut + 4 g + reg); rows past the batch read zeros
    struct Step {
        float4 gt[2][4], c[2], dout[2];
    };
    auto load_gates = [&](int t, Step& s) {
#pragma unroll
        for (int ut = 0; ut < 2; ++ut) {
            const int unit = u0 + 16 * ut + 4 * g;
            const long long bt = brow * T + t;
#pragma unroll
            for (int gate = 0; gate < 4; ++gate)
                s.gt[ut][gate] = row_ok ? *reinterpret_cast<const float4*>(p.gates + bt * G4 + gate * H + unit) : zero4();
            if (p.last_only)
                s.dout[ut] = (row_ok && t + 1 == T) ? *reinterpret_cast<const float4*>(p.dout + brow * H + unit) : zero4();
            else
                s.dout[ut] = row_ok ? *reinterpret_cast<const float4*>(p.dout + bt * H + unit) : zero4();
        }
    };
    // c_t of step t; t = -1 is the zero initial state
    auto load_cell = [&](int t, float4 (&c)[2]) {
#pragma unroll
        for (int ut = 0; ut < 2; ++ut) {
            const int unit = u0 + 16 * ut + 4 * g;
            c[ut] = (row_ok && t >= 0) ? *reinterpret_cast<const float4*>(p.cell + (brow * T + t) * H + unit) : zero4();
        }
    };

    Step cur, nxt;
    float4 cprev[2];                                 // c_{t-1}
    load_gates(T - 1, cur);
    load_cell(T - 1, cur.c);
    load_cell(T - 2, cprev);
    float dhr[2][4], dcc[2][4];
#pragma unroll
    for (int ut = 0; ut < 2; ++ut)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) dhr[ut][reg] = dcc[ut][reg] = 0.f;

    const float* const wa = p.w_hh_t + (long long)(u0 + r) * G4 + 4 * g;       // tile ut: + 16 ut G4; chunk q: + 16 q
    const float* const bb = dgs + r * DS + 4 * g;

    for (int t = T - 1; t >= 0; --t) {
        // ---- gate math: dG_t of this lane's (row, units) to memory and to the LDS tile
#pragma unroll
        for (int ut = 0; ut < 2; ++ut) {
            float dgv[4][4];
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const float gi = at(cur.gt[ut][0], reg), gf = at(cur.gt[ut][1], reg), gg = at(cur.gt[ut][2], reg), go = at(cur.gt[ut][3], reg);
                const float tc = apq::tanhf_(at(cur.c[ut], reg));
                const float dh = at(cur.dout[ut], reg) + dhr[ut][reg];
                const float dc = dh * go * (1.f - tc * tc) + dcc[ut][reg];
                dgv[0][reg] = dc * gg * (gi * (1.f - gi));
                dgv[1][reg] = dc * at(cprev[ut], reg) * (gf * (1.f - gf));
                dgv[2][reg] = dc * gi * (1.f - gg * gg);
                dgv[3][reg] = dh * tc * (go * (1.f - go));
                dcc[ut][reg] = dc * gf;
            }
            const int unit = u0 + 16 * ut + 4 * g;
#pragma unroll
            for (int gate = 0; gate < 4; ++gate) {
                const float4 v = make_float4(dgv[gate][0], dgv[gate][1], dgv[gate][2], dgv[gate][3]);
                *reinterpret_cast<float4*>(dgs + r * DS + gate * H + unit) = v;
                if (row_ok) *reinterpret_cast<float4*>(p.dgates + (brow * T + t) * G4 + gate * H + unit) = v;
            }
        }
        if (t == 0) break;                           // (uniform) nothing reads dh_rec of step 0
        __syncthreads();                             // the dG tile is complete

        // ---- step t - 1's inputs land under the products
        load_gates(t - 1, nxt);
        load_cell(t - 2, nxt.c);                     // becomes c_{t-2} = the next step's c_{t-1}

        // ---- dh_rec = dG_t W_hh: 64 chunks of K, the fragments of chunk q + 1 in flight while chunk q multiplies
        f32x4 acc[2][2];
#pragma unroll
        for (int ut = 0; ut < 2; ++ut)
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) acc[ut][h2][reg] = 0.f;
        auto load_a = [&](int q, float4 (&a)[2]) {
#pragma unroll
            for (int ut = 0; ut < 2; ++ut) a[ut] = *reinterpret_cast<const float4*>(wa + (long long)(16 * ut) * G4 + 16 * q);
        };
        auto mma = [&](int q, int h2, const float4 (&a)[2]) {
            const float4 b = *reinterpret_cast<const float4*>(bb + 16 * q);
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int ut = 0; ut < 2; ++ut)
                    acc[ut][h2] = __builtin_amdgcn_mfma_f32_16x16x4f32(at(a[ut], m), at(b, m), acc[ut][h2], 0, 0, 0);
        };
        float4 a0[2], a1[2];
        load_a(0, a0);
        for (int q = 0; q < KCHUNKS; q += 2) {
            load_a(q + 1, a1);
            mma(q, 0, a0);
            if (q + 2 < KCHUNKS) load_a(q + 2, a0);
            mma(q + 1, 1, a1);
        }
#pragma unroll
        for (int ut = 0; ut < 2; ++ut)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) dhr[ut][reg] = acc[ut][0][reg] + acc[ut][1][reg];

        // ---- rotate: step t - 1 is next; its c_t is this step's c_{t-1}
#pragma unroll
        for (int ut = 0; ut < 2; ++ut) {
            const float4 c_tm1 = cprev[ut];
            cprev[ut] = nxt.c[ut];
            nxt.c[ut] = c_tm1;
        }
        cur = nxt;
        __syncthreads();                             // every wave has read the tile; step t - 1 may overwrite it
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

// a kernel gets 64 KiB of LDS without asking; both ask for what their largest plan needs
int allow_lds(const void* kernel, int bytes, const char* what) {
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) {
        snprintf(apq::err_buf(), 256, "%s: hipFuncSetAttribute: %s", what, hipGetErrorString(e));
        return APQ_ERR_LAUNCH;
    }
    (void)hipGetLastError();
    return APQ_OK;
}

template <bool VEC>
int launch_fwd_train(const TrainParams& tp, const apq::LstmPlan& pl, hipStream_t stream) {
    constexpr int kMaxLds = 2 * ROWS * (HS + (APQ_MAX_I + apq::kPad)) * (int)sizeof(float);
    const int rc = allow_lds(reinterpret_cast<const void*>(&lstm_batched_train_kernel<VEC>), kMaxLds, "lstm_layer_fwd_train");
    if (rc != APQ_OK) return rc;
    hipLaunchKernelGGL(lstm_batched_train_kernel<VEC>, dim3(pl.blocks), dim3(NT), pl.lds_bytes, stream, tp);
    return launched("lstm_layer_fwd_train");
}

}  // namespace

extern "C" {

int32_t apq_lstm_layer_fwd_train_ok(const float* x, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                                    const float* out, const float* gates, const float* cell, int32_t B, int32_t T, int32_t I,
                                    int32_t H_) {
    apq::LstmPlan pl;
    return apq::plan_lstm_layer_fwd_train(x, w_ih, w_hh, b_ih, b_hh, out, gates, cell, B, T, I, H_, &pl) == APQ_OK ? 1 : 0;
}

int apq_lstm_layer_fwd_train(const float* x, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, float* out,
                             float* gates, float* cell, int32_t B, int32_t T, int32_t I, int32_t H_, void* stream) {
    apq::LstmPlan pl;
    const int rc = apq::plan_lstm_layer_fwd_train(x, w_ih, w_hh, b_ih, b_hh, out, gates, cell, B, T, I, H_, &pl);
    if (rc != APQ_OK) return rc;
    TrainParams tp;
    tp.p.x = x; tp.p.w_ih = w_ih; tp.p.w_hh = w_hh; tp.p.b_ih = b_ih; tp.p.b_hh = b_hh; tp.p.out = out;
    tp.p.B = B; tp.p.T = T; tp.p.I = I; tp.p.xs = pl.xs; tp.p.last_only = 0;
    tp.gates = gates; tp.cell = cell;
    return pl.vec_ih ? launch_fwd_train<true>(tp, pl, (hipStream_t)stream) : launch_fwd_train<false>(tp, pl, (hipStream_t)stream);
}

int32_t apq_lstm_layer_bwd_ok(const float* dout, const float* gates, const float* cell, const float* w_hh_t, const float* dgates,
                              int32_t B, int32_t T, int32_t H_, int32_t last_only) {
    (void)last_only;
    apq::LstmBwdPlan pl;
    return apq::plan_lstm_layer_bwd(dout, gates, cell, w_hh_t, dgates, B, T, H_, &pl) == APQ_OK ? 1 : 0;
}

int apq_lstm_layer_bwd(const float* dout, const float* gates, const float* cell, const float* w_hh_t, float* dgates, int32_t B,
                       int32_t T, int32_t H_, int32_t last_only, void* stream) {
    apq::LstmBwdPlan pl;
    const int rc = apq::plan_lstm_layer_bwd(dout, gates, cell, w_hh_t, dgates, B, T, H_, &pl);
    if (rc != APQ_OK) return rc;
    const int rc2 = allow_lds(reinterpret_cast<const void*>(&lstm_batched_bwd_kernel), (int)pl.lds_bytes, "lstm_layer_bwd");
    if (rc2 != APQ_OK) return rc2;
    BwdParams p;
    p.dout = dout; p.gates = gates; p.cell = cell; p.w_hh_t = w_hh_t; p.dgates = dgates;
    p.B = B; p.T = T; p.last_only = last_only ? 1 : 0;
    hipLaunchKernelGGL(lstm_batched_bwd_kernel, dim3(pl.blocks), dim3(NT), pl.lds_bytes, (hipStream_t)stream, p);
    return launched("lstm_layer_bwd");
}

}  // extern "C"
