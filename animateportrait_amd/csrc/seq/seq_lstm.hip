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

#include "seq_lstm_body.h"

namespace {

// grid: ceil(B / 16) workgroups of 512 threads; dynamic LDS: plan.lds_bytes
template <bool VEC>
__global__ __launch_bounds__(NT) void lstm_batched_kernel(const Params p) {
    constexpr bool TRAIN = false;
    float* const gates_out = nullptr;
    float* const cell_out = nullptr;
#include "seq_lstm_body_inl.h"
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
