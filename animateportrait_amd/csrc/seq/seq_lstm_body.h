// What the two batched LSTM forward kernels of libapseq.so share: apq_lstm_layer_fwd (seq_lstm.hip) and
// apq_lstm_layer_fwd_train (seq_lstm_train.hip) are the same walk, the second with two more stores per step.  The constants and
// the argument block are here; the statements of the kernel are seq_lstm_body_inl.h, which each kernel includes between its
// braces.  Everything here has internal linkage: each translation unit gets its own copy.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

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

}  // namespace
