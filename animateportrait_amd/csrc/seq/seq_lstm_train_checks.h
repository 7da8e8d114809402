// Host side of the training calls of libapseq.so that needs no device: the argument checks and launch plans of
// apq_lstm_layer_fwd_train and apq_lstm_layer_bwd.  Plain C++, like seq_checks.h, whose forward plan the first one extends.
#pragma once

#include "seq_checks.h"

namespace apq {

// the dG tile's row in LDS: the 4H gate gradients of a batch row, plus the pad
constexpr int kDgStride = 4 * APQ_LSTM_H + kPad;

struct LstmBwdPlan {
    int blocks;          // workgroups: ceil(B / 16)
    size_t lds_bytes;    // one dG tile [16][4H + pad]
};

inline int plan_lstm_layer_fwd_train(const void* x, const void* w_ih, const void* w_hh, const void* b_ih, const void* b_hh,
                                     const void* out, const void* gates, const void* cell, int B, int T, int I, int H, LstmPlan* pl) {
    if (!gates) return fail(APQ_ERR_INVALID, "lstm_layer_fwd_train: null gates");
    if (!cell) return fail(APQ_ERR_INVALID, "lstm_layer_fwd_train: null cell");
    const int rc = plan_lstm_layer_fwd(x, w_ih, w_hh, b_ih, b_hh, out, B, T, I, H, pl);
    if (rc != APQ_OK) return rc;
    const long long bt = (long long)B * T;
    if (bt * 4 * H > APQ_MAX_ELEMS)
        return fail(APQ_ERR_UNSUPPORTED, "lstm_layer_fwd_train: gates of B T 4H = %lld elements, served: below 2^31", bt * 4 * H);
    if (misaligned(gates, APQ_ALIGN_WIDE)) return fail(APQ_ERR_UNSUPPORTED, "lstm_layer_fwd_train: gates is not %lld-byte aligned", APQ_ALIGN_WIDE);
    if (misaligned(cell, APQ_ALIGN_WIDE)) return fail(APQ_ERR_UNSUPPORTED, "lstm_layer_fwd_train: cell is not %lld-byte aligned", APQ_ALIGN_WIDE);
    return APQ_OK;
}

inline int plan_lstm_layer_bwd(const void* dout, const void* gates, const void* cell, const void* w_hh_t, const void* dgates, int B, int T,
                               int H, LstmBwdPlan* pl) {
    if (!dout) return fail(APQ_ERR_INVALID, "lstm_layer_bwd: null dout");
    if (!gates) return fail(APQ_ERR_INVALID, "lstm_layer_bwd: null gates");
    if (!cell) return fail(APQ_ERR_INVALID, "lstm_layer_bwd: null cell");
    if (!w_hh_t) return fail(APQ_ERR_INVALID, "lstm_layer_bwd: null w_hh_t");
    if (!dgates) return fail(APQ_ERR_INVALID, "lstm_layer_bwd: null dgates");
    if (B < 1) return fail(APQ_ERR_INVALID, "lstm_layer_bwd: B = %lld (at least 1)", B);
    if (T < 1) return fail(APQ_ERR_INVALID, "lstm_layer_bwd: T = %lld (at least 1)", T);
    if (H != APQ_LSTM_H) return fail(APQ_ERR_UNSUPPORTED, "lstm_layer_bwd: H = %lld (built for H = %lld)", H, APQ_LSTM_H);
    if (B > APQ_MAX_B) return fail(APQ_ERR_UNSUPPORTED, "lstm_layer_bwd: B = %lld, served: up to %lld", B, APQ_MAX_B);
    if (T > APQ_MAX_T) return fail(APQ_ERR_UNSUPPORTED, "lstm_layer_bwd: T = %lld, served: up to %lld", T, APQ_MAX_T);
    const long long bt = (long long)B * T;
    if (bt * 4 * H > APQ_MAX_ELEMS)
        return fail(APQ_ERR_UNSUPPORTED, "lstm_layer_bwd: dgates of B T 4H = %lld elements, served: below 2^31", bt * 4 * H);
    if (misaligned(dout, APQ_ALIGN_WIDE)) return fail(APQ_ERR_UNSUPPORTED, "lstm_layer_bwd: dout is not %lld-byte aligned", APQ_ALIGN_WIDE);
    if (misaligned(gates, APQ_ALIGN_WIDE)) return fail(APQ_ERR_UNSUPPORTED, "lstm_layer_bwd: gates is not %lld-byte aligned", APQ_ALIGN_WIDE);
    if (misaligned(cell, APQ_ALIGN_WIDE)) return fail(APQ_ERR_UNSUPPORTED, "lstm_layer_bwd: cell is not %lld-byte aligned", APQ_ALIGN_WIDE);
    if (misaligned(w_hh_t, APQ_ALIGN_WIDE)) return fail(APQ_ERR_UNSUPPORTED, "lstm_layer_bwd: w_hh_t is not %lld-byte aligned", APQ_ALIGN_WIDE);
    if (misaligned(dgates, APQ_ALIGN_WIDE)) return fail(APQ_ERR_UNSUPPORTED, "lstm_layer_bwd: dgates is not %lld-byte aligned", APQ_ALIGN_WIDE);
    pl->blocks = (B + kRows - 1) / kRows;
    pl->lds_bytes = (size_t)kRows * kDgStride * sizeof(float);
    return APQ_OK;
}

}  // namespace apq
