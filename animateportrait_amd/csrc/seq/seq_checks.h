// Host side of libapseq.so that needs no device: the argument checks and the launch plan of apq_lstm_layer_fwd.  Plain C++, so
// that a stand-alone program can compile it with the host sanitisers.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../../include/animateportrait_seq.h"

namespace apq {

inline char* err_buf() {
    static thread_local char buf[256] = "";
    return buf;
}

// writes the message, returns `code`
inline int fail(int code, const char* fmt, long long a = 0, long long b = 0, long long c = 0) {
    snprintf(err_buf(), 256, fmt, a, b, c);
    return code;
}

constexpr int kRows = 16;        // batch rows of a workgroup (the N of the 16x16x4 matrix instruction)
constexpr int kThreads = 512;    // 8 waves, 32 hidden units each
constexpr int kPad = 4;          // floats behind an LDS row: consecutive rows start 4 banks apart

// the input tile's row in LDS: I rounded up to the K chunk of 16 (zero filled), plus the pad
inline int x_stride(int I) { return (I + 15) / 16 * 16 + kPad; }

struct LstmPlan {
    int blocks;          // workgroups: ceil(B / 16)
    int vec_ih;          // 1: rows of w_ih are read 128 bits at a time
    int xs;              // x_stride(I)
    size_t lds_bytes;    // two h tiles [16][H + pad] and two x tiles [16][xs]
};

inline bool misaligned(const void* p, int a) { return ((uintptr_t)p & (uintptr_t)(a - 1)) != 0; }

inline int plan_lstm_layer_fwd(const void* x, const void* w_ih, const void* w_hh, const void* b_ih, const void* b_hh, const void* out,
                               int B, int T, int I, int H, LstmPlan* pl) {
    if (!x) return fail(APQ_ERR_INVALID, "lstm_layer_fwd: null x");
    if (!w_ih) return fail(APQ_ERR_INVALID, "lstm_layer_fwd: null w_ih");
    if (!w_hh) return fail(APQ_ERR_INVALID, "lstm_layer_fwd: null w_hh");
    if (!b_ih) return fail(APQ_ERR_INVALID, "lstm_layer_fwd: null b_ih");
    if (!b_hh) return fail(APQ_ERR_INVALID, "lstm_layer_fwd: null b_hh");
    if (!out) return fail(APQ_ERR_INVALID, "lstm_layer_fwd: null out");
    if (B < 1) return fail(APQ_ERR_INVALID, "lstm_layer_fwd: B = %lld (at least 1)", B);
    if (T < 1) return fail(APQ_ERR_INVALID, "lstm_layer_fwd: T = %lld (at least 1)", T);
    if (I < 1) return fail(APQ_ERR_INVALID, "lstm_layer_fwd: I = %lld (at least 1)", I);
    if (H != APQ_LSTM_H) return fail(APQ_ERR_UNSUPPORTED, "lstm_layer_fwd: H = %lld (built for H = %lld)", H, APQ_LSTM_H);
    if (B > APQ_MAX_B) return fail(APQ_ERR_UNSUPPORTED, "lstm_layer_fwd: B = %lld, served: up to %lld", B, APQ_MAX_B);
    if (T > APQ_MAX_T) return fail(APQ_ERR_UNSUPPORTED, "lstm_layer_fwd: T = %lld, served: up to %lld", T, APQ_MAX_T);
    if (I > APQ_MAX_I) return fail(APQ_ERR_UNSUPPORTED, "lstm_layer_fwd: I = %lld, served: up to %lld", I, APQ_MAX_I);
    const long long bt = (long long)B * T;
    if (bt * I > APQ_MAX_ELEMS) return fail(APQ_ERR_UNSUPPORTED, "lstm_layer_fwd: x of B T I = %lld elements, served: below 2^31", bt * I);
    if (bt * H > APQ_MAX_ELEMS) return fail(APQ_ERR_UNSUPPORTED, "lstm_layer_fwd: out of B T H = %lld elements, served: below 2^31", bt * H);
    if (misaligned(x, APQ_ALIGN_ELEM)) return fail(APQ_ERR_UNSUPPORTED, "lstm_layer_fwd: x is not %lld-byte aligned", APQ_ALIGN_ELEM);
    if (misaligned(w_ih, APQ_ALIGN_ELEM)) return fail(APQ_ERR_UNSUPPORTED, "lstm_layer_fwd: w_ih is not %lld-byte aligned", APQ_ALIGN_ELEM);
    if (misaligned(b_ih, APQ_ALIGN_ELEM)) return fail(APQ_ERR_UNSUPPORTED, "lstm_layer_fwd: b_ih is not %lld-byte aligned", APQ_ALIGN_ELEM);
    if (misaligned(b_hh, APQ_ALIGN_ELEM)) return fail(APQ_ERR_UNSUPPORTED, "lstm_layer_fwd: b_hh is not %lld-byte aligned", APQ_ALIGN_ELEM);
    if (misaligned(w_hh, APQ_ALIGN_WIDE)) return fail(APQ_ERR_UNSUPPORTED, "lstm_layer_fwd: w_hh is not %lld-byte aligned", APQ_ALIGN_WIDE);
    if (misaligned(out, APQ_ALIGN_WIDE)) return fail(APQ_ERR_UNSUPPORTED, "lstm_layer_fwd: out is not %lld-byte aligned", APQ_ALIGN_WIDE);
    pl->blocks = (B + kRows - 1) / kRows;
    pl->vec_ih = (I % 4 == 0 && !misaligned(w_ih, APQ_ALIGN_WIDE)) ? 1 : 0;
    pl->xs = x_stride(I);
    pl->lds_bytes = (size_t)2 * kRows * (APQ_LSTM_H + kPad + pl->xs) * sizeof(float);
    return APQ_OK;
}

}  // namespace apq
