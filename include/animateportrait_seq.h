/*
 * animateportrait_seq.h -- C ABI of libapseq.so: the batched LSTM forward of Module1's two landmark networks
 * (Module1/src/models/model_audio2landmark.py:41-55 and :312-318: 3-layer LSTMs with 256 hidden units over up to 512
 * windows of 18 frames) on the MI355X (gfx950).
 *
 * Like libapdata.so, libapstyle.so and libapface.so this library is NOT part of the model boundary
 * (include/animateportrait_amd.h, libapamd.so).  That one serves the batch-1 recurrence of the AutoVC converter
 * (ap_lstm_recurrence); this one serves whole batches of short sequences, where the batch rows are independent: a
 * workgroup owns 16 rows for the entire sequence, so there is no traffic between workgroups, no atomics, no workspace.
 *
 * Conventions: as in animateportrait_amd.h -- device pointers to contiguous fp32 tensors, caller-owned buffers, calls only
 * enqueue on `stream` (a hipStream_t as void*), 0 = ok, negative = error with a thread-local message (apq_last_error()).
 * A refused call launches nothing and writes nothing; apq_lstm_layer_fwd_ok needs no device.
 */
#ifndef ANIMATEPORTRAIT_SEQ_H
#define ANIMATEPORTRAIT_SEQ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define APQ_ABI_VERSION 1

enum { APQ_OK = 0, APQ_ERR_INVALID = -1, APQ_ERR_UNSUPPORTED = -2, APQ_ERR_LAUNCH = -3 };

/* served region of apq_lstm_layer_fwd */
#define APQ_LSTM_H 256          /* hidden units: the one size built */
#define APQ_MAX_B 1048576       /* batch rows (65536 workgroups of 16 rows) */
#define APQ_MAX_T 65536         /* time steps */
#define APQ_MAX_I 512           /* input features: a step's 16 x I input tile is staged twice in LDS */
#define APQ_MAX_ELEMS 0x7fffffffLL   /* elements of x and of out */
/* alignment in bytes: w_hh and out are moved 128 bits at a time; x, w_ih and the biases element by element unless w_ih and
 * I allow 128-bit loads (I % 4 == 0 and w_ih on a 16-byte boundary), which the call finds out by itself */
#define APQ_ALIGN_WIDE 16
#define APQ_ALIGN_ELEM 4

int32_t apq_abi_version(void);
const char* apq_last_error(void);

/* One unidirectional LSTM layer over whole sequences, zero initial state, fp32, PyTorch's gate order i, f, g, o:
 *   gates_t = W_ih x_t + b_ih + W_hh h_{t-1} + b_hh,   c_t = f c_{t-1} + i g,   h_t = o tanh(c_t)
 *   x     [B][T][I]
 *   w_ih  [4H][I],  w_hh [4H][H],  b_ih, b_hh [4H]
 *   out   [B][T][H], or with last_only != 0 [B][H] = h_{T-1}
 * The input projection runs inside the kernel (one product over K = I + H per step on the fp32 matrix pipe); nothing but
 * `out` is written.  One launch.
 * apq_lstm_layer_fwd_ok: 1 when apq_lstm_layer_fwd serves the call, else 0 with the reason in apq_last_error(); it launches
 * nothing and never dereferences a pointer.  apq_lstm_layer_fwd applies the same checks: APQ_ERR_INVALID for null pointers
 * and empty sizes, APQ_ERR_UNSUPPORTED for H != 256, sizes above the limits and misaligned pointers. */
int32_t apq_lstm_layer_fwd_ok(const float* x, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                              const float* out, int32_t B, int32_t T, int32_t I, int32_t H, int32_t last_only);
int apq_lstm_layer_fwd(const float* x, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, float* out,
                       int32_t B, int32_t T, int32_t I, int32_t H, int32_t last_only, void* stream);

#ifdef __cplusplus
}
#endif

#endif
