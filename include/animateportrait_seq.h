/*
 * animateportrait_seq.h -- C ABI of libapseq.so: the batched LSTM forward of Module1's two landmark networks
 * (Module1/src/models/model_audio2landmark.py:41-55 and :312-318: 3-layer LSTMs with 256 hidden units over up to 512
 * windows of 18 frames) on the MI355X (gfx950), the training pair of that layer (a forward that keeps its gates, and the
 * reverse-time recurrence: Module1/src/approaches/train_content.py), and the clip-level post-processing of their landmark sequence
 * (train_audio2landmark.py:101-141, 235-309, 594-617 and main_end2end_module2.py:262-272): Savitzky-Golay smoothing,
 * baseline calibration, segment assembly with the inverted-lip fix, the image transform with the eye lids.
 *
 * Like libapdata.so, libapstyle.so and libapface.so this library is NOT part of the model boundary
 * (include/animateportrait_amd.h, libapamd.so).  That one serves the batch-1 recurrence of the AutoVC converter
 * (ap_lstm_recurrence); this one serves whole batches of short sequences, where the batch rows are independent: a
 * workgroup owns 16 rows for the entire sequence, so there is no traffic between workgroups, no atomics, no workspace.
 *
 * Conventions: as in animateportrait_amd.h -- device pointers to contiguous fp32 tensors, caller-owned buffers, calls only
 * enqueue on `stream` (a hipStream_t as void*), 0 = ok, negative = error with a thread-local message (apq_last_error()).
 * A refused call launches nothing and writes nothing; every launching call has a twin `<name>_ok` that needs no device.
 * The post-processing entry points were added without a change of APQ_ABI_VERSION: nothing that existed changed; so were the
 * clip's f0 track, the two ends of its speaker embedding, its audio front end and the two launches per layer of the pose
 * network's self-attention encoder (further down).
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

/* ------------------------------------------------------------- training the same layer (seq_lstm_train.hip)
 * One launch each, a workgroup per 16 batch rows as above: no atomics, no workspace, no traffic between workgroups.  Served:
 * H = 256 and the APQ_MAX_* limits of apq_lstm_layer_fwd; gates / dgates of B T 4H elements below 2^31; x, w_ih and the biases
 * aligned as there, every other tensor to 16 bytes (APQ_ALIGN_WIDE).  The `_ok` twins and the error codes follow the rules of
 * apq_lstm_layer_fwd_ok.  Added without a change of APQ_ABI_VERSION: nothing that existed changed.
 *
 * apq_lstm_layer_fwd_train: apq_lstm_layer_fwd with last_only = 0 that also writes, per step, the activated gates
 *   gates [B][T][4H]  (i, f, g, o: sigmoid, sigmoid, tanh, sigmoid of the four H-wide blocks)  and  cell [B][T][H] = c_t.
 * `out` has the bits apq_lstm_layer_fwd writes: the same products in the same order, the same gate functions. */
int32_t apq_lstm_layer_fwd_train_ok(const float* x, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                                    const float* out, const float* gates, const float* cell, int32_t B, int32_t T, int32_t I,
                                    int32_t H);
int apq_lstm_layer_fwd_train(const float* x, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, float* out,
                             float* gates, float* cell, int32_t B, int32_t T, int32_t I, int32_t H, void* stream);

/* The reverse-time recurrence of that layer: from the gradient of its output to the gradient of its pre-activation gates,
 *   dout    [B][T][H], or with last_only != 0 [B][H]: the gradient of h_{T-1}, every other step's being zero
 *   gates, cell       what apq_lstm_layer_fwd_train wrote
 *   w_hh_t  [H][4H]   the transpose of w_hh, made by the caller
 *   dgates  [B][T][4H]  dG_t, gate order i, f, g, o
 * per step, t = T - 1 .. 0, with dh_rec = dc_carry = 0 at the start and c_{-1} = 0:
 *   dh = dout_t + dh_rec,  do = dh tanh(c_t) o (1 - o),  dc = dh o (1 - tanh^2 c_t) + dc_carry,  di = dc g i (1 - i),
 *   df = dc c_{t-1} f (1 - f),  dg = dc i (1 - g^2),  dc_carry = dc f,  dh_rec = dG_t w_hh
 * (dh_rec: one product over K = 4H per step on the fp32 matrix pipe, the 16 x 4H tile of dG_t staged in LDS.)  The
 * time-parallel products are the caller's GEMMs over the B T rows of dgates: dx = dG w_ih, dw_ih = dG^T x, dw_hh = dG^T h_{t-1},
 * db_ih = db_hh = the column sums.  The order of every sum is the same for every row and launch. */
int32_t apq_lstm_layer_bwd_ok(const float* dout, const float* gates, const float* cell, const float* w_hh_t, const float* dgates,
                              int32_t B, int32_t T, int32_t H, int32_t last_only);
int apq_lstm_layer_bwd(const float* dout, const float* gates, const float* cell, const float* w_hh_t, float* dgates, int32_t B,
                       int32_t T, int32_t H, int32_t last_only, void* stream);

/* ---------------------------------------------------------------- clip-level landmark post-processing (seq_post.hip)
 * A landmark sequence is [T][204] fp32: 68 points x (x, y, z) per frame.  No call uses atomics, a workspace or a host
 * synchronisation; all need 4-byte aligned pointers (APQ_ALIGN_ELEM).  Each `_ok` twin takes the launching call's
 * arguments without the stream and returns 1 when the call is served, else 0 with the reason in apq_last_error(); it
 * launches nothing and never dereferences a pointer.  The launching calls apply the same checks: APQ_ERR_INVALID for
 * null pointers and empty or inconsistent sizes, APQ_ERR_UNSUPPORTED for sizes outside the served region and misaligned
 * pointers. */
#define APQ_LM_C 204            /* coordinates of a frame */
#define APQ_SG_MIN_W 5          /* Savitzky-Golay window: odd, 5 .. 31, at most T */
#define APQ_SG_MAX_W 31
#define APQ_SEG_MAX_T 512       /* frames of a segment (apq_calib_baseline, apq_segment_assemble) */
#define APQ_MAX_STAMPS 4096     /* blink stamps of apq_image_landmarks */

/* Savitzky-Golay of order 3 along time on x [T][C] into y [T][C] (out of place), edges as scipy's mode='interp'.
 * Columns [c0, c1) are filtered with window W0, columns [c1, c2) with W1; every other column of y stays untouched, and an
 * empty range ignores its window and table.  0 <= c0 <= c1 <= c2 <= C.
 * taps [(W / 2 + 1)][W]: row i < W / 2 gives output row i from the first W samples, x[0] first, and output row T - 1 - i
 * from the last W samples, x[T - 1] first; row W / 2 holds the interior taps, x[t - W / 2] first.  (The rows are rows of the
 * projector on cubics over W equidistant samples, which is symmetric under reversal of both indices.) */
int32_t apq_savgol_ok(const float* x, const float* y, const float* taps0, const float* taps1, int32_t T, int32_t C,
                      int32_t c0, int32_t c1, int32_t c2, int32_t W0, int32_t W1);
int apq_savgol(const float* x, float* y, const float* taps0, const float* taps1, int32_t T, int32_t C, int32_t c0, int32_t c1,
               int32_t c2, int32_t W0, int32_t W1, void* stream);

/* __calib_baseline_pred_fls__ on x [T][204] into y [T][204] (out of place): per column subtract the mean of its k smallest
 * values, then multiply the mouth's x columns (144, 147, ...) by amp_x and its y columns (145, 148, ...) by amp_y.
 * 2 <= T <= APQ_SEG_MAX_T, 1 <= k < T.  Only the sum of the k smallest is used, so ties do not matter. */
int32_t apq_calib_baseline_ok(const float* x, const float* y, int32_t T, int32_t k, float amp_x, float amp_y);
int apq_calib_baseline(const float* x, float* y, int32_t T, int32_t k, float amp_x, float amp_y, void* stream);

/* One segment, in [T][204] -> out [T][204] (out of place), 1 <= T <= APQ_SEG_MAX_T; `flags` selects the steps, in this order:
 *   APQ_SEG_CLOSE  close_pose_branch_mouth(in, ratio), then x amp, then + base [T][204] + fid [204] when both are given
 *                  (base and fid: both or neither);
 *   APQ_SEG_LIP    __solve_inverse_lip2__: the frames whose inner-lip polygon (points 60..67) has a negative area get
 *                  their inner lip closed and their outer-lip y moved along with the frame before, which is already fixed;
 *   APQ_SEG_NOSE   point 27 = 2 x point 28 - point 29.
 * All in fp32 in the operation order of the numpy statements (no fused multiply-add). */
#define APQ_SEG_CLOSE 1
#define APQ_SEG_LIP 2
#define APQ_SEG_NOSE 4
int32_t apq_segment_assemble_ok(const float* in, const float* base, const float* fid, const float* out, int32_t T, double ratio,
                                float amp, int32_t flags);
int apq_segment_assemble(const float* in, const float* base, const float* fid, float* out, int32_t T, double ratio, float amp,
                         int32_t flags, void* stream);

/* main_end2end_module2.py:262-266 on in [T][204] -> out [T][204] (out of place), 1 <= T <= APQ_MAX_T:
 *   APQ_IMG_TRANSFORM  x, y -> -x / scale - shift_x, -y / scale - shift_y (z untouched);
 *   APQ_IMG_EYES       add_naive_eye: the 0.95 / 0.05 lid mix on every frame, then a blink at each of the n_stamps frames in
 *                      stamps (int32, device).  A blink at t rewrites the frames t - 9 .. t + 14 from t - 10, t and t + 15,
 *                      so the call asks for T >= 46 and 1 <= n_stamps <= APQ_MAX_STAMPS; the stamps must be at least 25 apart
 *                      and in [10, T - 16], which the call cannot check: frames outside the sequence are never read (their
 *                      index is clamped), but such a blink is not the reference's.
 * Without APQ_IMG_EYES stamps may be null. */
#define APQ_IMG_TRANSFORM 1
#define APQ_IMG_EYES 2
int32_t apq_image_landmarks_ok(const float* in, const float* out, const int32_t* stamps, int32_t n_stamps, int32_t T, double scale,
                               double shift_x, double shift_y, int32_t flags);
int apq_image_landmarks(const float* in, float* out, const int32_t* stamps, int32_t n_stamps, int32_t T, double scale,
                        double shift_x, double shift_y, int32_t flags, void* stream);

/* ------------------------------------------------------------------- rigid registration of landmark frames (seq_register.hip)
 * Module1/util/icp.py on the 9-point "T shape" (points 27, 28, 29, 30, 33, 36, 39, 42, 45) of every frame, and its three uses
 * (train_content.py:176-183, train_audio2landmark.py:312-338), as tests/register_reference.py states them in float64:
 *   in [T][204] fp32, std [204] fp32  ->  out [T][204] fp32,  pose [T][12] fp64 or null
 * Per frame, in this order:
 *   APQ_REG_CENTER    p <- p - mean_68(p) + mean_68(std)
 *   T = icp(frame's T shape, std's T shape): correspondences by index, at most 50 rounds of the best rigid fit (Kabsch through
 *       a 3x3 SVD whose smallest direction is the one mirrored when the fit would reflect), stopped when the summed squared
 *       distance moves by less than 1e-4 between rounds; then the fit of the frame's own T shape onto the moved one.
 *       pose, when given, receives that frame's row-major 3x4 [R | t], before any angle is removed
 *   APQ_REG_NO_X_ROT  with R = Rz(c) Ry(b) Rx(a): p <- Rz(c) Ry(b) (p - t) + t   (the reference's switch no_y_rotation)
 *   APQ_REG_REGISTER  p <- R p + t   (excludes the two flags above)
 * flags == 0 copies the rows (and still fills pose).  Rows are fp32 in and out, everything between is fp64, rounded once at the
 * store.  One launch of T waves, a wave per frame: no workspace, no atomics, no host synchronisation; a frame's result does not
 * depend on its place in the clip or on T.  A degenerate frame (T-shape covariance of rank below 2, NaN, |b| within 1e-6 of 90
 * degrees) gets unspecified values in its own rows and nothing else.  out may be in itself (exactly in place), no other overlap
 * of out or pose with in, std or each other.  1 <= T <= APQ_MAX_T; in, std, out 4-byte aligned (APQ_ALIGN_ELEM), pose 8-byte
 * aligned (APQ_ALIGN_F64).  The `_ok` twin and the error codes follow the rules of the post-processing calls above.  Added
 * without a change of APQ_ABI_VERSION: nothing that existed changed. */
#define APQ_REG_CENTER 1
#define APQ_REG_NO_X_ROT 2
#define APQ_REG_REGISTER 4
#define APQ_REG_MAX_ROUNDS 50   /* icp's max_iterations */
int32_t apq_rigid_register_ok(const float* in, const float* std, const float* out, const double* pose, int32_t T, int32_t flags);
int apq_rigid_register(const float* in, const float* std, float* out, double* pose, int32_t T, int32_t flags, void* stream);

/* ------------------------------------------------------------------------------- the clip's f0 track (seq_f0.hip)
 * RAPT (Talkin 1995, the get_f0 defaults) with one NCCF pass at the full rate, as tests/f0_reference.py states it in float64:
 * apq_f0_candidates makes every frame's table (one workgroup per frame, no frame reads another's results), apq_f0_track runs
 * the dynamic programme, the backtrack and speaker_normalization in one workgroup.  One launch each, no atomics, no host
 * synchronisation, no workspace beyond the caller's tensors below; 4-byte aligned pointers (APQ_ALIGN_ELEM; the byte tensors
 * need none).  The `_ok` twins and the error codes follow the rules of the post-processing calls above.  Added without a change
 * of APQ_ABI_VERSION: nothing that existed changed. */
#define APQ_F0_HOP 256          /* samples between frames: frame t is centred on sample 256 t */
#define APQ_F0_CANDS 19         /* voiced hypotheses kept per frame */
#define APQ_F0_STATES 20        /* ... plus the unvoiced one */
#define APQ_F0_MIN_LAG 2        /* kmin >= 2 (phi is evaluated from kmin - 1 on) */
#define APQ_F0_MAX_LAG 320      /* kmax <= 320 (16 kHz / 50 Hz) */
#define APQ_F0_UNVOICED 255     /* path entry of an unvoiced frame */

/* x [L]: the signal on the 16-bit scale (float32(wav) * 32768), L >= 1, any length; frames t = 0 .. T - 1, 1 <= T <= APQ_MAX_T
 * (the mel's frame count is L / 256 + 1; samples outside [0, L) read as zero, so a frame may lie wholly past the signal).
 * APQ_F0_MIN_LAG <= kmin <= kmax <= APQ_F0_MAX_LAG.  Written per frame:
 *   count [T] int32        candidates kept, 0 .. 19
 *   lag, val [T][19]       their refined lags (samples, ascending) and NCCF values; zero behind count
 *   rr [T], s [T]          the rms ratio and the spectral stationarity term of the transition costs (frame 0: 1, 1) */
int32_t apq_f0_candidates_ok(const float* x, int32_t L, int32_t T, int32_t kmin, int32_t kmax, const int32_t* count,
                             const float* lag, const float* val, const float* rr, const float* s);
int apq_f0_candidates(const float* x, int32_t L, int32_t T, int32_t kmin, int32_t kmax, int32_t* count, float* lag, float* val,
                      float* rr, float* s, void* stream);

/* The dynamic programme over the tables of apq_f0_candidates (a count outside 0 .. 19 is clamped), fs > 0 the sample rate:
 *   back [T][20] uint8     best predecessor state of every state (states: the candidates, then the unvoiced hypothesis)
 *   path [T] uint8         the chosen candidate of every frame, APQ_F0_UNVOICED where unvoiced
 *   f0 [T]                 f0_norm: (clip((ln(fs / lag) - mean) / std / 4, -1, 1) + 1) / 2 on voiced frames, -1e10 on unvoiced
 *                          ones; no voiced frame: all -1e10; std = 0: voiced frames get 0.5 */
int32_t apq_f0_track_ok(const int32_t* count, const float* lag, const float* val, const float* rr, const float* s, int32_t T,
                        int32_t kmax, double fs, const uint8_t* back, const uint8_t* path, const float* f0);
int apq_f0_track(const int32_t* count, const float* lag, const float* val, const float* rr, const float* s, int32_t T,
                 int32_t kmax, double fs, uint8_t* back, uint8_t* path, float* f0, void* stream);

/* ------------------------------------------------------------------------- the clip's speaker embedding (seq_speaker.hip)
 * The two ends of resemblyzer's VoiceEncoder as tests/speaker_reference.py states them in float64; its three LSTM layers of 256
 * hidden units lie between them (apq_lstm_layer_fwd or the library's).  One launch each, no atomics, no workspace, no host
 * synchronisation.  The `_ok` twins and the error codes follow the rules of the post-processing calls above.  Added without a
 * change of APQ_ABI_VERSION: nothing that existed changed. */
#define APQ_MEL_MIN_FFT 16      /* n_fft: even, 16 .. 1024, a power of two or not */
#define APQ_MEL_MAX_FFT 1024
#define APQ_MEL_MAX_MELS 128    /* rows of the filter bank */
#define APQ_ALIGN_F64 8         /* alignment in bytes of the fp64 window */
#define APQ_SPK_E 256           /* width of the embedding (= APQ_LSTM_H) */
#define APQ_SPK_MAX_B 4096      /* windows of an utterance */

/* Mel frames of a centred short-time Fourier transform:
 *   x [L] fp32 samples, window [n_fft] fp64, basis [n_mels][n_fft / 2 + 1] fp32  ->  out [T][n_mels] fp32, T = L / hop + 1
 * Frame t is the n_fft samples centred on sample t hop of the reflect-padded signal (numpy's 'reflect': the edge sample is not
 * repeated; n_fft / 2 samples on each side).  Per frame: times window, the DFT bins 0 .. n_fft / 2, |X|^power (power 1 or 2),
 * times basis.  All of it is carried in fp64 and rounded to fp32 once, at the store.
 * Served: n_fft even in [APQ_MEL_MIN_FFT, APQ_MEL_MAX_FFT], 1 <= hop <= n_fft, 1 <= n_mels <= APQ_MEL_MAX_MELS,
 * L > n_fft / 2 (one reflection reaches every sample a frame reads), T <= APQ_MAX_T.  x, basis and out 4-byte aligned
 * (APQ_ALIGN_ELEM), window 8-byte aligned (APQ_ALIGN_F64). */
int32_t apq_mel_frames_ok(const float* x, const double* window, const float* basis, const float* out, int32_t L, int32_t n_fft,
                          int32_t hop, int32_t n_mels, int32_t power);
int apq_mel_frames(const float* x, const double* window, const float* basis, float* out, int32_t L, int32_t n_fft, int32_t hop,
                   int32_t n_mels, int32_t power, void* stream);

/* The encoder's head on h [B][256], the last LSTM layer's h_{T-1} of every window; w [256][256] (rows = outputs), b [256]:
 *   partial [B][256]  relu(w h + b) divided by its L2 norm, per row
 *   embed [256]       the mean of the partial rows divided by its L2 norm
 * The products are fp32 (four runs of 64 fused multiply-adds per output, added as (0 + 1) + (2 + 3), then + b); the norms and the
 * mean are accumulated in fp64 in a fixed order (the mean over the unrounded quotients, row 0 first), so the result does not
 * depend on scheduling.  A row whose ReLU output is all zero stays zero and still counts in the mean; when every row is zero,
 * embed is zero (the reference's arithmetic gives 0 / 0 in both places).  1 <= B <= APQ_SPK_MAX_B; 4-byte aligned pointers. */
int32_t apq_speaker_head_ok(const float* h, const float* w, const float* b, const float* partial, const float* embed, int32_t B);
int apq_speaker_head(const float* h, const float* w, const float* b, float* partial, float* embed, int32_t B, void* stream);

/* ------------------------------------------------------------------------------ the clip's audio front end (seq_audio.hip)
 * What lies between the decoded samples and the mel windows (animateportrait_amd/audio.py: resample_to_16k,
 * normalize_loudness, conditioned_signal, mel_spectrogram) on fp64 device tensors.  Each call is one launch, or two where the
 * text says so, on the caller's stream; no atomics, no kernel waits for another workgroup; workspaces are the caller's.  The
 * `_ok` twins and the error codes follow the rules of the post-processing calls above; fp64 tensors are 8-byte aligned
 * (APQ_ALIGN_F64).  Added without a change of APQ_ABI_VERSION: nothing that existed changed. */
#define APQ_RS_MAX_RATE 1024    /* up and down of apq_resample_poly, reduced by their common divisor by the caller */
#define APQ_RS_MAX_TAPS 16384   /* taps of its filter (scipy designs 20 max(up, down) + 1: rates up to 819) */
#define APQ_RS_MAX_C 2          /* channels */
#define APQ_RS_MAX_L 0x3fffffff /* input samples per channel */
#define APQ_LOUD_MAX_N 8388607  /* samples of all channels: N 2^30 < 2^53, so numpy's mean of the squares is exact too */
#define APQ_LOUD_MAX_BLOCKS 256 /* partial sums of apq_loudness_sumsq */
#define APQ_FF_MAX_M 8          /* order of apq_filtfilt's filter: b and a have M + 1 coefficients */
#define APQ_FF_MAX_L 0x3fffffc0 /* samples */
#define APQ_FF_TILE 1024        /* samples staged at a time */

/* scipy.signal.resample_poly(x, up, down, axis=0) with the filter h the caller designed (scipy's default: a Kaiser-5.0 firwin
 * of 20 max(up, down) + 1 taps, times up):
 *   x [L][C] fp64, h [N] fp64, N odd  ->  y [ceil(L up / down)][C] fp64
 * upfirdn's index arithmetic: the filter is delayed by down - (N / 2) % down zeros so that its centre falls on an output, the
 * signal is zero outside [0, L), the first (N / 2 + that delay) / down outputs are dropped.  One thread per output sample; the
 * taps of that sample's phase only, added in ascending tap order in fp64 (fused multiply-add). */
int32_t apq_resample_poly_ok(const double* x, const double* h, const double* y, int32_t L, int32_t C, int32_t N, int32_t up,
                             int32_t down);
int apq_resample_poly(const double* x, const double* h, double* y, int32_t L, int32_t C, int32_t N, int32_t up, int32_t down,
                      void* stream);

/* pydub's apply_gain on 16-bit samples in two halves (audio.normalize_loudness); x [N] fp64, all channels alike.
 * apq_loudness_sumsq: q = clip(rint(32768 x), -32768, 32767) (round half to even), *sum = the exact 64-bit integer sum of q^2.
 *   Two launches: partial sums of up to APQ_LOUD_MAX_BLOCKS workgroups into workspace (apq_loudness_workspace_bytes(N) bytes),
 *   then one workgroup adds them.  The caller reads the 8 bytes back and computes the gain.
 * apq_loudness_apply: y = floor(v) / 32768 with v = q gain, v > 32767 -> 32767, v < -32767 -> -32768 (audioop's fbound, then
 *   floor); with apply_gain == 0 (an rms of 0) y = q / 32768 and gain is ignored.  y may be x. */
int64_t apq_loudness_workspace_bytes(int32_t N);
int32_t apq_loudness_sumsq_ok(const double* x, const void* workspace, const int64_t* sum, int32_t N);
int apq_loudness_sumsq(const double* x, void* workspace, int64_t* sum, int32_t N, void* stream);
int32_t apq_loudness_apply_ok(const double* x, const double* y, int32_t N, double gain, int32_t apply_gain);
int apq_loudness_apply(const double* x, double* y, int32_t N, double gain, int32_t apply_gain, void* stream);

/* scipy.signal.filtfilt(b, a, x) with its defaults, one channel, fp64, out of place: x [L] -> y [L].  b, a [M + 1] and
 * zi [M] = lfilter_zi(b, a) are HOST arrays (they travel in the launch's arguments); 1 <= M <= APQ_FF_MAX_M, L > 3 (M + 1).
 * The signal is extended oddly by 3 (M + 1) samples at both ends, filtered forward from zi ext[0], the result filtered
 * backward from zi (its last sample), the extension dropped.  Every sample is lfilter's transposed direct form II step with
 * lfilter's own operation order and no fused multiply-add, one sample after the other, so the result has scipy's bits: the
 * recurrence is NOT evaluated in parallel (DESIGN.md 4e-4 says why a blocked scan cannot be).  One launch of one workgroup:
 * its lanes stage tiles of APQ_FF_TILE samples between memory and LDS while one lane runs the recurrence.
 * workspace: apq_filtfilt_workspace_bytes(L, M) bytes (the forward pass's output). */
int64_t apq_filtfilt_workspace_bytes(int32_t L, int32_t M);
int32_t apq_filtfilt_ok(const double* x, const double* y, const double* b, const double* a, const double* zi, const void* workspace,
                        int32_t L, int32_t M);
int apq_filtfilt(const double* x, double* y, const double* b, const double* a, const double* zi, void* workspace, int32_t L,
                 int32_t M, void* stream);

/* apq_mel_frames on fp64 samples with the reference's output map (audio.mel_spectrogram):
 *   out [T][n_mels] fp32 = (20 log10(max(1e-5, |STFT| basis)) - 16 + 100) / 100,   T = L / hop + 1
 * carried in fp64 and rounded to fp32 once, at the store.  Served as apq_mel_frames (power 1), x 8-byte aligned. */
int32_t apq_logmel_frames_ok(const double* x, const double* window, const float* basis, const float* out, int32_t L, int32_t n_fft,
                             int32_t hop, int32_t n_mels);
int apq_logmel_frames(const double* x, const double* window, const float* basis, float* out, int32_t L, int32_t n_fft, int32_t hop,
                      int32_t n_mels, void* stream);

/* ------------------------------------------------------- the pose network's self-attention encoder (seq_encoder.hip)
 * Encoder.forward of Module1/src/models/model_audio2landmark_speaker_aware.py (:195-209, its pieces :26-161) at inference, behind
 * the embedding and the positional term: per layer the two launches below, as tests/encoder_reference.py states them in float64.
 * Every product runs on the fp32 matrix pipe (v_mfma_f32_16x16x4_f32, exact fp32 products, K walked in chunks of four); a
 * workgroup owns 16 rows and talks to no other: no atomics, no spin, no workspace beyond q, k and v.  The weights keep nn.Linear's
 * layout [out][in]; nothing is packed or cached.  No mask, no dropout.  Every pointer is 16-byte aligned (APQ_ALIGN_WIDE).  The
 * `_ok` twins and the error codes follow the rules of apq_lstm_layer_fwd_ok.  Added without a change of APQ_ABI_VERSION:
 * nothing that existed changed. */
#define APQ_ENC_D 64            /* d_model: the one width built */
#define APQ_ENC_HEADS 2         /* heads of d_k = 32 */
#define APQ_ENC_ROWS 16         /* rows of a workgroup */
#define APQ_ENC_MAX_T 512       /* rows of a sequence (PositionalEncoder's table): a tile's 2 x 16 x T scores live in LDS */
#define APQ_ENC_FF_CHUNK 256    /* d_ff is walked in chunks of this many hidden units: d_ff is a multiple of it */
#define APQ_ENC_MAX_FF 8192     /* d_ff */

/* Norm_1 and the three projections of a layer for all B T rows, one launch of ceil(B T / 16) workgroups:
 *   n = alpha (x - mean) / (std + eps) + bias per row, std unbiased (divided by 63), eps added to the std
 *   q = n wq^T + bq,  k = n wk^T + bk,  v = n wv^T + bv
 *   x [B][T][64];  alpha, bias [64];  wq, wk, wv [64][64];  bq, bk, bv [64];  q, k, v [B][T][64] (the caller's workspace)
 * 1 <= T <= APQ_ENC_MAX_T, 1 <= B <= APQ_MAX_B, B T 64 below 2^31, d_model == APQ_ENC_D. */
int32_t apq_enc_qkv_ok(const float* x, const float* alpha, const float* bias, float eps, const float* wq, const float* bq,
                       const float* wk, const float* bk, const float* wv, const float* bv, const float* q, const float* k,
                       const float* v, int32_t B, int32_t T, int32_t d_model);
int apq_enc_qkv(const float* x, const float* alpha, const float* bias, float eps, const float* wq, const float* bq, const float* wk,
                const float* bk, const float* wv, const float* bv, float* q, float* k, float* v, int32_t B, int32_t T,
                int32_t d_model, void* stream);

/* The rest of EncoderLayer.forward, one launch of B ceil(T / 16) workgroups, each with 16 query rows of one sequence:
 *   per head h: p = softmax(q_h k_h^T / sqrt(32)) over the T keys of the row's own sequence (maximum subtracted first),
 *               c[:, 32 h : 32 h + 32] = p v_h                               (the heads side by side, head-major columns)
 *   x1 = x + (c wo^T + bo),   n = Norm_2(x1) with alpha2, bias2, eps2
 *   y  = x1 + (relu(n w1^T + b1) w2^T + b2)      (d_ff walked in chunks: the hidden activations stay in registers)
 *   with alpha_f and bias_f non-null (both or neither): y = Norm(y) with alpha_f, bias_f, eps_f -- the encoder's closing Norm
 *   x, q, k, v, y [B][T][64];  wo [64][64], bo [64];  w1 [d_ff][64], b1 [d_ff];  w2 [64][d_ff], b2 [64]
 * Keys at and beyond T are never read.  y may be x (a workgroup reads only its own rows of x).  Served as apq_enc_qkv, with
 * heads == APQ_ENC_HEADS and d_ff a multiple of APQ_ENC_FF_CHUNK up to APQ_ENC_MAX_FF.  The order of every sum is the same for
 * every row and launch: a sequence's result does not depend on its place in the batch. */
int32_t apq_enc_attn_ff_ok(const float* x, const float* q, const float* k, const float* v, const float* wo, const float* bo,
                           const float* alpha2, const float* bias2, float eps2, const float* w1, const float* b1, const float* w2,
                           const float* b2, const float* alpha_f, const float* bias_f, float eps_f, const float* y, int32_t B,
                           int32_t T, int32_t d_model, int32_t heads, int32_t d_ff);
int apq_enc_attn_ff(const float* x, const float* q, const float* k, const float* v, const float* wo, const float* bo,
                    const float* alpha2, const float* bias2, float eps2, const float* w1, const float* b1, const float* w2,
                    const float* b2, const float* alpha_f, const float* bias_f, float eps_f, float* y, int32_t B, int32_t T,
                    int32_t d_model, int32_t heads, int32_t d_ff, void* stream);

#ifdef __cplusplus
}
#endif

#endif
