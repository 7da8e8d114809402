// Host side of the audio front end's calls of libapseq.so that needs no device: their argument checks and the sizes both sides
// share.  Plain C++ like seq_checks.h, so that a stand-alone program can compile it with the host sanitisers.
#pragma once

#include "seq_speaker_checks.h"

namespace apq {

constexpr int kRsThreads = 256;                       // resampler: a thread per output sample
constexpr int kLoudThreads = 256;                     // loudness: 4 waves a workgroup
constexpr int kLoudPerBlock = 1024;                   // ... samples a workgroup takes before another one is added
constexpr int kFfThreads = 256;                       // filtfilt: the one workgroup that stages the tiles
constexpr int kFfTile = APQ_FF_TILE;                  // ... samples of a tile

// ---------------------------------------------------------------------------------------------------------------- resampler
// scipy.signal.resample_poly's bookkeeping for a filter of N = 2 half + 1 taps
inline long long rs_out_len(long long L, int up, int down) { return (L * up + down - 1) / down; }
inline int rs_pre_pad(int N, int down) { return down - ((N - 1) / 2) % down; }
inline int rs_pre_remove(int N, int down) { return ((N - 1) / 2 + rs_pre_pad(N, down)) / down; }

inline int check_resample_poly(const void* x, const void* h, const void* y, int L, int C, int N, int up, int down) {
    if (!x) return fail(APQ_ERR_INVALID, "resample_poly: null x");
    if (!h) return fail(APQ_ERR_INVALID, "resample_poly: null h");
    if (!y) return fail(APQ_ERR_INVALID, "resample_poly: null y");
    if (L < 1) return fail(APQ_ERR_INVALID, "resample_poly: L = %lld (at least 1)", L);
    if (C < 1) return fail(APQ_ERR_INVALID, "resample_poly: C = %lld (at least 1)", C);
    if (N < 1) return fail(APQ_ERR_INVALID, "resample_poly: N = %lld taps (at least 1)", N);
    if (up < 1) return fail(APQ_ERR_INVALID, "resample_poly: up = %lld (at least 1)", up);
    if (down < 1) return fail(APQ_ERR_INVALID, "resample_poly: down = %lld (at least 1)", down);
    if (C > APQ_RS_MAX_C) return fail(APQ_ERR_UNSUPPORTED, "resample_poly: C = %lld, served: up to %lld", C, APQ_RS_MAX_C);
    if (up > APQ_RS_MAX_RATE) return fail(APQ_ERR_UNSUPPORTED, "resample_poly: up = %lld, served: up to %lld", up, APQ_RS_MAX_RATE);
    if (down > APQ_RS_MAX_RATE) return fail(APQ_ERR_UNSUPPORTED, "resample_poly: down = %lld, served: up to %lld", down, APQ_RS_MAX_RATE);
    if (N % 2 == 0) return fail(APQ_ERR_UNSUPPORTED, "resample_poly: N = %lld taps is even, served: odd (a centred filter)", N);
    if (N > APQ_RS_MAX_TAPS) return fail(APQ_ERR_UNSUPPORTED, "resample_poly: N = %lld taps, served: up to %lld", N, APQ_RS_MAX_TAPS);
    if (L > APQ_RS_MAX_L) return fail(APQ_ERR_UNSUPPORTED, "resample_poly: L = %lld, served: up to %lld", L, APQ_RS_MAX_L);
    if (rs_out_len(L, up, down) * C > APQ_MAX_ELEMS)
        return fail(APQ_ERR_UNSUPPORTED, "resample_poly: y of %lld elements, served: below 2^31", rs_out_len(L, up, down) * C);
    if (misaligned(x, APQ_ALIGN_F64)) return fail(APQ_ERR_UNSUPPORTED, "resample_poly: x is not %lld-byte aligned", APQ_ALIGN_F64);
    if (misaligned(h, APQ_ALIGN_F64)) return fail(APQ_ERR_UNSUPPORTED, "resample_poly: h is not %lld-byte aligned", APQ_ALIGN_F64);
    if (misaligned(y, APQ_ALIGN_F64)) return fail(APQ_ERR_UNSUPPORTED, "resample_poly: y is not %lld-byte aligned", APQ_ALIGN_F64);
    return APQ_OK;
}

// ----------------------------------------------------------------------------------------------------------------- loudness
inline int loud_blocks(long long N) {
    const long long b = (N + kLoudPerBlock - 1) / kLoudPerBlock;
    return (int)(b < 1 ? 1 : (b > APQ_LOUD_MAX_BLOCKS ? APQ_LOUD_MAX_BLOCKS : b));
}

inline int check_loudness_n(const char* what, long long N) {
    if (N < 1) return fail(APQ_ERR_INVALID, what[0] == 's' ? "loudness_sumsq: N = %lld (at least 1)" : "loudness_apply: N = %lld (at least 1)", N);
    if (N > APQ_LOUD_MAX_N)
        return fail(APQ_ERR_UNSUPPORTED, what[0] == 's' ? "loudness_sumsq: N = %lld, served: up to %lld (the sum of squares is exact in fp64)"
                                                        : "loudness_apply: N = %lld, served: up to %lld (the sum of squares is exact in fp64)",
                    N, APQ_LOUD_MAX_N);
    return APQ_OK;
}

inline int check_loudness_sumsq(const void* x, const void* workspace, const void* sum, int N) {
    if (!x) return fail(APQ_ERR_INVALID, "loudness_sumsq: null x");
    if (!workspace) return fail(APQ_ERR_INVALID, "loudness_sumsq: null workspace");
    if (!sum) return fail(APQ_ERR_INVALID, "loudness_sumsq: null sum");
    const int rc = check_loudness_n("sumsq", N);
    if (rc != APQ_OK) return rc;
    if (misaligned(x, APQ_ALIGN_F64)) return fail(APQ_ERR_UNSUPPORTED, "loudness_sumsq: x is not %lld-byte aligned", APQ_ALIGN_F64);
    if (misaligned(workspace, APQ_ALIGN_F64))
        return fail(APQ_ERR_UNSUPPORTED, "loudness_sumsq: workspace is not %lld-byte aligned", APQ_ALIGN_F64);
    if (misaligned(sum, APQ_ALIGN_F64)) return fail(APQ_ERR_UNSUPPORTED, "loudness_sumsq: sum is not %lld-byte aligned", APQ_ALIGN_F64);
    return APQ_OK;
}

inline int check_loudness_apply(const void* x, const void* y, int N, double gain, int apply_gain) {
    if (!x) return fail(APQ_ERR_INVALID, "loudness_apply: null x");
    if (!y) return fail(APQ_ERR_INVALID, "loudness_apply: null y");
    const int rc = check_loudness_n("apply", N);
    if (rc != APQ_OK) return rc;
    if (apply_gain != 0 && apply_gain != 1) return fail(APQ_ERR_INVALID, "loudness_apply: apply_gain = %lld (0 or 1)", apply_gain);
    if (apply_gain && !(gain > 0.0 && gain <= 1.7976931348623157e308)) return fail(APQ_ERR_INVALID, "loudness_apply: the gain is not a positive finite number");
    if (misaligned(x, APQ_ALIGN_F64)) return fail(APQ_ERR_UNSUPPORTED, "loudness_apply: x is not %lld-byte aligned", APQ_ALIGN_F64);
    if (misaligned(y, APQ_ALIGN_F64)) return fail(APQ_ERR_UNSUPPORTED, "loudness_apply: y is not %lld-byte aligned", APQ_ALIGN_F64);
    return APQ_OK;
}

// ----------------------------------------------------------------------------------------------------------------- filtfilt
inline int ff_padlen(int M) { return 3 * (M + 1); }                         // scipy's default: 3 max(len(a), len(b))
inline long long ff_ext_len(long long L, int M) { return L + 2LL * ff_padlen(M); }
inline long long ff_workspace_bytes(long long L, int M) { return ff_ext_len(L, M) * (long long)sizeof(double); }

// b, a and zi are HOST arrays; the check never reads them
inline int check_filtfilt(const void* x, const void* y, const void* b, const void* a, const void* zi, const void* workspace, int L, int M) {
    if (!x) return fail(APQ_ERR_INVALID, "filtfilt: null x");
    if (!y) return fail(APQ_ERR_INVALID, "filtfilt: null y");
    if (!b) return fail(APQ_ERR_INVALID, "filtfilt: null b");
    if (!a) return fail(APQ_ERR_INVALID, "filtfilt: null a");
    if (!zi) return fail(APQ_ERR_INVALID, "filtfilt: null zi");
    if (!workspace) return fail(APQ_ERR_INVALID, "filtfilt: null workspace");
    if (L < 1) return fail(APQ_ERR_INVALID, "filtfilt: L = %lld (at least 1)", L);
    if (M < 1 || M > APQ_FF_MAX_M) return fail(APQ_ERR_UNSUPPORTED, "filtfilt: M = %lld, served: 1 .. %lld", M, APQ_FF_MAX_M);
    if (L <= ff_padlen(M))
        return fail(APQ_ERR_UNSUPPORTED, "filtfilt: L = %lld, served: above the pad length 3 (M + 1) = %lld", L, ff_padlen(M));
    if (L > APQ_FF_MAX_L) return fail(APQ_ERR_UNSUPPORTED, "filtfilt: L = %lld, served: up to %lld", L, APQ_FF_MAX_L);
    if (x == y) return fail(APQ_ERR_UNSUPPORTED, "filtfilt: y is x (the call is out of place)");
    if (misaligned(x, APQ_ALIGN_F64)) return fail(APQ_ERR_UNSUPPORTED, "filtfilt: x is not %lld-byte aligned", APQ_ALIGN_F64);
    if (misaligned(y, APQ_ALIGN_F64)) return fail(APQ_ERR_UNSUPPORTED, "filtfilt: y is not %lld-byte aligned", APQ_ALIGN_F64);
    if (misaligned(workspace, APQ_ALIGN_F64)) return fail(APQ_ERR_UNSUPPORTED, "filtfilt: workspace is not %lld-byte aligned", APQ_ALIGN_F64);
    return APQ_OK;
}

// ------------------------------------------------------------------------------------------------------------------ log-mel
inline int check_logmel_frames(const void* x, const void* window, const void* basis, const void* out, int L, int n_fft, int hop, int n_mels) {
    if (!x) return fail(APQ_ERR_INVALID, "logmel_frames: null x");
    if (!window) return fail(APQ_ERR_INVALID, "logmel_frames: null window");
    if (!basis) return fail(APQ_ERR_INVALID, "logmel_frames: null basis");
    if (!out) return fail(APQ_ERR_INVALID, "logmel_frames: null out");
    if (L < 1) return fail(APQ_ERR_INVALID, "logmel_frames: L = %lld (at least 1)", L);
    if (n_fft < 1) return fail(APQ_ERR_INVALID, "logmel_frames: n_fft = %lld (at least 1)", n_fft);
    if (hop < 1) return fail(APQ_ERR_INVALID, "logmel_frames: hop = %lld (at least 1)", hop);
    if (n_mels < 1) return fail(APQ_ERR_INVALID, "logmel_frames: n_mels = %lld (at least 1)", n_mels);
    if (n_fft % 2 != 0) return fail(APQ_ERR_UNSUPPORTED, "logmel_frames: n_fft = %lld is odd, served: even sizes", n_fft);
    if (n_fft < APQ_MEL_MIN_FFT || n_fft > APQ_MEL_MAX_FFT)
        return fail(APQ_ERR_UNSUPPORTED, "logmel_frames: n_fft = %lld, served: %lld .. %lld", n_fft, APQ_MEL_MIN_FFT, APQ_MEL_MAX_FFT);
    if (hop > n_fft) return fail(APQ_ERR_UNSUPPORTED, "logmel_frames: hop = %lld above n_fft = %lld", hop, n_fft);
    if (n_mels > APQ_MEL_MAX_MELS) return fail(APQ_ERR_UNSUPPORTED, "logmel_frames: n_mels = %lld, served: up to %lld", n_mels, APQ_MEL_MAX_MELS);
    if (L <= n_fft / 2)
        return fail(APQ_ERR_UNSUPPORTED, "logmel_frames: L = %lld, served: above n_fft / 2 = %lld (the reflection)", L, n_fft / 2);
    if (mel_frame_count(L, hop) > APQ_MAX_T)
        return fail(APQ_ERR_UNSUPPORTED, "logmel_frames: T = %lld frames, served: up to %lld", mel_frame_count(L, hop), APQ_MAX_T);
    if (misaligned(x, APQ_ALIGN_F64)) return fail(APQ_ERR_UNSUPPORTED, "logmel_frames: x is not %lld-byte aligned", APQ_ALIGN_F64);
    if (misaligned(window, APQ_ALIGN_F64)) return fail(APQ_ERR_UNSUPPORTED, "logmel_frames: window is not %lld-byte aligned", APQ_ALIGN_F64);
    if (misaligned(basis, APQ_ALIGN_ELEM)) return fail(APQ_ERR_UNSUPPORTED, "logmel_frames: basis is not %lld-byte aligned", APQ_ALIGN_ELEM);
    if (misaligned(out, APQ_ALIGN_ELEM)) return fail(APQ_ERR_UNSUPPORTED, "logmel_frames: out is not %lld-byte aligned", APQ_ALIGN_ELEM);
    return APQ_OK;
}

}  // namespace apq
