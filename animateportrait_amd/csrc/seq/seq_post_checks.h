// Host side of the landmark post-processing calls of libapseq.so that needs no device: their argument checks.  Plain C++ like
// seq_checks.h, so that a stand-alone program can compile it with the host sanitisers.
#pragma once

#include "seq_checks.h"

namespace apq {

constexpr int kLipPoint0 = 48;                  // the mouth: points 48 .. 67
constexpr int kLipCols = (68 - kLipPoint0) * 3; // its 60 coordinates ...
constexpr int kLipStride = kLipCols + 1;        // ... and their row in LDS: odd, so that a thread per frame meets no bank twice
constexpr int kPostThreads = 512;

inline int check_sg_window(const char* which, const void* taps, int W, int T) {
    if (!taps) return fail(APQ_ERR_INVALID, which[0] == '0' ? "savgol: null taps0" : "savgol: null taps1");
    if (W > APQ_SG_MAX_W || W < APQ_SG_MIN_W)
        return fail(APQ_ERR_UNSUPPORTED, which[0] == '0' ? "savgol: W0 = %lld, served: %lld .. %lld" : "savgol: W1 = %lld, served: %lld .. %lld",
                    W, APQ_SG_MIN_W, APQ_SG_MAX_W);
    if (W % 2 == 0) return fail(APQ_ERR_UNSUPPORTED, which[0] == '0' ? "savgol: W0 = %lld is even" : "savgol: W1 = %lld is even", W);
    if (T < W) return fail(APQ_ERR_UNSUPPORTED, "savgol: T = %lld < W = %lld", T, W);
    if (misaligned(taps, APQ_ALIGN_ELEM))
        return fail(APQ_ERR_UNSUPPORTED, which[0] == '0' ? "savgol: taps0 is not %lld-byte aligned" : "savgol: taps1 is not %lld-byte aligned", APQ_ALIGN_ELEM);
    return APQ_OK;
}

inline int check_savgol(const void* x, const void* y, const void* taps0, const void* taps1, int T, int C, int c0, int c1, int c2,
                        int W0, int W1) {
    if (!x) return fail(APQ_ERR_INVALID, "savgol: null x");
    if (!y) return fail(APQ_ERR_INVALID, "savgol: null y");
    if (x == y) return fail(APQ_ERR_INVALID, "savgol: x and y are the same buffer (the filter runs out of place)");
    if (T < 1) return fail(APQ_ERR_INVALID, "savgol: T = %lld (at least 1)", T);
    if (C < 1) return fail(APQ_ERR_INVALID, "savgol: C = %lld (at least 1)", C);
    if (c0 < 0 || c0 > c1 || c1 > c2 || c2 > C) return fail(APQ_ERR_INVALID, "savgol: column ranges %lld <= %lld <= %lld do not lie in order inside the row", c0, c1, c2);
    if (T > APQ_MAX_T) return fail(APQ_ERR_UNSUPPORTED, "savgol: T = %lld, served: up to %lld", T, APQ_MAX_T);
    if ((long long)T * C > APQ_MAX_ELEMS) return fail(APQ_ERR_UNSUPPORTED, "savgol: T C = %lld elements, served: below 2^31", (long long)T * C);
    if (misaligned(x, APQ_ALIGN_ELEM)) return fail(APQ_ERR_UNSUPPORTED, "savgol: x is not %lld-byte aligned", APQ_ALIGN_ELEM);
    if (misaligned(y, APQ_ALIGN_ELEM)) return fail(APQ_ERR_UNSUPPORTED, "savgol: y is not %lld-byte aligned", APQ_ALIGN_ELEM);
    if (c1 > c0) {
        const int rc = check_sg_window("0", taps0, W0, T);
        if (rc != APQ_OK) return rc;
    }
    if (c2 > c1) {
        const int rc = check_sg_window("1", taps1, W1, T);
        if (rc != APQ_OK) return rc;
    }
    return APQ_OK;
}

inline int check_calib_baseline(const void* x, const void* y, int T, int k) {
    if (!x) return fail(APQ_ERR_INVALID, "calib_baseline: null x");
    if (!y) return fail(APQ_ERR_INVALID, "calib_baseline: null y");
    if (T < 2) return fail(APQ_ERR_INVALID, "calib_baseline: T = %lld (at least 2)", T);
    if (T > APQ_SEG_MAX_T) return fail(APQ_ERR_UNSUPPORTED, "calib_baseline: T = %lld, served: up to %lld (one segment)", T, APQ_SEG_MAX_T);
    if (k < 1 || k >= T) return fail(APQ_ERR_INVALID, "calib_baseline: k = %lld, served: 1 .. T - 1 = %lld", k, T - 1);
    if (misaligned(x, APQ_ALIGN_ELEM)) return fail(APQ_ERR_UNSUPPORTED, "calib_baseline: x is not %lld-byte aligned", APQ_ALIGN_ELEM);
    if (misaligned(y, APQ_ALIGN_ELEM)) return fail(APQ_ERR_UNSUPPORTED, "calib_baseline: y is not %lld-byte aligned", APQ_ALIGN_ELEM);
    return APQ_OK;
}

inline int check_segment_assemble(const void* in, const void* base, const void* fid, const void* out, int T, int flags) {
    if (!in) return fail(APQ_ERR_INVALID, "segment_assemble: null in");
    if (!out) return fail(APQ_ERR_INVALID, "segment_assemble: null out");
    if (in == out) return fail(APQ_ERR_INVALID, "segment_assemble: in and out are the same buffer (the call runs out of place)");
    if ((base == nullptr) != (fid == nullptr)) return fail(APQ_ERR_INVALID, "segment_assemble: base and fid come together or not at all");
    if (base && !(flags & APQ_SEG_CLOSE)) return fail(APQ_ERR_INVALID, "segment_assemble: base and fid belong to APQ_SEG_CLOSE");
    if (flags & ~(APQ_SEG_CLOSE | APQ_SEG_LIP | APQ_SEG_NOSE)) return fail(APQ_ERR_INVALID, "segment_assemble: flags = %lld", flags);
    if (T < 1) return fail(APQ_ERR_INVALID, "segment_assemble: T = %lld (at least 1)", T);
    if (T > APQ_SEG_MAX_T) return fail(APQ_ERR_UNSUPPORTED, "segment_assemble: T = %lld, served: up to %lld (one segment)", T, APQ_SEG_MAX_T);
    if (misaligned(in, APQ_ALIGN_ELEM)) return fail(APQ_ERR_UNSUPPORTED, "segment_assemble: in is not %lld-byte aligned", APQ_ALIGN_ELEM);
    if (misaligned(out, APQ_ALIGN_ELEM)) return fail(APQ_ERR_UNSUPPORTED, "segment_assemble: out is not %lld-byte aligned", APQ_ALIGN_ELEM);
    if (base && misaligned(base, APQ_ALIGN_ELEM)) return fail(APQ_ERR_UNSUPPORTED, "segment_assemble: base is not %lld-byte aligned", APQ_ALIGN_ELEM);
    if (fid && misaligned(fid, APQ_ALIGN_ELEM)) return fail(APQ_ERR_UNSUPPORTED, "segment_assemble: fid is not %lld-byte aligned", APQ_ALIGN_ELEM);
    return APQ_OK;
}

inline int check_image_landmarks(const void* in, const void* out, const void* stamps, int n_stamps, int T, double scale, int flags) {
    if (!in) return fail(APQ_ERR_INVALID, "image_landmarks: null in");
    if (!out) return fail(APQ_ERR_INVALID, "image_landmarks: null out");
    if (in == out) return fail(APQ_ERR_INVALID, "image_landmarks: in and out are the same buffer (the call runs out of place)");
    if (flags & ~(APQ_IMG_TRANSFORM | APQ_IMG_EYES)) return fail(APQ_ERR_INVALID, "image_landmarks: flags = %lld", flags);
    if (T < 1) return fail(APQ_ERR_INVALID, "image_landmarks: T = %lld (at least 1)", T);
    if (T > APQ_MAX_T) return fail(APQ_ERR_UNSUPPORTED, "image_landmarks: T = %lld, served: up to %lld", T, APQ_MAX_T);
    if ((flags & APQ_IMG_TRANSFORM) && !(scale != 0.0)) return fail(APQ_ERR_INVALID, "image_landmarks: scale is 0 or not a number");
    if (flags & APQ_IMG_EYES) {
        if (!stamps) return fail(APQ_ERR_INVALID, "image_landmarks: null stamps");
        if (T < 46) return fail(APQ_ERR_UNSUPPORTED, "image_landmarks: T = %lld, the first blink reads frame 45", T);
        if (n_stamps < 1 || n_stamps > APQ_MAX_STAMPS) return fail(APQ_ERR_UNSUPPORTED, "image_landmarks: n_stamps = %lld, served: 1 .. %lld", n_stamps, APQ_MAX_STAMPS);
        if (misaligned(stamps, APQ_ALIGN_ELEM)) return fail(APQ_ERR_UNSUPPORTED, "image_landmarks: stamps is not %lld-byte aligned", APQ_ALIGN_ELEM);
    }
    if (misaligned(in, APQ_ALIGN_ELEM)) return fail(APQ_ERR_UNSUPPORTED, "image_landmarks: in is not %lld-byte aligned", APQ_ALIGN_ELEM);
    if (misaligned(out, APQ_ALIGN_ELEM)) return fail(APQ_ERR_UNSUPPORTED, "image_landmarks: out is not %lld-byte aligned", APQ_ALIGN_ELEM);
    return APQ_OK;
}

}  // namespace apq
