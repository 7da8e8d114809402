// Host side of the f0 calls of libapseq.so that needs no device: their argument checks and the sizes both sides share.  Plain
// C++ like seq_checks.h, so that a stand-alone program can compile it with the host sanitisers.
#pragma once

#include "seq_checks.h"

namespace apq {

constexpr int kF0Corr = 120;                          // the correlation window: 0.0075 x 16 kHz
constexpr int kF0Lpc = 480;                           // the rms / LPC window
constexpr int kF0Order = 18;                          // LPC order
constexpr int kF0Span = kF0Corr + APQ_F0_MAX_LAG + 2; // samples a frame's correlations read, at most
constexpr int kF0Lags = APQ_F0_MAX_LAG - APQ_F0_MIN_LAG + 3;   // lags kmin - 1 .. kmax + 1, at most
constexpr int kF0Threads = 384;                       // a lane per lag (6 waves)
static_assert(kF0Lags <= kF0Threads, "a lane per lag");

inline int check_f0_candidates(const void* x, int L, int T, int kmin, int kmax, const void* count, const void* lag, const void* val,
                               const void* rr, const void* s) {
    if (!x) return fail(APQ_ERR_INVALID, "f0_candidates: null x");
    if (!count) return fail(APQ_ERR_INVALID, "f0_candidates: null count");
    if (!lag) return fail(APQ_ERR_INVALID, "f0_candidates: null lag");
    if (!val) return fail(APQ_ERR_INVALID, "f0_candidates: null val");
    if (!rr) return fail(APQ_ERR_INVALID, "f0_candidates: null rr");
    if (!s) return fail(APQ_ERR_INVALID, "f0_candidates: null s");
    if (L < 1) return fail(APQ_ERR_INVALID, "f0_candidates: L = %lld (at least 1)", L);
    if (T < 1) return fail(APQ_ERR_INVALID, "f0_candidates: T = %lld (at least 1)", T);
    if (kmin > kmax) return fail(APQ_ERR_INVALID, "f0_candidates: kmin = %lld above kmax = %lld", kmin, kmax);
    if (T > APQ_MAX_T) return fail(APQ_ERR_UNSUPPORTED, "f0_candidates: T = %lld, served: up to %lld", T, APQ_MAX_T);
    if (kmin < APQ_F0_MIN_LAG) return fail(APQ_ERR_UNSUPPORTED, "f0_candidates: kmin = %lld, served: from %lld", kmin, APQ_F0_MIN_LAG);
    if (kmax > APQ_F0_MAX_LAG) return fail(APQ_ERR_UNSUPPORTED, "f0_candidates: kmax = %lld, served: up to %lld", kmax, APQ_F0_MAX_LAG);
    if (misaligned(x, APQ_ALIGN_ELEM)) return fail(APQ_ERR_UNSUPPORTED, "f0_candidates: x is not %lld-byte aligned", APQ_ALIGN_ELEM);
    if (misaligned(count, APQ_ALIGN_ELEM)) return fail(APQ_ERR_UNSUPPORTED, "f0_candidates: count is not %lld-byte aligned", APQ_ALIGN_ELEM);
    if (misaligned(lag, APQ_ALIGN_ELEM)) return fail(APQ_ERR_UNSUPPORTED, "f0_candidates: lag is not %lld-byte aligned", APQ_ALIGN_ELEM);
    if (misaligned(val, APQ_ALIGN_ELEM)) return fail(APQ_ERR_UNSUPPORTED, "f0_candidates: val is not %lld-byte aligned", APQ_ALIGN_ELEM);
    if (misaligned(rr, APQ_ALIGN_ELEM)) return fail(APQ_ERR_UNSUPPORTED, "f0_candidates: rr is not %lld-byte aligned", APQ_ALIGN_ELEM);
    if (misaligned(s, APQ_ALIGN_ELEM)) return fail(APQ_ERR_UNSUPPORTED, "f0_candidates: s is not %lld-byte aligned", APQ_ALIGN_ELEM);
    return APQ_OK;
}

inline int check_f0_track(const void* count, const void* lag, const void* val, const void* rr, const void* s, int T, int kmax, double fs,
                          const void* back, const void* path, const void* f0) {
    if (!count) return fail(APQ_ERR_INVALID, "f0_track: null count");
    if (!lag) return fail(APQ_ERR_INVALID, "f0_track: null lag");
    if (!val) return fail(APQ_ERR_INVALID, "f0_track: null val");
    if (!rr) return fail(APQ_ERR_INVALID, "f0_track: null rr");
    if (!s) return fail(APQ_ERR_INVALID, "f0_track: null s");
    if (!back) return fail(APQ_ERR_INVALID, "f0_track: null back");
    if (!path) return fail(APQ_ERR_INVALID, "f0_track: null path");
    if (!f0) return fail(APQ_ERR_INVALID, "f0_track: null f0");
    if (T < 1) return fail(APQ_ERR_INVALID, "f0_track: T = %lld (at least 1)", T);
    if (!(fs > 0.0) || !(fs <= 1e9)) return fail(APQ_ERR_INVALID, "f0_track: fs is not a positive sample rate");
    if (T > APQ_MAX_T) return fail(APQ_ERR_UNSUPPORTED, "f0_track: T = %lld, served: up to %lld", T, APQ_MAX_T);
    if (kmax < APQ_F0_MIN_LAG || kmax > APQ_F0_MAX_LAG)
        return fail(APQ_ERR_UNSUPPORTED, "f0_track: kmax = %lld, served: %lld .. %lld", kmax, APQ_F0_MIN_LAG, APQ_F0_MAX_LAG);
    if (misaligned(count, APQ_ALIGN_ELEM)) return fail(APQ_ERR_UNSUPPORTED, "f0_track: count is not %lld-byte aligned", APQ_ALIGN_ELEM);
    if (misaligned(lag, APQ_ALIGN_ELEM)) return fail(APQ_ERR_UNSUPPORTED, "f0_track: lag is not %lld-byte aligned", APQ_ALIGN_ELEM);
    if (misaligned(val, APQ_ALIGN_ELEM)) return fail(APQ_ERR_UNSUPPORTED, "f0_track: val is not %lld-byte aligned", APQ_ALIGN_ELEM);
    if (misaligned(rr, APQ_ALIGN_ELEM)) return fail(APQ_ERR_UNSUPPORTED, "f0_track: rr is not %lld-byte aligned", APQ_ALIGN_ELEM);
    if (misaligned(s, APQ_ALIGN_ELEM)) return fail(APQ_ERR_UNSUPPORTED, "f0_track: s is not %lld-byte aligned", APQ_ALIGN_ELEM);
    if (misaligned(f0, APQ_ALIGN_ELEM)) return fail(APQ_ERR_UNSUPPORTED, "f0_track: f0 is not %lld-byte aligned", APQ_ALIGN_ELEM);
    return APQ_OK;
}

}  // namespace apq
