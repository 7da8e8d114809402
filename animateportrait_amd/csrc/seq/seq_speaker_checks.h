// Host side of the speaker-embedding calls of libapseq.so that needs no device: their argument checks and the sizes both sides
// share.  Plain C++ like seq_checks.h, so that a stand-alone program can compile it with the host sanitisers.
#pragma once

#include "seq_checks.h"

namespace apq {

constexpr int kMelBins = APQ_MEL_MAX_FFT / 2 + 1;     // bins of a frame, at most: 513
constexpr int kMelThreads = 576;                      // 9 waves: a lane per DFT bin
constexpr int kHeadThreads = 1024;                    // 4 lanes per output: each keeps 64 weights of its row in registers
constexpr int kHeadRun = APQ_SPK_E / 4;               // ... the length of a lane's run of products
static_assert(APQ_SPK_E == APQ_LSTM_H, "the head reads the LSTM's hidden state");
static_assert(kHeadThreads == 4 * APQ_SPK_E, "4 lanes per output");

// frames of a signal of L samples: L / hop + 1
inline long long mel_frame_count(int L, int hop) { return (long long)L / hop + 1; }

inline int check_mel_frames(const void* x, const void* window, const void* basis, const void* out, int L, int n_fft, int hop, int n_mels,
                            int power) {
    if (!x) return fail(APQ_ERR_INVALID, "mel_frames: null x");
    if (!window) return fail(APQ_ERR_INVALID, "mel_frames: null window");
    if (!basis) return fail(APQ_ERR_INVALID, "mel_frames: null basis");
    if (!out) return fail(APQ_ERR_INVALID, "mel_frames: null out");
    if (L < 1) return fail(APQ_ERR_INVALID, "mel_frames: L = %lld (at least 1)", L);
    if (n_fft < 1) return fail(APQ_ERR_INVALID, "mel_frames: n_fft = %lld (at least 1)", n_fft);
    if (hop < 1) return fail(APQ_ERR_INVALID, "mel_frames: hop = %lld (at least 1)", hop);
    if (n_mels < 1) return fail(APQ_ERR_INVALID, "mel_frames: n_mels = %lld (at least 1)", n_mels);
    if (power != 1 && power != 2) return fail(APQ_ERR_INVALID, "mel_frames: power = %lld (1 or 2)", power);
    if (n_fft % 2 != 0) return fail(APQ_ERR_UNSUPPORTED, "mel_frames: n_fft = %lld is odd, served: even sizes", n_fft);
    if (n_fft < APQ_MEL_MIN_FFT || n_fft > APQ_MEL_MAX_FFT)
        return fail(APQ_ERR_UNSUPPORTED, "mel_frames: n_fft = %lld, served: %lld .. %lld", n_fft, APQ_MEL_MIN_FFT, APQ_MEL_MAX_FFT);
    if (hop > n_fft) return fail(APQ_ERR_UNSUPPORTED, "mel_frames: hop = %lld above n_fft = %lld", hop, n_fft);
    if (n_mels > APQ_MEL_MAX_MELS) return fail(APQ_ERR_UNSUPPORTED, "mel_frames: n_mels = %lld, served: up to %lld", n_mels, APQ_MEL_MAX_MELS);
    if (L <= n_fft / 2)
        return fail(APQ_ERR_UNSUPPORTED, "mel_frames: L = %lld, served: above n_fft / 2 = %lld (the reflection)", L, n_fft / 2);
    if (mel_frame_count(L, hop) > APQ_MAX_T)
        return fail(APQ_ERR_UNSUPPORTED, "mel_frames: T = %lld frames, served: up to %lld", mel_frame_count(L, hop), APQ_MAX_T);
    if (misaligned(x, APQ_ALIGN_ELEM)) return fail(APQ_ERR_UNSUPPORTED, "mel_frames: x is not %lld-byte aligned", APQ_ALIGN_ELEM);
    if (misaligned(window, APQ_ALIGN_F64)) return fail(APQ_ERR_UNSUPPORTED, "mel_frames: window is not %lld-byte aligned", APQ_ALIGN_F64);
    if (misaligned(basis, APQ_ALIGN_ELEM)) return fail(APQ_ERR_UNSUPPORTED, "mel_frames: basis is not %lld-byte aligned", APQ_ALIGN_ELEM);
    if (misaligned(out, APQ_ALIGN_ELEM)) return fail(APQ_ERR_UNSUPPORTED, "mel_frames: out is not %lld-byte aligned", APQ_ALIGN_ELEM);
    return APQ_OK;
}

inline int check_speaker_head(const void* h, const void* w, const void* b, const void* partial, const void* embed, int B) {
    if (!h) return fail(APQ_ERR_INVALID, "speaker_head: null h");
    if (!w) return fail(APQ_ERR_INVALID, "speaker_head: null w");
    if (!b) return fail(APQ_ERR_INVALID, "speaker_head: null b");
    if (!partial) return fail(APQ_ERR_INVALID, "speaker_head: null partial");
    if (!embed) return fail(APQ_ERR_INVALID, "speaker_head: null embed");
    if (B < 1) return fail(APQ_ERR_INVALID, "speaker_head: B = %lld (at least 1)", B);
    if (B > APQ_SPK_MAX_B) return fail(APQ_ERR_UNSUPPORTED, "speaker_head: B = %lld, served: up to %lld", B, APQ_SPK_MAX_B);
    if (misaligned(h, APQ_ALIGN_ELEM)) return fail(APQ_ERR_UNSUPPORTED, "speaker_head: h is not %lld-byte aligned", APQ_ALIGN_ELEM);
    if (misaligned(w, APQ_ALIGN_ELEM)) return fail(APQ_ERR_UNSUPPORTED, "speaker_head: w is not %lld-byte aligned", APQ_ALIGN_ELEM);
    if (misaligned(b, APQ_ALIGN_ELEM)) return fail(APQ_ERR_UNSUPPORTED, "speaker_head: b is not %lld-byte aligned", APQ_ALIGN_ELEM);
    if (misaligned(partial, APQ_ALIGN_ELEM)) return fail(APQ_ERR_UNSUPPORTED, "speaker_head: partial is not %lld-byte aligned", APQ_ALIGN_ELEM);
    if (misaligned(embed, APQ_ALIGN_ELEM)) return fail(APQ_ERR_UNSUPPORTED, "speaker_head: embed is not %lld-byte aligned", APQ_ALIGN_ELEM);
    return APQ_OK;
}

}  // namespace apq
