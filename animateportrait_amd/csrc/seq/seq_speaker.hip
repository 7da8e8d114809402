// seq_speaker.hip -- the two ends of the clip's speaker embedding (include/animateportrait_seq.h: apq_mel_frames,
// apq_speaker_head).  The reference gets the embedding from resemblyzer's VoiceEncoder (Module1/thirdparty/resemblyer_util/
// speaker_emb.py): 40 mel bands of a 400-point power spectrum every 10 ms, windows of 160 frames through a 3-layer LSTM with 256
// hidden units, then linear + ReLU + L2 norm per window, the mean over the windows and its L2 norm.  The LSTM is
// apq_lstm_layer_fwd's size; this file holds what lies before and behind it.  tests/speaker_reference.py states both in float64
// and is the contract.
//
// A clip is about a thousand frames and a few dozen windows: the work is tiny, so both kernels are laid out for few dependent
// steps and a fixed summation order, not for throughput.
//   mel_frames_kernel    one workgroup per frame, a lane per DFT bin.  The windowed frame (fp64) and a table of the n_fft twiddle
//                        factors (cos, sin as one 16-byte entry, index k n mod n_fft) sit in LDS.  A lane walks the frame: the
//                        sample is one address for the whole wave (a broadcast), the twiddle a 16-byte gather with stride k n
//                        between lanes -- 16 entries span the 64 banks, so a wave's read takes several turns for most n; at
//                        400 x 201 products a frame that is not worth a second table layout.  A direct DFT serves every even
//                        size alike (400 is no power of two).  Then a wave per mel band: lanes over the bins, a butterfly of
//                        shuffles.  Every sum is fp64; the one rounding to fp32 is the store.
//   speaker_head_kernel  one workgroup of 1024 lanes walks the rows.  Lane (j, q) keeps the weights w[j][64 q .. 64 q + 63] in
//                        registers for the whole call; a row of h is staged in LDS (the next one while this one is used) and
//                        read as broadcasts.  Per row: 64 fp32 fused multiply-adds a lane, the four runs of an output added as
//                        (0 + 1) + (2 + 3), bias, ReLU; the squared norm in fp64 (butterfly per wave, then the four waves in
//                        order); lane (j, 0) adds its quotient to its fp64 mean.  Rows come in order, so the mean's summation
//                        order is the row order.
// Neither kernel uses atomics, a workspace or a host synchronisation.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "seq_dft.h"
#include "seq_speaker_checks.h"

namespace {

constexpr int MT = apq::kMelThreads;
constexpr int MWAVES = MT / 64;
constexpr int E = APQ_SPK_E;
constexpr int HT = apq::kHeadThreads;
constexpr int RUN = apq::kHeadRun;
static_assert(apq::kMelBins <= MT, "a lane per bin");
static_assert(MT % 64 == 0 && HT % 64 == 0, "whole waves");

int launched(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(apq::err_buf(), 256, "%s: launch failed: %s", what, hipGetErrorString(e));
        return APQ_ERR_LAUNCH;
    }
    return APQ_OK;
}

__device__ __forceinline__ double wave_sum(double v) { return apq::dft_wave_sum(v); }

// ------------------------------------------------------------------------------------------------------------------ mel frames
struct MelParams {
    const float* x;
    const double* window;
    const float* basis;
    float* out;
    int L, n_fft, hop, n_mels, power;
};

// grid: T workgroups (frame t = blockIdx.x) of 576 threads
__global__ __launch_bounds__(MT) void mel_frames_kernel(const MelParams p) {
    __shared__ double fr[APQ_MEL_MAX_FFT];           // the frame times the window
    __shared__ double2 tw[APQ_MEL_MAX_FFT];          // (cos, sin)(2 pi i / n_fft)
    __shared__ double mag[apq::kMelBins];            // |X_k|^power

    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nb = p.n_fft / 2 + 1;
    apq::dft_frame_magnitudes<MT>(p.x, p.window, p.L, p.n_fft, p.hop, p.power, t, fr, tw, mag);      // (seq_dft.h)

    for (int m = wave; m < p.n_mels; m += MWAVES) {
        const double acc = apq::mel_band_sum(p.basis + (long long)m * nb, mag, nb, lane);
        if (lane == 0) p.out[(long long)t * p.n_mels + m] = (float)acc;
    }
}

// ---------------------------------------------------------------------------------------------------------------------- head
struct HeadParams {
    const float *h, *w, *b;
    float *partial, *embed;
    int B;
};

// grid: one workgroup of 1024 threads; lane (j, q) = (tid & 255, tid >> 8), so q is one value per wave
__global__ __launch_bounds__(HT) void speaker_head_kernel(const HeadParams p) {
    __shared__ float hs[2][E];
    __shared__ float part[4][E];
    __shared__ double red[2][4];

    const int tid = threadIdx.x, j = tid & (E - 1), q = tid >> 8, lane = tid & 63, wave = tid >> 6;
    const bool owner = tid < E;                      // the lanes (j, 0): waves 0 .. 3
    float wr[RUN];
#pragma unroll
    for (int i = 0; i < RUN; ++i) wr[i] = p.w[j * E + q * RUN + i];
    const float bias = p.b[j];
    double mean = 0.0;

    if (owner) hs[0][tid] = p.h[tid];
    __syncthreads();
    for (int r = 0; r < p.B; ++r) {
        const int cur = r & 1;
        if (owner && r + 1 < p.B) hs[cur ^ 1][tid] = p.h[(r + 1) * E + tid];     // read again only behind the next barrier
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < RUN; ++i) acc = fmaf(wr[i], hs[cur][q * RUN + i], acc);
        part[q][j] = acc;
        __syncthreads();
        float v = 0.f;
        if (owner) {
            v = ((part[0][j] + part[1][j]) + (part[2][j] + part[3][j])) + bias;
            v = v > 0.f ? v : 0.f;
            const double sq = wave_sum((double)v * (double)v);
            if (lane == 0) red[cur][wave] = sq;
        }
        __syncthreads();
        if (owner) {
            const double n2 = (red[cur][0] + red[cur][1]) + (red[cur][2] + red[cur][3]);
            const double quot = n2 > 0.0 ? (double)v / sqrt(n2) : 0.0;
            p.partial[r * E + j] = (float)quot;
            mean += quot;
        }
    }
    __syncthreads();                                 // (red[0] of the last rows is read above, written below)
    if (owner) {
        mean /= (double)p.B;
        const double sq = wave_sum(mean * mean);
        if (lane == 0) red[0][wave] = sq;
    }
    __syncthreads();
    if (owner) {
        const double n2 = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        p.embed[j] = (float)(n2 > 0.0 ? mean / sqrt(n2) : 0.0);
    }
}

}  // namespace

extern "C" {

int32_t apq_mel_frames_ok(const float* x, const double* window, const float* basis, const float* out, int32_t L, int32_t n_fft,
                          int32_t hop, int32_t n_mels, int32_t power) {
    return apq::check_mel_frames(x, window, basis, out, L, n_fft, hop, n_mels, power) == APQ_OK ? 1 : 0;
}

int apq_mel_frames(const float* x, const double* window, const float* basis, float* out, int32_t L, int32_t n_fft, int32_t hop,
                   int32_t n_mels, int32_t power, void* stream) {
    const int rc = apq::check_mel_frames(x, window, basis, out, L, n_fft, hop, n_mels, power);
    if (rc != APQ_OK) return rc;
    MelParams p;
    p.x = x; p.window = window; p.basis = basis; p.out = out; p.L = L; p.n_fft = n_fft; p.hop = hop; p.n_mels = n_mels; p.power = power;
    const int T = (int)apq::mel_frame_count(L, hop);
    (void)hipGetLastError();
    hipLaunchKernelGGL(mel_frames_kernel, dim3(T), dim3(MT), 0, (hipStream_t)stream, p);
    return launched("mel_frames");
}

int32_t apq_speaker_head_ok(const float* h, const float* w, const float* b, const float* partial, const float* embed, int32_t B) {
    return apq::check_speaker_head(h, w, b, partial, embed, B) == APQ_OK ? 1 : 0;
}

int apq_speaker_head(const float* h, const float* w, const float* b, float* partial, float* embed, int32_t B, void* stream) {
    const int rc = apq::check_speaker_head(h, w, b, partial, embed, B);
    if (rc != APQ_OK) return rc;
    HeadParams p;
    p.h = h; p.w = w; p.b = b; p.partial = partial; p.embed = embed; p.B = B;
    (void)hipGetLastError();
    hipLaunchKernelGGL(speaker_head_kernel, dim3(1), dim3(HT), 0, (hipStream_t)stream, p);
    return launched("speaker_head");
}

}  // extern "C"
