// seq_audio.hip -- the clip's audio front end on fp64 device tensors (include/animateportrait_seq.h: apq_resample_poly,
// apq_loudness_sumsq / apq_loudness_apply, apq_filtfilt, apq_logmel_frames): what animateportrait_amd/audio.py does with scipy
// and numpy between the decoded samples and the mel windows (resample_to_16k, normalize_loudness, the filtfilt of
// conditioned_signal, mel_spectrogram).  audio.py is the contract; audio_device.py is the caller.
//
//   resample_poly_kernel   a thread per output sample (o, c); it walks the taps of its own phase only (j = j0, j0 + up, ...) in
//                          ascending order with fused multiply-adds in fp64.  Neighbouring threads read neighbouring samples of
//                          x; the taps (at most 128 KB) stay in the caches.
//   loudness_sumsq_kernel  up to 256 workgroups, grid-stride: q = clip(rint(32768 x)), q^2 summed in 64-bit integers (exact in
//                          any order), a butterfly per wave, the waves through LDS, one partial per workgroup.
//   loudness_final_kernel  one workgroup adds the partials.  Two launches instead of an arrival counter.
//   loudness_apply_kernel  element-wise: audioop's clamp-then-floor.
//   filtfilt_kernel        ONE workgroup; lane 0 runs lfilter's transposed direct form II recurrence sample after sample -- the
//                          operations of scipy's C loop in their order, unfused -- while all 256 lanes move tiles of 1024
//                          samples between memory and LDS (the next tile in, the last one out) around it.  Forward pass over
//                          the oddly extended signal into the workspace, backward pass over the workspace reversed into y.
//                          A clip is a few hundred thousand dependent steps of three fp64 operations: milliseconds, and the
//                          only evaluation that has scipy's bits.  The blocked scan (chunks from a zero state, the states
//                          carried by A^K) was measured and rejected: for the front end's 5th-order 30 Hz high-pass the entries
//                          of A^K reach 1e8 at K = 256, and the result is off by 1e-4 .. 1 of the signal's peak where 1e-10 is
//                          asked.
//   logmel_frames_kernel   apq_mel_frames' frame (seq_dft.h) on fp64 samples, then the reference's dB map; one rounding to fp32.
// No kernel uses atomics or waits for another workgroup.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "seq_audio_checks.h"
#include "seq_dft.h"

// the loudness and filter formulas keep numpy's / scipy's operation order; the sums that may fuse ask for fma() by name
#pragma clang fp contract(off)

namespace {

constexpr int RT = apq::kRsThreads;
constexpr int LT = apq::kLoudThreads;
constexpr int FT = apq::kFfThreads;
constexpr int TILE = apq::kFfTile;
constexpr int MT = apq::kMelThreads;
constexpr int MWAVES = MT / 64;
static_assert(LT == 256 && APQ_LOUD_MAX_BLOCKS <= LT, "the final pass gives every partial a lane");
static_assert(TILE % FT == 0, "whole rounds of the staging loop");

int launched(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(apq::err_buf(), 256, "%s: launch failed: %s", what, hipGetErrorString(e));
        return APQ_ERR_LAUNCH;
    }
    return APQ_OK;
}

// ------------------------------------------------------------------------------------------------------------------ resampler
struct RsParams {
    const double *x, *h;
    double* y;
    int L, C, N, up, down, pre_pad, pre_remove;
    long long total;             // outputs: ceil(L up / down) C
};

__global__ __launch_bounds__(RT) void resample_poly_kernel(const RsParams p) {
    const long long idx = (long long)blockIdx.x * RT + threadIdx.x;
    if (idx >= p.total) return;
    const long long o = idx / p.C;
    const int c = (int)(idx - o * p.C);
    // output o is upfirdn's output n = o + pre_remove: sum over j of h[j] xu[m - j], xu the zero-stuffed signal, m = n down - pre_pad
    const long long m = (o + p.pre_remove) * p.down - p.pre_pad;
    long long xi = m >= 0 ? m / p.up : -((-m + p.up - 1) / p.up);        // floor(m / up)
    const int j0 = (int)(m - xi * p.up);                                // m mod up, in [0, up)
    double acc = 0.0;
    for (int j = j0; j < p.N && xi >= 0; j += p.up, --xi)
        if (xi < p.L) acc = fma(p.h[j], p.x[xi * p.C + c], acc);
    p.y[idx] = acc;
}

// ------------------------------------------------------------------------------------------------------------------- loudness
__device__ __forceinline__ double quantise16(double x) {
    const double r = rint(x * 32768.0);                                 // round half to even, as np.round
    return r < -32768.0 ? -32768.0 : (r > 32767.0 ? 32767.0 : r);
}

__device__ __forceinline__ long long block_sum_i64(long long v, long long* red) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(LT) void loudness_sumsq_kernel(const double* x, long long* partial, int N) {
    __shared__ long long red[LT / 64];
    long long acc = 0;
    for (long long i = (long long)blockIdx.x * LT + threadIdx.x; i < N; i += (long long)gridDim.x * LT) {
        const long long q = (long long)quantise16(x[i]);
        acc += q * q;
    }
    acc = block_sum_i64(acc, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

__global__ __launch_bounds__(LT) void loudness_final_kernel(const long long* partial, long long* sum, int blocks) {
    __shared__ long long red[LT / 64];
    const long long acc = block_sum_i64((int)threadIdx.x < blocks ? partial[threadIdx.x] : 0, red);
    if (threadIdx.x == 0) *sum = acc;
}

__global__ __launch_bounds__(LT) void loudness_apply_kernel(const double* x, double* y, int N, double gain, int apply_gain) {
    const long long i = (long long)blockIdx.x * LT + threadIdx.x;
    if (i >= N) return;
    const double q = quantise16(x[i]);
    if (!apply_gain) {
        y[i] = q / 32768.0;
        return;
    }
    double v = q * gain;
    v = v > 32767.0 ? 32767.0 : (v < -32767.0 ? -32768.0 : v);          // audioop's fbound: below minval + 1 becomes minval
    y[i] = floor(v) / 32768.0;
}

// ------------------------------------------------------------------------------------------------------------------- filtfilt
struct FfParams {
    const double* x;
    double *y, *w;               // w [L + 2 pad]: the forward pass's output
    int L, pad;
    double b[APQ_FF_MAX_M + 1], a[APQ_FF_MAX_M + 1], zi[APQ_FF_MAX_M];
};

// sample e of scipy's odd extension, 0 <= e < L + 2 pad; pad < L keeps every index inside x
__device__ __forceinline__ double ff_ext(const FfParams& p, long long e) {
    if (e < p.pad) return 2.0 * p.x[0] - p.x[p.pad - e];
    e -= p.pad;
    if (e < p.L) return p.x[e];
    return 2.0 * p.x[p.L - 1] - p.x[p.L - 2 - (e - p.L)];
}

// grid: one workgroup of 256 threads
template <int M>
__global__ __launch_bounds__(FT) void filtfilt_kernel(const FfParams p) {
    __shared__ double in[2][TILE];
    __shared__ double out[2][TILE];
    const int tid = threadIdx.x;
    const long long Le = (long long)p.L + 2LL * p.pad;
    const long long ntiles = (Le + TILE - 1) / TILE;

    for (int pass = 0; pass < 2; ++pass) {
        // tile i of the pass's input: the extension (forward), the workspace read from its end (backward)
        auto load = [&](long long i, double* dst) {
            for (int j = tid; j < TILE; j += FT) {
                const long long r = i * TILE + j;
                if (r < Le) dst[j] = pass == 0 ? ff_ext(p, r) : p.w[Le - 1 - r];
            }
        };
        // ... of its output: the workspace (forward), y without the extension (backward)
        auto store = [&](long long i, const double* src) {
            for (int j = tid; j < TILE; j += FT) {
                const long long r = i * TILE + j;
                if (r >= Le) continue;
                if (pass == 0) {
                    p.w[r] = src[j];
                } else {
                    const long long e = Le - 1 - r - p.pad;
                    if (e >= 0 && e < p.L) p.y[e] = src[j];
                }
            }
        };

        double z[M];
        const double s0 = pass == 0 ? ff_ext(p, 0) : p.w[Le - 1];
#pragma unroll
        for (int k = 0; k < M; ++k) z[k] = p.zi[k] * s0;

        load(0, in[0]);
        __syncthreads();
        for (long long i = 0; i < ntiles; ++i) {
            const int cur = (int)(i & 1);
            if (i + 1 < ntiles) load(i + 1, in[cur ^ 1]);
            if (i > 0) store(i - 1, out[cur ^ 1]);
            if (tid == 0) {
                const long long left = Le - i * TILE;
                const int n = left < TILE ? (int)left : TILE;
                // eight samples at a time: their LDS reads are issued ahead of the dependent chain (a tile's tail is padded
                // with whatever the buffer holds; those steps' outputs are never stored and the state is not used again)
                for (int j0 = 0; j0 < n; j0 += 8) {
                    double xs[8], ys[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) xs[u] = in[cur][j0 + u];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        // scipy's lfilter (transposed direct form II), its operations in its order
                        const double xn = xs[u];
                        const double yn = z[0] + p.b[0] * xn;
#pragma unroll
                        for (int k = 0; k < M - 1; ++k) z[k] = (z[k + 1] + xn * p.b[k + 1]) - yn * p.a[k + 1];
                        z[M - 1] = xn * p.b[M] - yn * p.a[M];
                        ys[u] = yn;
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u) out[cur][j0 + u] = ys[u];
                }
            }
            __syncthreads();
        }
        store(ntiles - 1, out[(ntiles - 1) & 1]);
        __threadfence();                             // the backward pass reads what other lanes of this workgroup wrote to w
        __syncthreads();
    }
}

template <int M>
void launch_filtfilt(const FfParams& p, hipStream_t s) {
    hipLaunchKernelGGL(filtfilt_kernel<M>, dim3(1), dim3(FT), 0, s, p);
}

// -------------------------------------------------------------------------------------------------------------------- log-mel
struct LogMelParams {
    const double *x, *window;
    const float* basis;
    float* out;
    int L, n_fft, hop, n_mels;
    double min_level;
};

// grid: T workgroups (frame t = blockIdx.x) of 576 threads
__global__ __launch_bounds__(MT) void logmel_frames_kernel(const LogMelParams p) {
    __shared__ double fr[APQ_MEL_MAX_FFT];
    __shared__ double2 tw[APQ_MEL_MAX_FFT];
    __shared__ double mag[apq::kMelBins];

    const int t = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nb = p.n_fft / 2 + 1;
    apq::dft_frame_magnitudes<MT>(p.x, p.window, p.L, p.n_fft, p.hop, 1, t, fr, tw, mag);

    for (int m = wave; m < p.n_mels; m += MWAVES) {
        const double acc = apq::mel_band_sum(p.basis + (long long)m * nb, mag, nb, lane);
        if (lane == 0) {
            const double db = 20.0 * log10(acc > p.min_level ? acc : p.min_level) - 16.0;
            p.out[(long long)t * p.n_mels + m] = (float)((db + 100.0) / 100.0);
        }
    }
}

}  // namespace

extern "C" {

int32_t apq_resample_poly_ok(const double* x, const double* h, const double* y, int32_t L, int32_t C, int32_t N, int32_t up,
                             int32_t down) {
    return apq::check_resample_poly(x, h, y, L, C, N, up, down) == APQ_OK ? 1 : 0;
}

int apq_resample_poly(const double* x, const double* h, double* y, int32_t L, int32_t C, int32_t N, int32_t up, int32_t down,
                      void* stream) {
    const int rc = apq::check_resample_poly(x, h, y, L, C, N, up, down);
    if (rc != APQ_OK) return rc;
    RsParams p;
    p.x = x; p.h = h; p.y = y; p.L = L; p.C = C; p.N = N; p.up = up; p.down = down;
    p.pre_pad = apq::rs_pre_pad(N, down);
    p.pre_remove = apq::rs_pre_remove(N, down);
    p.total = apq::rs_out_len(L, up, down) * C;
    (void)hipGetLastError();
    hipLaunchKernelGGL(resample_poly_kernel, dim3((unsigned)((p.total + RT - 1) / RT)), dim3(RT), 0, (hipStream_t)stream, p);
    return launched("resample_poly");
}

int64_t apq_loudness_workspace_bytes(int32_t N) { return (int64_t)apq::loud_blocks(N) * (int64_t)sizeof(int64_t); }

int32_t apq_loudness_sumsq_ok(const double* x, const void* workspace, const int64_t* sum, int32_t N) {
    return apq::check_loudness_sumsq(x, workspace, sum, N) == APQ_OK ? 1 : 0;
}

int apq_loudness_sumsq(const double* x, void* workspace, int64_t* sum, int32_t N, void* stream) {
    const int rc = apq::check_loudness_sumsq(x, workspace, sum, N);
    if (rc != APQ_OK) return rc;
    const int blocks = apq::loud_blocks(N);
    (void)hipGetLastError();
    hipLaunchKernelGGL(loudness_sumsq_kernel, dim3(blocks), dim3(LT), 0, (hipStream_t)stream, x, (long long*)workspace, N);
    hipLaunchKernelGGL(loudness_final_kernel, dim3(1), dim3(LT), 0, (hipStream_t)stream, (const long long*)workspace, (long long*)sum,
                       blocks);
    return launched("loudness_sumsq");
}

int32_t apq_loudness_apply_ok(const double* x, const double* y, int32_t N, double gain, int32_t apply_gain) {
    return apq::check_loudness_apply(x, y, N, gain, apply_gain) == APQ_OK ? 1 : 0;
}

int apq_loudness_apply(const double* x, double* y, int32_t N, double gain, int32_t apply_gain, void* stream) {
    const int rc = apq::check_loudness_apply(x, y, N, gain, apply_gain);
    if (rc != APQ_OK) return rc;
    (void)hipGetLastError();
    hipLaunchKernelGGL(loudness_apply_kernel, dim3((N + LT - 1) / LT), dim3(LT), 0, (hipStream_t)stream, x, y, N, gain, apply_gain);
    return launched("loudness_apply");
}

int64_t apq_filtfilt_workspace_bytes(int32_t L, int32_t M) {
    return (L < 1 || M < 1 || M > APQ_FF_MAX_M) ? 0 : (int64_t)apq::ff_workspace_bytes(L, M);
}

int32_t apq_filtfilt_ok(const double* x, const double* y, const double* b, const double* a, const double* zi, const void* workspace,
                        int32_t L, int32_t M) {
    return apq::check_filtfilt(x, y, b, a, zi, workspace, L, M) == APQ_OK ? 1 : 0;
}

int apq_filtfilt(const double* x, double* y, const double* b, const double* a, const double* zi, void* workspace, int32_t L,
                 int32_t M, void* stream) {
    const int rc = apq::check_filtfilt(x, y, b, a, zi, workspace, L, M);
    if (rc != APQ_OK) return rc;
    const double a0 = a[0];                          // (host arrays: read only behind the checks)
    if (!(a0 != 0.0)) return apq::fail(APQ_ERR_INVALID, "filtfilt: a[0] is zero or not a number");
    FfParams p = {};
    p.x = x; p.y = y; p.w = (double*)workspace; p.L = L; p.pad = apq::ff_padlen(M);
    for (int k = 0; k <= M; ++k) {                   // lfilter divides both by a[0]
        p.b[k] = b[k] / a0;
        p.a[k] = a[k] / a0;
    }
    for (int k = 0; k < M; ++k) p.zi[k] = zi[k];
    const hipStream_t s = (hipStream_t)stream;
    (void)hipGetLastError();
    switch (M) {
        case 1: launch_filtfilt<1>(p, s); break;
        case 2: launch_filtfilt<2>(p, s); break;
        case 3: launch_filtfilt<3>(p, s); break;
        case 4: launch_filtfilt<4>(p, s); break;
        case 5: launch_filtfilt<5>(p, s); break;
        case 6: launch_filtfilt<6>(p, s); break;
        case 7: launch_filtfilt<7>(p, s); break;
        default: launch_filtfilt<8>(p, s); break;
    }
    return launched("filtfilt");
}

int32_t apq_logmel_frames_ok(const double* x, const double* window, const float* basis, const float* out, int32_t L, int32_t n_fft,
                             int32_t hop, int32_t n_mels) {
    return apq::check_logmel_frames(x, window, basis, out, L, n_fft, hop, n_mels) == APQ_OK ? 1 : 0;
}

int apq_logmel_frames(const double* x, const double* window, const float* basis, float* out, int32_t L, int32_t n_fft, int32_t hop,
                      int32_t n_mels, void* stream) {
    const int rc = apq::check_logmel_frames(x, window, basis, out, L, n_fft, hop, n_mels);
    if (rc != APQ_OK) return rc;
    LogMelParams p;
    p.x = x; p.window = window; p.basis = basis; p.out = out; p.L = L; p.n_fft = n_fft; p.hop = hop; p.n_mels = n_mels;
    p.min_level = exp(-100.0 / 20.0 * log(10.0));    // the reference's 1e-5
    const int T = (int)apq::mel_frame_count(L, hop);
    (void)hipGetLastError();
    hipLaunchKernelGGL(logmel_frames_kernel, dim3(T), dim3(MT), 0, (hipStream_t)stream, p);
    return launched("logmel_frames");
}

}  // extern "C"
