// Device code the two mel kernels share (seq_speaker.hip: apq_mel_frames on fp32 samples; seq_audio.hip: apq_logmel_frames on
// fp64 samples): one frame of a centred short-time Fourier transform as a direct DFT in fp64, and a mel band's sum over its bins.
// The arithmetic and its order are apq_mel_frames' as it was before the split; only the sample type is a parameter.
#pragma once

#include <hip/hip_runtime.h>

namespace apq {

__device__ __forceinline__ double dft_wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// Frame t of x [L] (reflect-padded, numpy's 'reflect') times window [N] into fr, the N twiddle factors into tw, then |X_k|^power of
// the bins k = 0 .. N / 2 into mag.  Called by every thread of a workgroup of THREADS >= N / 2 + 1 lanes; the caller reads mag
// behind the function's last barrier.  fr, tw: N entries of LDS; mag: N / 2 + 1.
template <int THREADS, typename S>
__device__ __forceinline__ void dft_frame_magnitudes(const S* x, const double* window, int L, int N, int hop, int power, int t, double* fr,
                                                     double2* tw, double* mag) {
    const int tid = threadIdx.x;
    const int nb = N / 2 + 1;
    const long long first = (long long)t * hop - N / 2;       // the frame's first sample in the signal's own index

    for (int n = tid; n < N; n += THREADS) {
        // numpy's 'reflect'.  -N / 2 <= g <= L - 1 + N / 2 and L > N / 2: one reflection lands in [0, L)
        long long g = first + n;
        if (g < 0) g = -g;
        if (g >= L) g = 2LL * (L - 1) - g;
        fr[n] = (double)x[g] * window[n];
        const double a = 2.0 * (double)n / (double)N;
        tw[n] = make_double2(cospi(a), sinpi(a));
    }
    __syncthreads();

    if (tid < nb) {
        const int k = tid;                           // k <= N / 2 < N: one subtraction keeps idx = k n mod N below N
        double re = 0.0, im = 0.0;
        int idx = 0;
        for (int n = 0; n < N; ++n) {
            const double f = fr[n];
            const double2 c = tw[idx];
            re = fma(f, c.x, re);
            im = fma(f, c.y, im);
            idx += k;
            idx = idx >= N ? idx - N : idx;
        }
        const double m2 = re * re + im * im;
        mag[k] = power == 2 ? m2 : sqrt(m2);
    }
    __syncthreads();
}

// A wave's sum of row[k] mag[k] over the bins: lanes over the bins, a butterfly of shuffles; every lane returns the sum
__device__ __forceinline__ double mel_band_sum(const float* row, const double* mag, int nb, int lane) {
    double acc = 0.0;
    for (int k = lane; k < nb; k += 64) acc = fma((double)row[k], mag[k], acc);
    return dft_wave_sum(acc);
}

}  // namespace apq
