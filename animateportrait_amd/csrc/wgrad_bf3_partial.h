// wgrad_bf3_partial.h -- the partial sums of the bf16 weight-gradient GEMMs: how wgrad_bf16x3 (wgrad_bf16x3.h) and wgrad_xs_kernel
// (wgrad_xs.h) store a workgroup's accumulator tiles, and the kernel that sums the pixel splits and scatters them into dW.
#pragma once
#include "conv_igemm.h"     // f32x16

namespace apamd {

// Partial sums leave in the accumulators' own order, partial[split][tile = mt * c_tiles + ct][wave][tap][r][lane]:
// every store is 256 contiguous bytes per wave.  (The OIHW order -- element (m, ci, tap) at m * Q + ci * T + tap --
// put a lane's 4 bytes 36..64 bytes from its neighbour's: 144 fully scattered store instructions per wave, 115 of
// the kernel's 250 us.)  wgrad_bf3_reduce_kernel sums the splits in this order and scatters once.
template <int NWAVES, int T>
__device__ __forceinline__ void wgrad_bf3_store_partial(float* partial, int split, int m_tiles, int c_tiles, int mt, int ct, int wave,
                                                        int lane, const f32x16 (&acc)[T]) {
    const long long tile_floats = (long long)NWAVES * T * 1024;
    float* out = partial + ((long long)split * m_tiles * c_tiles + (long long)mt * c_tiles + ct) * tile_floats +
                 (long long)wave * T * 1024 + lane;
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) out[(t * 16 + r) * 64] = acc[t][r];
}

// dW = sum over the P splits of the partial tiles (fixed order), scattered to the caller's
// layout: s2d_c == 0: dW[m][ci][ky][kx] (OIHW / IOHW rows as the plan defines M and Cin); s2d_c = C > 0: the kernel saw
// the space-to-depth form (4C channels, 2 x 2 taps) of a stride-2 K x K layer: ci' = (ry*2+rx)*C + c, tap = ty*2+tx ->
// dW[m][c][2 ty + ry][2 tx + rx], taps >= K (a 3x3 layer's seven all-zero ones) dropped.
__global__ __launch_bounds__(256) void wgrad_bf3_reduce_kernel(const float* __restrict__ partial, int P, int M, int Cin,
                                                               int T, int c_tiles, long long total, int s2d_c, int K,
                                                               float* __restrict__ dw, int WM = 2) {
    for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < total; j += (long long)gridDim.x * 256) {
        float s = 0.f;
        int k = 0;
        for (; k + 4 <= P; k += 4) {                 // four loads in flight (same summation order as one by one)
            const float a = partial[(long long)k * total + j], b = partial[(long long)(k + 1) * total + j];
            const float c = partial[(long long)(k + 2) * total + j], d = partial[(long long)(k + 3) * total + j];
            s += a; s += b; s += c; s += d;
        }
        for (; k < P; ++k) s += partial[(long long)k * total + j];
        const int lane = (int)(j & 63), r = (int)((j >> 6) & 15);
        const long long jt = j >> 10;
        const int t = (int)(jt % T);
        const int nw = 2 * WM;                       // waves per tile: WM (m) x 2 (ci)
        const int wave = (int)((jt / T) % nw);
        const int tile = (int)(jt / T / nw);
        const int mt = tile / c_tiles, ct = tile - mt * c_tiles;
        const int mm = mt * (32 * WM) + (wave % WM) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        const int ci = ct * 64 + (wave / WM) * 32 + (lane & 31);
        if (mm >= M || ci >= Cin) continue;
        if (s2d_c == 0) {
            dw[((long long)mm * Cin + ci) * T + t] = s;
        } else {
            const int r2 = ci / s2d_c, c = ci - r2 * s2d_c;
            const int ky = 2 * (t >> 1) + (r2 >> 1), kx = 2 * (t & 1) + (r2 & 1);
            if (ky < K && kx < K) dw[(((long long)mm * s2d_c + c) * K + ky) * K + kx] = s;
        }
    }
}

}  // namespace apamd
