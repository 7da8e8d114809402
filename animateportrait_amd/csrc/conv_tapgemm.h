// conv_tapgemm.h -- the 64 -> 1 channel 7x7 output layer (conv_direct.h's route) on the bf16 matrix pipe, split-bf16 arithmetic.
//
// One output channel leaves an implicit-GEMM tile 31/32 padding, and the Toeplitz form wastes 85 % of its products
// (profiles/r06_direct_conv.md).  Here the GEMM runs over the TAPS instead, and the convolution's sum over the window
// becomes a shift-add of its result:
//     T[t][p] = sum_c w[c][t] * x[c][p]            49 taps (padded to 64) x staged pixels x 64 channels, on the MFMA
//     y[oy][ox] = tanh(bias + sum_{ky,kx} T[ky * 7 + kx][(oy + ky, ox + kx)])
// with the three products xh*wh, xh*wl, xl*wh per multiply and fp32 accumulation, as conv_bf16x3.h.
//
// A workgroup (4 waves) owns a tile of TW = 58 output columns x th output rows (th: launch parameter) and walks the th + 6 staged
// rows of 64 pixels top to bottom, one row per step and ONE barrier per step:
//   * stage: lane = pixel of the row, wave w = channel octets w and w + 4 (the InstanceNorm constants of a wave's 16 channels
//     are wave-uniform).  The 16 raw fp32 loads of row r + 2 are issued (reflected, clamped addresses, all loads first) while
//     row r multiplies; row r + 1 is normalised, activated, split into bf16 head + tail and written to LDS as [pixel][64 x head |
//     64 x tail] with a 272-byte pixel stride, so that a B fragment (8 channels of one pixel) is one conflict-free ds_read_b128;
//   * tap GEMM: wave w multiplies the pixels 32 (w & 1) .. +31 by the taps 32 (w >> 1) .. +31: 4 k-steps x 3 MFMAs
//     (v_mfma_f32_32x32x16_bf16, taps = rows, pixels = columns).  The weights' A fragments (head and tail, 32 registers) are
//     split from the packed fp32 image [c][7][7] in the prologue and stay in registers;
//   * the accumulator has the pixel on the lane and 16 taps in its registers: it is written tap-major to LDS (T[tap][72]
//     floats, conflict-free rows of 32 lanes);
//   * shift-add, one step later: lane = output column, wave = ky (and ky + 4): the 7 terms of a tap row are 7 conflict-free
//     ds_read_b32, and their sum is added to the partial sum of output row r - ky, kept in an 8-row LDS ring; ky = 0 opens a
//     ring row, ky = 6 closes it (bias, activation, store).  Only ONE row of T is live per buffer -- never the tile's.
// LDS: 2 x 17,408 (staged rows) + 2 x 14,112 (T rows) + 2,048 (ring) = 65,088 bytes: two workgroups per CU.
#pragma once
#include "conv_igemm.h"
#include "lds_dma.h"

namespace apamd {

struct TapGemmParams {
    SrcSeg seg;              // the one source: 64 channels, raw fp32 with optional deferred InstanceNorm + activation
    int N, H, W;
    float* y;                // [N][1][H][W]
    const float* wp;         // packed fp32 weights [64][7][7] (conv_direct.h's image for one output channel)
    const float* bias;
    int act;
    int th, tiles_x, tiles_y;
};

struct TapGemmCfg {
    static constexpr int K = 7, R = 3, C = 64, NTAP = 49;
    static constexpr int SW = 64;                    // staged pixels per row = two MFMA column blocks
    static constexpr int TW = SW - (K - 1);          // output columns per tile
    static constexpr int XS = 2 * C * 2 + 16;        // bytes per staged pixel: head | tail | pad
    static constexpr int XROW = SW * XS;
    static constexpr int TS = 72;                    // floats per tap row of T (SW + K - 1 rounded up)
    static constexpr int TROW = NTAP * TS * 4;
    static constexpr int RING = 8 * SW * 4;
    static constexpr size_t lds_bytes() { return 2 * XROW + 2 * TROW + RING; }
};

// the kernel's address: instantiated in conv_tapgemm_inst.hip (its own translation unit, for build parallelism)
const void* tapgemm_kernel();

template <class G>
__global__ __launch_bounds__(256, 2) void conv_tapgemm_bf16x3(const TapGemmParams p) {
    typedef float f32x16 __attribute__((ext_vector_type(16)));
    extern __shared__ __attribute__((aligned(16))) unsigned char tg_smem[];
    unsigned char* const xbuf = tg_smem;
    float* const tbuf = reinterpret_cast<float*>(tg_smem + 2 * G::XROW);
    float* const ring = reinterpret_cast<float*>(tg_smem + 2 * G::XROW + 2 * G::TROW);

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    int b = (int)xcd_logical_block(gridDim.x, blockIdx.x);   // neighbouring tiles (shared halo) on one XCD's L2
    const int tix = b % p.tiles_x; b /= p.tiles_x;
    const int tiy = b % p.tiles_y;
    const int n = b / p.tiles_y;
    const int oy0 = tiy * p.th, ox0 = tix * G::TW;
    const int H = p.H, W = p.W, HW = H * W;
    const int th = min(p.th, H - oy0);
    const int nrows = th + G::K - 1;

    // weights: A fragments of this wave's 32 taps, lane l = tap (l & 31), channels 16 ks + 8 (l >> 5) + j
    const int tb = wave >> 1, pb = wave & 1, l31 = lane & 31, hh = lane >> 5;
    bf16x8 wh[4], wl[4];
    {
        const int t = tb * 32 + l31;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int c = ks * 16 + hh * 8 + j;
                float w = p.wp[c * G::NTAP + min(t, G::NTAP - 1)];      // (load, then select: no branch per element)
                w = t < G::NTAP ? w : 0.f;
                __bf16 h, l;
                split_bf16(w, h, l);
                wh[ks][j] = h;
                wl[ks][j] = l;
            }
    }

    // staging geometry: lane = staged column, wave-uniform channels 8 (wave + 4 q) + j
    const int gx = reflect_clamp(ox0 - G::R + lane, W);
    const float* const src = p.seg.data + (long long)n * G::C * HW + gx;
    float nm[2][8], nr[2][8];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = (wave + 4 * q) * 8 + j;
            nm[q][j] = p.seg.mean ? p.seg.mean[n * G::C + c] : 0.f;
            nr[q][j] = p.seg.mean ? p.seg.rstd[n * G::C + c] : 1.f;
            // wave-uniform, but 32 of them beside the addresses overflow the scalar file (one v_readlane per use): vector registers
            asm volatile("" : "+v"(nm[q][j]), "+v"(nr[q][j]));
        }
    const float slope = p.seg.act == 1 ? 0.f : (p.seg.act == 2 ? 0.2f : 1.f);      // act(t) = max(t, slope * t)

    float xr[2][8];
    auto issue = [&](int r) {
        const int gy = reflect_clamp(oy0 - G::R + r, H);
        const float* const row = src + gy * W;
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int j = 0; j < 8; ++j) xr[q][j] = row[((wave + 4 * q) * 8 + j) * HW];
    };
    auto commit = [&](unsigned char* dst) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            bf16x8 hv, lv;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float t = (xr[q][j] - nm[q][j]) * nr[q][j];
                const float v = fmaxf(t, slope * t);
                __bf16 h, l;
                split_bf16(v, h, l);
                hv[j] = h;
                lv[j] = l;
            }
            unsigned char* const d = dst + lane * G::XS + (wave + 4 * q) * 16;
            *reinterpret_cast<bf16x8*>(d) = hv;
            *reinterpret_cast<bf16x8*>(d + G::C * 2) = lv;
        }
    };
    // row rr of T (complete in tb): its seven tap rows into the partial sums of the output rows rr - ky
    const float bv = p.bias ? p.bias[0] : 0.f;
    auto shift_add = [&](int rr, const float* T) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int ky = wave + 4 * q;
            const int oyl = rr - ky;
            if (ky < G::K && oyl >= 0 && oyl < th) {                  // wave-uniform
                const float* const t0 = T + ky * G::K * G::TS + lane;
                float s = 0.f;
#pragma unroll
                for (int kx = 0; kx < G::K; ++kx) s += t0[kx * G::TS + kx];
                float* const slot = ring + (oyl & 7) * G::SW + lane;
                if (ky == 0) {
                    *slot = s;
                } else if (ky < G::K - 1) {
                    *slot += s;
                } else {
                    const float v = *slot + s + bv;
                    const int ox = ox0 + lane;
                    if (lane < G::TW && ox < W) p.y[((long long)n * H + oy0 + oyl) * W + ox] = apply_act(v, p.act);
                }
            }
        }
    };

    issue(0);
    commit(xbuf);
    if (nrows > 1) issue(1);
    __syncthreads();
    for (int r = 0; r < nrows; ++r) {
        const unsigned char* const X = xbuf + (r & 1) * G::XROW + (pb * 32 + l31) * G::XS + hh * 16;
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const bf16x8 xh = *reinterpret_cast<const bf16x8*>(X + ks * 32);
            const bf16x8 xl = *reinterpret_cast<const bf16x8*>(X + ks * 32 + G::C * 2);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl[ks], xh, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh[ks], xl, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh[ks], xh, acc, 0, 0, 0);
        }
        if (r + 1 < nrows) {
            commit(xbuf + ((r + 1) & 1) * G::XROW);
            if (r + 2 < nrows) issue(r + 2);
        }
        // accumulator register i of lane (l31, hh): tap 32 tb + (i & 3) + 8 (i >> 2) + 4 hh, pixel 32 pb + l31
        float* const T = tbuf + (r & 1) * (G::NTAP * G::TS);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int t = tb * 32 + (i & 3) + 8 * (i >> 2) + 4 * hh;
            if (t < G::NTAP) T[t * G::TS + pb * 32 + l31] = acc[i];
        }
        if (r > 0) shift_add(r - 1, tbuf + ((r - 1) & 1) * (G::NTAP * G::TS));
        __syncthreads();
    }
    shift_add(nrows - 1, tbuf + ((nrows - 1) & 1) * (G::NTAP * G::TS));
}

}  // namespace apamd
