// conv_pack.h -- the weight packer of the split-bf16 convolutions (conv_bf16x3.h).  Included by conv_pack.hip only.
#pragma once
#include "conv_bf16x3.h"

namespace apamd {

// ---- weight packer: out = LDS image per (cout tile, chunk): [part][tap][kgroup][CO_TILE][8] bf16
// The source is addressed through element strides, so that the operand of a data-gradient operator -- a channel slice, a
// transposed-tap view of the layer's parameter -- or of the derived forms below needs no contiguous temporary:
//   view == 0: the dense OIHW / IOHW tensor described by layout / Cin / Cout / K (strides derived here);
//   view == 1: element (co, cin, ky, kx) of the OPERATOR at  w[co * s_co + cin * s_ci + ky * s_ky + kx * s_kx];
//   s2d_c  > 0: the operator is the 2 x 2 space-to-depth form over 4 * s2d_c channels of a ksrc x ksrc stride-2 layer:
//               operator (cin = r * s2d_c + c, tap (ty, tx)) = source (c, 2 ty + (r >> 1), 2 tx + (r & 1)), zero beyond ksrc;
//   rows_c > 0: the operator is the 1 x K row form of a K x K stem over rows_c channels: operator cin = ky * rows_c + c.
struct PackBf3Params {
    const float* w;
    unsigned short* out;
    int Cin, Cout, K, layout, flip;
    int KH;                                             // 0: square K x K weights; 1: 1 x K
    int nseg, segC[kMaxSeg], chunk_begin[kMaxSeg];
    int CO_TILE, nchunks, co_tiles;
    int ntaps, tap_ky[kMaxTaps], tap_kx[kMaxTaps];      // source tap of packed tap t (already flipped if needed)
    int view, s2d_c, rows_c, ksrc;
    long long s_co, s_ci, s_ky, s_kx;
};

// One 16-byte slot (8 input channels of one cout, tap and k-group) per thread and step, head and tail images together:
// the source value is read once for both parts and leaves as two 16-byte stores (a thread per bf16 element measured 424 us
// for the generator's table, 0.45 TB/s).
__device__ __forceinline__ void pack_bf16x3_body(const PackBf3Params& p, long long first, long long step) {
    const int T = p.ntaps;
    const unsigned slots_blk = (unsigned)T * 2u * (unsigned)p.CO_TILE;          // slots of one part of a (cout tile, chunk) block
    const long long total = (long long)p.co_tiles * p.nchunks * slots_blk;
    const int KH = p.KH > 0 ? p.KH : p.K;                                       // KH != K: a 1 x K row kernel
    for (long long sidx = first; sidx < total; sidx += step) {
        const unsigned blk = (unsigned)(sidx / slots_blk);
        unsigned r = (unsigned)(sidx - (long long)blk * slots_blk);
        const int chunk = (int)(blk % (unsigned)p.nchunks), cot = (int)(blk / (unsigned)p.nchunks);
        const int col = (int)(r % (unsigned)p.CO_TILE); r /= (unsigned)p.CO_TILE;
        const int kg = (int)(r & 1u);
        const int t = (int)(r >> 1);
        const int co = cot * p.CO_TILE + col;
        int s = 0;
        if (p.nseg > 1 && chunk >= p.chunk_begin[1]) s = 1;
        if (p.nseg > 2 && chunk >= p.chunk_begin[2]) s = 2;
        int seg0 = 0;
        for (int j = 0; j < s; ++j) seg0 += p.segC[j];
        const int cs0 = (chunk - p.chunk_begin[s]) * 16 + kg * 8;
        const bool row_ok = co < p.Cout && p.tap_ky[t] >= 0;       // tap_ky < 0: a window position this phase does not have
        bf16x8 hv, lv;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int cs = cs0 + c;
            float v = 0.f;
            if (row_ok && cs < p.segC[s]) {
                int cin = cs + seg0;
                int ky = p.tap_ky[t], kx = p.tap_kx[t];
                bool ok = true;
                if (p.s2d_c > 0) {
                    const int rr = cin / p.s2d_c;
                    cin -= rr * p.s2d_c;
                    ky = 2 * ky + (rr >> 1);
                    kx = 2 * kx + (rr & 1);
                    ok = ky < p.ksrc && kx < p.ksrc;
                } else if (p.rows_c > 0) {
                    ky = cin / p.rows_c;
                    cin -= ky * p.rows_c;
                    ok = ky < p.ksrc;
                }
                if (ok) {
                    long long off;
                    if (p.view) {
                        off = co * p.s_co + cin * p.s_ci + ky * p.s_ky + kx * p.s_kx;
                    } else {
                        off = p.layout == 0 ? (((long long)co * p.Cin + cin) * KH + ky) * p.K + kx
                                            : (((long long)cin * p.Cout + co) * KH + ky) * p.K + kx;
                    }
                    v = p.w[off];
                }
            }
            __bf16 h, l;
            split_bf16(v, h, l);
            hv[c] = h;
            lv[c] = l;
        }
        // image of the block: [part][tap][kgroup][CO_TILE] slots
        bf16x8* const img = reinterpret_cast<bf16x8*>(p.out) + (long long)blk * 2 * slots_blk;
        const unsigned slot = ((unsigned)t * 2u + (unsigned)kg) * (unsigned)p.CO_TILE + (unsigned)col;
        img[slot] = hv;
        img[slots_blk + slot] = lv;
    }
}

static __global__ void pack_bf16x3_kernel(const PackBf3Params p) {
    pack_bf16x3_body(p, (long long)blockIdx.x * blockDim.x + threadIdx.x, (long long)gridDim.x * blockDim.x);
}

// every (layer, variant) of a network in ONE launch: entry blockIdx.y of a device-resident table (built once: the parameters
// are views of the optimiser's flat buffer and the packed images are persistent, so the pointers do not change)
static __global__ void pack_bf16x3_table_kernel(const PackBf3Params* __restrict__ table) {
    __shared__ PackBf3Params p;
    const int* src = reinterpret_cast<const int*>(table + blockIdx.y);
    int* dst = reinterpret_cast<int*>(&p);
    for (int i = threadIdx.x; i < (int)(sizeof(PackBf3Params) / sizeof(int)); i += blockDim.x) dst[i] = src[i];
    __syncthreads();
    pack_bf16x3_body(p, (long long)blockIdx.x * blockDim.x + threadIdx.x, (long long)gridDim.x * blockDim.x);
}

}  // namespace apamd
