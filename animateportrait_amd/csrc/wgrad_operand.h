// wgrad_operand.h -- the operand passes of the bf16 weight-gradient GEMM (wgrad_bf16x3.h).  Both of its operands are pixel-octet
// slots with the CHANNEL innermost,
//     T[n][head|tail][row][x / 8][channel][8 x bf16]        (the tail planes are not written for a head-only consumer),
// a padded view of act(IN(concat(src))): (row, x) <-> source (row - pad, x - pad); zeros beyond the padded image and for channels
// >= C.  Source forms and the kernel that serves each (SplitTForm in wgrad_plan.h, chosen by split_transpose_form):
//   plain           any padding, segments and width; also the ROW view (rows_k)    split_transpose_kernel      ST_GENERAL
//                   unpadded, whole octet rows (the gradient operand)              split_transpose_vec_kernel  ST_VEC
//   padded rows     pad 1, W in {32, 64, 128, 256}; fp32 or bf16 segments          split_transpose_pad_kernel  ST_PAD_ROWS
//   space-to-depth  the 2 x 2 view of a stride-2 layer's source, whole rows        split_transpose_s2d_kernel  ST_S2D_ROWS
//                   (other widths: split_transpose_kernel, s2d_c)
//   split copy      the forward pass's XS slots re-tiled, plain or s2d view        xs_transpose_kernel
// Included by wgrad_operand.hip only: the kernels have external linkage.
#pragma once
#include "conv_igemm.h"
#include "lds_dma.h"

namespace apamd {

// ---- from the fp32 (or bf16) tensors: reflection or zero padding inside [0, H+2pad) x [0, W+2pad).  The transposition goes
// through LDS: fp32 reads run along x, slot writes along c.
struct SplitTParams {
    SrcSeg seg[kMaxSeg];      // chunk_begin = first concat channel
    int nseg;
    int N, C, H, W, pad, pad_mode, Hp, X8, Cp;
    int s2d_c;                // > 0: space-to-depth view of a pad-1 source with s2d_c channels (see below)
    int heads_only;           // 1: the consumer multiplies head parts only (AP_PRECISION_BF16): the tail planes are not written
    int rows_k;               // > 0: row view of a K x K layer's source, K = rows_k (see below; split_transpose_kernel only)
    uint4* out;
};

// The tail of the four split_transpose kernels -- 8 floats of an LDS row split into a head and a tail bf16x8, the head slot stored,
// the tail slot unless heads_only -- is written out in each of them (split_store_octets serves the pad kernel only).  One
// __forceinline__ helper for it was tried by value, by reference and with (row, index) arguments: every form changed all four
// kernels (split_transpose_vec_kernel 2083 -> 2077 instructions, split_transpose_kernel 86 -> 68 SGPRs and 3777 -> 4171).

// Space-to-depth view (s2d_c = C0 > 0): channel c' = (ry * 2 + rx) * C0 + c of the (H, W) = (H0/2 + 1, W0/2 + 1) map is
// pad1(act(IN(concat(src))))[c][2 y + ry][2 x + rx] -- the operand of a stride-2 K x K (K = 3, 4) layer rewritten as
// the 2 x 2 stride-1 layer over 4 C0 channels (as ap_split_prepass_s2d does for the forward pass), so that strided
// weight gradients run on the same bf16 GEMM kernel.  p.H / p.W are then the source's own size and pad must be 0.
// Row view (rows_k = K > 0): channel c' = c * K + ky of the H x (W + 2 pad) map is pad(act(IN(src)))[c][y + ky][x] -- the operand of
// a K x K stride-1 layer on few channels rewritten as the 1 x K layer over K C channels (as ap_split_prepass_rows does for the
// forward pass: WgradBf3Cfg KY = 1).  p.C is then the number of VIEW channels (K times the source's).
// grid: (ceil(Hp * X8 / 8), Cp / 64, N): a workgroup transposes 8 consecutive octets (64 padded pixels, possibly
// across a row boundary) of 64 channels.
__global__ __launch_bounds__(256) void split_transpose_kernel(const SplitTParams p) {
    __shared__ float f[64][65];
    const int cg = blockIdx.y, n = blockIdx.z, tid = threadIdx.x;
    const int He = p.H + 2 * p.pad, We = p.W + 2 * p.pad, HW = p.H * p.W;
    const int oct0 = blockIdx.x * 8, noct = p.Hp * p.X8;
    // phase 1: thread = (pixel of the span, channel quarter): 16 independent loads, 8-pixel runs per octet
    {
        const int px = tid & 63, oct = oct0 + (px >> 3);
        const int y = oct / p.X8, x = (oct - y * p.X8) * 8 + (px & 7);
        int sy = y - p.pad, sx = x - p.pad;
        bool ok = oct < noct && y < He && x < We;
        if (p.s2d_c > 0) {
            ok = oct < noct && y <= p.H / 2 && x <= p.W / 2;       // the view is (H/2 + 1) x (W/2 + 1)
        } else if (p.rows_k > 0) {
            ok = oct < noct && y < p.H && x < We;                  // the view is H x (W + 2 pad); rows resolved per channel
        } else if (p.pad_mode == 1) {
            sy = reflect_clamp(sy, p.H);
            sx = reflect_clamp(sx, p.W);
        } else {
            ok = ok && sy >= 0 && sy < p.H && sx >= 0 && sx < p.W;
        }
        const int soff = ok ? sy * p.W + sx : 0;
        const int cq = __builtin_amdgcn_readfirstlane(tid >> 6) * 16;   // this wave's 16 channels of the group (scalar: see split_transpose_pad_kernel)
        float v[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            int c = cg * 64 + cq + i;
            v[i] = 0.f;
            if (c < p.C) {
                bool okc = ok;
                int so = soff;
                if (p.s2d_c > 0) {                                 // (wave-uniform: 16 consecutive channels share r
                    const int r = c / p.s2d_c;                     //  unless they straddle a multiple of C0)
                    c -= r * p.s2d_c;
                    const int yy = 2 * y + (r >> 1) - 1, xx = 2 * x + (r & 1) - 1;
                    okc = ok && yy >= 0 && yy < p.H && xx >= 0 && xx < p.W;
                    so = okc ? yy * p.W + xx : 0;
                } else if (p.rows_k > 0) {
                    const int cc = c / p.rows_k;
                    int yy = y + (c - cc * p.rows_k) - p.pad, xx = sx;
                    c = cc;
                    if (p.pad_mode == 1) {
                        yy = reflect_clamp(yy, p.H);
                        xx = reflect_clamp(xx, p.W);
                    } else {
                        okc = ok && yy >= 0 && yy < p.H && xx >= 0 && xx < p.W;
                    }
                    so = okc ? yy * p.W + xx : 0;
                }
                const int s = concat_seg(p.nseg, c, p.seg[1].chunk_begin, p.seg[2].chunk_begin);
                const SrcSeg sg = s == 0 ? p.seg[0] : (s == 1 ? p.seg[1] : p.seg[2]);   // wave-uniform
                const int cs = c - sg.chunk_begin;
                float t = sg.data[((long long)n * sg.C + cs) * HW + so];
                if (sg.mean != nullptr) t = (t - sg.mean[n * sg.C + cs]) * sg.rstd[n * sg.C + cs];
                t = sg.act == 1 ? fmaxf(t, 0.f) : (sg.act == 2 ? (t > 0.f ? t : 0.2f * t) : t);
                v[i] = okc ? t : 0.f;
            }
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) f[cq + i][px] = v[i];
    }
    __syncthreads();
    // phase 2: thread = (channel, octet): 64 consecutive channels of one octet per wave-store (1 KiB contiguous)
    const int c = tid & 63;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int o = (tid >> 6) + 4 * k, oct = oct0 + o;
        if (oct < noct) {
            bf16x8 hv, lv;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                __bf16 h, l;
                split_bf16(f[c][o * 8 + j], h, l);
                hv[j] = h;
                lv[j] = l;
            }
            *reinterpret_cast<bf16x8*>(p.out + ((long long)(n * 2 + 0) * noct + oct) * p.Cp + cg * 64 + c) = hv;
            if (!p.heads_only) *reinterpret_cast<bf16x8*>(p.out + ((long long)(n * 2 + 1) * noct + oct) * p.Cp + cg * 64 + c) = lv;
        }
    }
}

__device__ __forceinline__ float4 norm_act4(float4 v, const SrcSeg& sg, int nc) {
    if (sg.mean != nullptr) {
        const float m = sg.mean[nc], r = sg.rstd[nc];
        v.x = (v.x - m) * r; v.y = (v.y - m) * r; v.z = (v.z - m) * r; v.w = (v.w - m) * r;
    }
    if (sg.act == 1) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
    else if (sg.act == 2) {
        v.x = v.x > 0.f ? v.x : 0.2f * v.x; v.y = v.y > 0.f ? v.y : 0.2f * v.y;
        v.z = v.z > 0.f ? v.z : 0.2f * v.z; v.w = v.w > 0.f ? v.w : 0.2f * v.w;
    }
    return v;
}

// Fast path of split_transpose_kernel for an unpadded operand whose rows are whole octet rows (pad == 0, X8 * 8 == W:
// the gradient operand of every 64 / 128 / 256-pixel-wide layer): a workgroup converts 32 consecutive octets = 256
// consecutive pixels of 64 channels.  Loads are 16 bytes per lane and 1 KiB contiguous per wave (the general kernel
// reads 256-byte runs from 16 planes per thread: 2.6 TB/s); stores are the same 1 KiB slot rows.
// grid: (ceil(Hp * X8 / 32), Cp / 64, N)
__global__ __launch_bounds__(256) void split_transpose_vec_kernel(const SplitTParams p) {
    extern __shared__ float fv[];                    // [64][257]
    constexpr int LP = 257;
    const int cg = blockIdx.y, n = blockIdx.z, tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int HW = p.H * p.W, noct = p.Hp * p.X8;
    const int oct0 = blockIdx.x * 32;
    const SrcSeg sg = p.seg[0];
    {
        const int oct = oct0 + (lane >> 1);
        const int y = oct / p.X8, x = (oct - y * p.X8) * 8 + (lane & 1) * 4;
        const bool ok = oct < noct && y < p.H;       // (x < W by construction: X8 * 8 == W)
        const long long soff = (long long)y * p.W + x;
        float4 vv[16];                               // all loads first (see split_transpose_pad_kernel)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int c = cg * 64 + i * 4 + wave;
            vv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ok && c < p.C) vv[i] = *reinterpret_cast<const float4*>(sg.data + ((long long)n * sg.C + c) * HW + soff);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int cl = i * 4 + wave, c = cg * 64 + cl;
            float4 v = vv[i];
            if (ok && c < p.C) v = norm_act4(v, sg, n * sg.C + c);
            float* d = fv + cl * LP + lane * 4;
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
    }
    __syncthreads();
    const int c = lane;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int o = wave + 4 * k, oct = oct0 + o;
        if (oct < noct) {
            bf16x8 hv, lv;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                __bf16 h, l;
                split_bf16(fv[c * LP + o * 8 + j], h, l);
                hv[j] = h;
                lv[j] = l;
            }
            *reinterpret_cast<bf16x8*>(p.out + ((long long)(n * 2 + 0) * noct + oct) * p.Cp + cg * 64 + c) = hv;
            if (!p.heads_only) *reinterpret_cast<bf16x8*>(p.out + ((long long)(n * 2 + 1) * noct + oct) * p.Cp + cg * 64 + c) = lv;
        }
    }
}

// Row forms of split_transpose_kernel: a workgroup converts whole padded rows of 64 channels, so that every source row
// is read with 16-byte loads (1 KiB contiguous per wave in the interior) instead of 256-byte runs of 4-byte loads.
//
// (1) pad == 1 (reflection or zero), W in {32, 64, 128, 256}: R = 256 / W padded rows per workgroup; one wave-load
//     covers the R rows of one channel; the two border columns and the zero slots up to the octet boundary are written
//     by the lanes that hold the neighbouring values.            grid: (ceil(Hp / R), Cp / 64, N)
__device__ __forceinline__ void split_store_octets(const SplitTParams& p, const float* fv, int LP, int n, int cg, int oct0,
                                                   int nocts_tile, int wave, int lane) {
    const int noct = p.Hp * p.X8;
    for (int o = wave; o < nocts_tile; o += 4) {
        const int oct = oct0 + o;
        if (oct >= noct) break;
        bf16x8 hv, lv;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            __bf16 h, l;
            split_bf16(fv[lane * LP + o * 8 + j], h, l);
            hv[j] = h;
            lv[j] = l;
        }
        *reinterpret_cast<bf16x8*>(p.out + ((long long)(n * 2 + 0) * noct + oct) * p.Cp + cg * 64 + lane) = hv;
        if (!p.heads_only) *reinterpret_cast<bf16x8*>(p.out + ((long long)(n * 2 + 1) * noct + oct) * p.Cp + cg * 64 + lane) = lv;
    }
}

__global__ __launch_bounds__(256) void split_transpose_pad_kernel(const SplitTParams p) {
    extern __shared__ float fv[];                    // [64][R * X8 * 8 + 1]
    // (the wave index as a SCALAR: the channel a wave works on, its segment, base pointer and statistics then live in
    // SGPRs; left in a VGPR the compiler fetches the selected SrcSeg with vector loads and every iteration becomes a
    // chain of three dependent memory round trips)
    const int cg = blockIdx.y, n = blockIdx.z, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int LPR = p.W >> 2, R = 64 / LPR;          // lanes per row, rows per workgroup
    const int RS = p.X8 * 8, LP = R * RS + 1;        // slots per padded row, LDS row pitch
    const int He = p.H + 2, HW = p.H * p.W;
    const int y0 = blockIdx.x * R;
    {
        const int r = lane / LPR, xl = (lane - r * LPR) * 4;
        const int y = y0 + r;
        int sy = y - 1;
        bool ok = y < He;
        if (p.pad_mode == 1) sy = reflect_clamp(sy, p.H);
        else ok = ok && sy >= 0 && sy < p.H;
        const long long soff = ok ? (long long)sy * p.W + xl : 0;
        const bool refl = p.pad_mode == 1 && ok;
        // all 16 loads of the wave first (the compiler does not hoist them over the LDS stores on its own: one memory
        // round trip per channel otherwise), then the arithmetic and the LDS writes
        float4 v[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int c = cg * 64 + i * 4 + wave;
            v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c < p.C) {
                const int sgi = concat_seg(p.nseg, c, p.seg[1].chunk_begin, p.seg[2].chunk_begin);
                const float* base = (sgi == 0 ? p.seg[0].data : (sgi == 1 ? p.seg[1].data : p.seg[2].data));
                const int sc = sgi == 0 ? p.seg[0].C : (sgi == 1 ? p.seg[1].C : p.seg[2].C);
                const int cs = c - (sgi == 0 ? 0 : (sgi == 1 ? p.seg[1].chunk_begin : p.seg[2].chunk_begin));
                const int b16 = sgi == 0 ? p.seg[0].pad_ : (sgi == 1 ? p.seg[1].pad_ : p.seg[2].pad_);   // the segment holds bf16 values
                if (ok) {
                    if (b16) {
                        const uint2 t = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned short*>(base) + ((long long)n * sc + cs) * HW + soff);
                        v[i] = make_float4(__uint_as_float(t.x << 16), __uint_as_float(t.x & 0xffff0000u), __uint_as_float(t.y << 16),
                                           __uint_as_float(t.y & 0xffff0000u));
                    } else {
                        v[i] = *reinterpret_cast<const float4*>(base + ((long long)n * sc + cs) * HW + soff);
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int cl = i * 4 + wave, c = cg * 64 + cl;
            float4 w = v[i];
            if (c < p.C && ok) {
                const int sgi = concat_seg(p.nseg, c, p.seg[1].chunk_begin, p.seg[2].chunk_begin);
                const SrcSeg sg = sgi == 0 ? p.seg[0] : (sgi == 1 ? p.seg[1] : p.seg[2]);   // wave-uniform, scalar
                w = norm_act4(w, sg, n * sg.C + c - sg.chunk_begin);
            }
            float* d = fv + cl * LP + r * RS;
            d[1 + xl] = w.x; d[2 + xl] = w.y; d[3 + xl] = w.z; d[4 + xl] = w.w;
            if (xl == 0) d[0] = refl ? w.y : 0.f;                        // padded column 0 <- source column 1
            if (xl == p.W - 4) d[p.W + 1] = refl ? w.z : 0.f;            // padded column W + 1 <- source column W - 2
        }
        // the slots between the padded row's end and the octet boundary
        const int rsh = __ffs(R) - 1;
        for (int e = tid; e < 64 * R; e += 256) {
            float* d = fv + (e >> rsh) * LP + (e & (R - 1)) * RS;
            for (int z = p.W + 2; z < RS; ++z) d[z] = 0.f;
        }
    }
    __syncthreads();
    split_store_octets(p, fv, LP, n, cg, y0 * p.X8, R * p.X8, wave, lane);
}

// (2) the space-to-depth view (s2d_c = C0, C0 % 32 == 0, source W0 in {64, 128, 256}): a workgroup reads R = 256 / W0
//     source rows of equal parity of 32 source channels -- whole rows, every element used -- and writes both column
//     parities rx = 0, 1: view channels (ry * 2 + rx) * C0 + c of view rows y = (sy + 1 - ry) / 2.  The 64 LDS rows are
//     [rx][32 channels]; a wave-store is two 512-byte runs.
//     grid: (ceil(Hv / R) * 2 [ry], C0 / 32, N), Hv = H0 / 2 + 1 view rows (the operand has Hp >= Hv rows: the rest is
//     zero-filled by the workgroups of the last row group)
__global__ __launch_bounds__(256) void split_transpose_s2d_kernel(const SplitTParams p) {
    extern __shared__ float fv[];                    // [2 * 32][R * X8 * 8 + 1]
    const int n = blockIdx.z, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int C0 = p.s2d_c;
    const int LPR = p.W >> 2, R = 64 / LPR;
    const int RS = p.X8 * 8, LP = R * RS + 1;
    const int Hv = p.H / 2 + 1, Wv = p.W / 2 + 1, HW = p.H * p.W;
    const int ry = blockIdx.x & 1, y0 = (blockIdx.x >> 1) * R;
    const int cb = blockIdx.y * 32;
    const SrcSeg sg = p.seg[0];
    {
        const int r = lane / LPR, l = lane - r * LPR, xl = l * 4;
        const int y = y0 + r, sy = 2 * y + ry - 1;
        const bool ok = y < Hv && sy >= 0 && sy < p.H;
        const long long soff = ok ? (long long)sy * p.W + xl : 0;
        float4 vv[8];                                // all loads first (see split_transpose_pad_kernel)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            vv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ok) vv[i] = *reinterpret_cast<const float4*>(sg.data + ((long long)n * sg.C + cb + i * 4 + wave) * HW + soff);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int cl = i * 4 + wave, c = cb + cl;
            float4 v = vv[i];
            if (ok) v = norm_act4(v, sg, n * sg.C + c);
            // rx = 0: view column x <- source column 2x - 1 (odd columns; x = 0 is the zero border)
            float* d0 = fv + cl * LP + r * RS;
            d0[2 * l + 1] = v.y; d0[2 * l + 2] = v.w;
            // rx = 1: view column x <- source column 2x (even columns; x = W0 / 2 is the zero border)
            float* d1 = fv + (32 + cl) * LP + r * RS;
            d1[2 * l] = v.x; d1[2 * l + 1] = v.z;
            if (l == 0) d0[0] = 0.f;
            if (l == LPR - 1) {
                d1[Wv - 1] = 0.f;
                for (int z = Wv; z < RS; ++z) { d0[z] = 0.f; d1[z] = 0.f; }
            }
        }
    }
    __syncthreads();
    // thread = (rx, channel) of the 64 LDS rows; view channel (ry * 2 + rx) * C0 + cb + c
    const int noct = p.Hp * p.X8;
    const int rx = lane >> 5, c = lane & 31;
    const long long cofs = (long long)(ry * 2 + rx) * C0 + cb + c;
    for (int o = wave; o < R * p.X8; o += 4) {
        const int oct = y0 * p.X8 + o;
        if (oct >= noct) break;
        bf16x8 hv, lv;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            __bf16 h, l2;
            split_bf16(fv[lane * LP + o * 8 + j], h, l2);
            hv[j] = h;
            lv[j] = l2;
        }
        *reinterpret_cast<bf16x8*>(p.out + ((long long)(n * 2 + 0) * noct + oct) * p.Cp + cofs) = hv;
        if (!p.heads_only) *reinterpret_cast<bf16x8*>(p.out + ((long long)(n * 2 + 1) * noct + oct) * p.Cp + cofs) = lv;
    }
}

// ---- the same operand from the FORWARD pass's split copy.  The convolution that produced the layer's output staged
// XS[n][part][C/8][HW + 1][8 channels] (conv_prepass.h: act(IN(.)) applied, split, slot HW all-zero) of every source; it is
// still alive when the backward pass runs, and it holds exactly the values the operand needs -- so the operand is a
// re-tiling of 16-byte slots (8 channels of a pixel -> 8 pixels of a channel), not a second normalisation pass over the
// fp32 tensor: a thread loads the 8 slots of one pixel octet (padding = index arithmetic; out-of-image taps of a
// zero-padded layer read slot HW), transposes the 8 x 8 halfwords in registers (32 v_perm_b32) and stores 128 contiguous
// bytes.  No LDS, no statistics, bf16 in and out: 33 MB read + 39 MB written for a 256-channel 64 x 64 layer at B = 16
// in plain-bf16 mode, where split_transpose_pad_kernel reads 67 (bf16 source) .. 134 MB.
// The space-to-depth operand of a stride-2 layer comes the same way from ITS forward copy (ap_split_prepass_s2d: the
// view (4 C0, H0/2 + 1, W0/2 + 1), zero ring included): pad = 0 on the view.
// Lanes: 8 consecutive lanes own one pixel octet, lane e its pixel e -- a load instruction fetches 64 consecutive pixels'
// slots (1 KiB contiguous) and, after the transposition, lane c holds the octet's slot of channel c, so a store
// instruction writes whole 128-byte lines (8 channels x 16 bytes per octet).  The 8 x 8 halfword transposition runs
// ACROSS the 8 lanes as three butterfly exchanges (lane ^ 4 on dword pairs: ds_swizzle; lane ^ 2 on dwords and lane ^ 1
// on halfwords: DPP quad permutes + v_perm_b32).  (First form, one thread per (octet, channel octet) with a register
// transposition: every load and store instruction touched 64 different lines, 16 bytes of each -- 38 us per launch in
// the train step where this form takes ~20.)
// grid: (ceil(Hp * X8 / 32), ceil(Cp / 8 / 4), N): a workgroup = 32 pixel octets x 4 channel octets.
struct XsTParams {
    const uint4* xs[kMaxSeg];     // split copy of each source segment
    int cg_begin[kMaxSeg + 1];    // first channel octet of each segment; [nseg] = total octets (C / 8)
    int nseg;
    int N, H, W, pad, pad_mode, Hp, X8, Cp;
    int parts;                    // 1: head planes only
    int s2d_c, H0, W0;            // s2d_c = C0 > 0: the space-to-depth view (4 C0, H, W) = (.., H0/2 + 1, W0/2 + 1) gathered from the
                                  // PLAIN copy of the (C0, H0, W0) source (a stride-2 layer whose forward pass staged that one):
                                  // view channel r * C0 + c, pixel (y, x) = pad1(source)[c][2 y + (r >> 1)][2 x + (r & 1)]
    uint4* out;
};

constexpr int kXsCgPerThread = 4;

template <int XOR>
__device__ __forceinline__ unsigned lane_xor(unsigned v) {
    if constexpr (XOR == 4) return (unsigned)__builtin_amdgcn_ds_swizzle((int)v, 0x101F);               // bit mode: and 0x1f, xor 4
    else if constexpr (XOR == 2) return (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xF, 0xF, true);   // quad_perm [2,3,0,1]
    else return (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, true);                       // quad_perm [1,0,3,2]
}

__global__ __launch_bounds__(256) void xs_transpose_kernel(const XsTParams p) {
    const int tid = threadIdx.x, e = tid & 7;
    const int pos = blockIdx.x * 32 + (tid >> 3);
    if (pos >= p.Hp * p.X8) return;                                 // (whole 8-lane groups)
    const int n = blockIdx.z;
    const int y = pos / p.X8, k = pos - y * p.X8;
    const int HW = p.H * p.W, He = p.H + 2 * p.pad, We = p.W + 2 * p.pad;
    int idx;
    {
        const int x = k * 8 + e;
        int sy = y - p.pad, sx = x - p.pad;
        bool ok = y < He && x < We;
        if (p.pad_mode == 1) {
            sy = reflect_clamp(sy, p.H);
            sx = reflect_clamp(sx, p.W);
        } else {
            ok = ok && sy >= 0 && sy < p.H && sx >= 0 && sx < p.W;
        }
        idx = ok ? sy * p.W + sx : HW;                              // slot HW: zeros
    }
    const int total_cg = p.cg_begin[p.nseg];
    for (int part = 0; part < p.parts; ++part) {
        uint4 v[kXsCgPerThread];
#pragma unroll
        for (int i = 0; i < kXsCgPerThread; ++i) {
            const int cg = blockIdx.y * kXsCgPerThread + i;         // (block-uniform)
            v[i] = make_uint4(0u, 0u, 0u, 0u);
            if (cg < total_cg) {
                if (p.s2d_c > 0) {
                    const int CG0 = p.s2d_c >> 3, r = cg / CG0, cgl = cg - r * CG0, HW0 = p.H0 * p.W0;
                    const int yy = 2 * y + (r >> 1) - 1, xx = 2 * (k * 8 + e) + (r & 1) - 1;
                    const bool ok = y < p.H && k * 8 + e < p.W && yy >= 0 && yy < p.H0 && xx >= 0 && xx < p.W0;
                    v[i] = p.xs[0][((long long)(n * 2 + part) * CG0 + cgl) * (HW0 + 1) + (ok ? yy * p.W0 + xx : HW0)];
                    continue;
                }
                int s = 0;                                          // (concat_seg here, by value or by reference: 800 -> 798 / 790 instructions)
                if (p.nseg > 1 && cg >= p.cg_begin[1]) s = 1;
                if (p.nseg > 2 && cg >= p.cg_begin[2]) s = 2;
                const int CGs = p.cg_begin[s + 1] - p.cg_begin[s], cgl = cg - p.cg_begin[s];
                const uint4* src = s == 0 ? p.xs[0] : (s == 1 ? p.xs[1] : p.xs[2]);
                v[i] = src[((long long)(n * 2 + part) * CGs + cgl) * (HW + 1) + idx];
            }
        }
#pragma unroll
        for (int i = 0; i < kXsCgPerThread; ++i) {
            const int cg = blockIdx.y * kXsCgPerThread + i;
            if (cg * 8 >= p.Cp) continue;
            unsigned d0 = v[i].x, d1 = v[i].y, d2 = v[i].z, d3 = v[i].w;
            {   // lane ^ 4: dword pairs
                const bool hi = e & 4;
                const unsigned s0 = hi ? d0 : d2, s1 = hi ? d1 : d3;
                const unsigned r0 = lane_xor<4>(s0), r1 = lane_xor<4>(s1);
                if (hi) { d0 = r0; d1 = r1; } else { d2 = r0; d3 = r1; }
            }
            {   // lane ^ 2: dwords inside each pair
                const bool hi = e & 2;
                const unsigned s0 = hi ? d0 : d1, s1 = hi ? d2 : d3;
                const unsigned r0 = lane_xor<2>(s0), r1 = lane_xor<2>(s1);
                if (hi) { d0 = r0; d2 = r1; } else { d1 = r0; d3 = r1; }
            }
            {   // lane ^ 1: halfwords inside each dword.  even lane: (own.lo, other.lo); odd lane: (other.hi, own.hi)
                const bool hi = e & 1;
                const unsigned r0 = lane_xor<1>(d0), r1 = lane_xor<1>(d1), r2 = lane_xor<1>(d2), r3 = lane_xor<1>(d3);
                d0 = hi ? __builtin_amdgcn_perm(d0, r0, 0x07060302u) : __builtin_amdgcn_perm(r0, d0, 0x05040100u);
                d1 = hi ? __builtin_amdgcn_perm(d1, r1, 0x07060302u) : __builtin_amdgcn_perm(r1, d1, 0x05040100u);
                d2 = hi ? __builtin_amdgcn_perm(d2, r2, 0x07060302u) : __builtin_amdgcn_perm(r2, d2, 0x05040100u);
                d3 = hi ? __builtin_amdgcn_perm(d3, r3, 0x07060302u) : __builtin_amdgcn_perm(r3, d3, 0x05040100u);
            }
            // lane e now holds channel e of the octet: pixels 0..7
            p.out[(((long long)(n * 2 + part) * p.Hp + y) * p.X8 + k) * p.Cp + cg * 8 + e] = make_uint4(d0, d1, d2, d3);
        }
    }
}

}  // namespace apamd
