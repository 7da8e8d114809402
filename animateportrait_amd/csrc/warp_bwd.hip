// warp_bwd.hip -- backward of the fused double_feature_warping (forward: warp_fwd.hip) w.r.t. x: the tap-by-tap scatter
// and its tiled form, which accumulates a tile's taps in LDS.
#include "warp_sample.h"
#include <climits>

namespace apamd {

// backward w.r.t. x only (motion / flow / mask carry no gradient: geomgm_ifw_fore_model.py:443-505 feeds
// them as data).  dx must be zero on entry; taps are scattered with fp32 atomics (L2).
__global__ __launch_bounds__(256) void warp_concat_bwd_kernel(const float* __restrict__ gout,
                                                              const float* __restrict__ motion,
                                                              const float* __restrict__ flow,
                                                              const float* __restrict__ ifmask, float* __restrict__ dx,
                                                              int C, int H, int W, int S, float flow_scale) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= H * W) return;
    const int n = blockIdx.z;
    const int oy = pix / W, ox = pix - oy * W;
    const long long SS = (long long)S * S;
    float gx, gy, fx, fy, mk;
    if (H == S && W == S) {
        const float2 g = reinterpret_cast<const float2*>(motion)[n * SS + pix];
        gx = g.x; gy = g.y;
        fx = flow[(n * 2 + 0) * SS + pix] * flow_scale;
        fy = flow[(n * 2 + 1) * SS + pix] * flow_scale;
        mk = ifmask[n * SS + pix];
    } else {
        const Lerp ly = make_lerp(oy, S, H), lx = make_lerp(ox, S, W);
        const int o00 = ly.i0 * S + lx.i0, o01 = ly.i0 * S + lx.i1, o10 = ly.i1 * S + lx.i0, o11 = ly.i1 * S + lx.i1;
        const float2* mo = reinterpret_cast<const float2*>(motion) + n * SS;
        const float2 a = mo[o00], b = mo[o01], c = mo[o10], d = mo[o11];
#ifdef APAMD_HZ_NOP
        asm volatile("s_nop 4" ::: "memory");       // co-residency lab, victim-side variant: idle states behind the four tap loads
#endif
        gx = bilerp(a.x, b.x, c.x, d.x, ly, lx);
        gy = bilerp(a.y, b.y, c.y, d.y, ly, lx);
        const float* f0 = flow + (n * 2 + 0) * SS;
        const float* f1 = flow + (n * 2 + 1) * SS;
        fx = bilerp(f0[o00] * flow_scale, f0[o01] * flow_scale, f0[o10] * flow_scale, f0[o11] * flow_scale, ly, lx);
        fy = bilerp(f1[o00] * flow_scale, f1[o01] * flow_scale, f1[o10] * flow_scale, f1[o11] * flow_scale, ly, lx);
        const float* mp = ifmask + n * SS;
        mk = bilerp(mp[o00], mp[o01], mp[o10], mp[o11], ly, lx);
    }
    const Taps tm = make_taps(gx, gy, H, W);
    const float wgx = 2.0f * ((float)ox + fx) / (float)(W - 1 > 1 ? W - 1 : 1) - 1.0f;
    const float wgy = 2.0f * ((float)oy + fy) / (float)(H - 1 > 1 ? H - 1 : 1) - 1.0f;
    const Taps tf = make_taps(wgx, wgy, H, W);
    const bool keep = mk > 0.5f;
    const int HW = H * W;
    const int c0 = blockIdx.y * kWarpCG;
    const int c1 = c0 + kWarpCG < C ? c0 + kWarpCG : C;
    for (int c = c0; c < c1; ++c) {
        float* plane = dx + ((long long)n * C + c) * HW;
        const float g1 = gout[((long long)n * 2 * C + c) * HW + pix];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (tm.off[k] >= 0) atomicAdd(plane + tm.off[k], g1 * tm.w[k]);
        if (keep) {
            const float g2 = gout[((long long)n * 2 * C + C + c) * HW + pix];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (tf.off[k] >= 0) atomicAdd(plane + tf.off[k], g2 * tf.w[k]);
        }
    }
}

// ---- tiled form of the same scatter.  Both sampling maps are smooth, so the taps of a 32 x 16 output tile land in a
// compact window of the input; the tile accumulates them in LDS for 8 channels at once and flushes every window element
// with ONE global atomic -- ~5x fewer L2 atomics than a tap-by-tap scatter, on contiguous rows.  Taps beyond the window
// (strong magnification, noise) scatter directly, as warp_concat_bwd_kernel does.
struct PixelTaps {
    int x0[2], y0[2];       // north-west tap of the motion sample / the flow sample
    float w[2][4];          // nw, ne, sw, se weights; 0 for out-of-range taps
    bool live;              // pixel inside the image
    bool keep;              // mask > 0.5: the flow branch carries gradient
};

__device__ __forceinline__ void taps_xy(float gx, float gy, int H, int W, int& x0, int& y0, float (&w)[4]) {
    float ix = ((gx + 1.f) * (float)W - 1.f) / 2.f;
    float iy = ((gy + 1.f) * (float)H - 1.f) / 2.f;
    ix = fminf(fmaxf(ix, -2.f), (float)W + 1.f);
    iy = fminf(fmaxf(iy, -2.f), (float)H + 1.f);
    const float fx = floorf(ix), fy = floorf(iy);
    x0 = (int)fx; y0 = (int)fy;
    const float ex = fx + 1.f, ey = fy + 1.f;
    const bool xin0 = x0 >= 0 && x0 < W, xin1 = x0 + 1 >= 0 && x0 + 1 < W;
    const bool yin0 = y0 >= 0 && y0 < H, yin1 = y0 + 1 >= 0 && y0 + 1 < H;
    w[0] = (xin0 && yin0) ? (ex - ix) * (ey - iy) : 0.f;
    w[1] = (xin1 && yin0) ? (ix - fx) * (ey - iy) : 0.f;
    w[2] = (xin0 && yin1) ? (ex - ix) * (iy - fy) : 0.f;
    w[3] = (xin1 && yin1) ? (ix - fx) * (iy - fy) : 0.f;
}

__device__ __forceinline__ PixelTaps pixel_taps(int n, int oy, int ox, const float* __restrict__ motion,
                                                const float* __restrict__ flow, const float* __restrict__ ifmask,
                                                int H, int W, int S, float flow_scale) {
    PixelTaps t;
    t.live = oy < H && ox < W;
    if (!t.live) {
        t.keep = false;
        t.x0[0] = t.x0[1] = t.y0[0] = t.y0[1] = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) t.w[0][k] = t.w[1][k] = 0.f;
        return t;
    }
    const long long SS = (long long)S * S;
    float gx, gy, fx, fy, mk;
    if (H == S && W == S) {
        const int pix = oy * W + ox;
        const float2 g = reinterpret_cast<const float2*>(motion)[n * SS + pix];
        gx = g.x; gy = g.y;
        fx = flow[(n * 2 + 0) * SS + pix] * flow_scale;
        fy = flow[(n * 2 + 1) * SS + pix] * flow_scale;
        mk = ifmask[n * SS + pix];
    } else {
        const Lerp ly = make_lerp(oy, S, H), lx = make_lerp(ox, S, W);
        const int o00 = ly.i0 * S + lx.i0, o01 = ly.i0 * S + lx.i1, o10 = ly.i1 * S + lx.i0, o11 = ly.i1 * S + lx.i1;
        const float2* mo = reinterpret_cast<const float2*>(motion) + n * SS;
        const float2 a = mo[o00], b = mo[o01], c = mo[o10], d = mo[o11];
#ifdef APAMD_HZ_NOP
        asm volatile("s_nop 4" ::: "memory");       // co-residency lab, victim-side variant: idle states behind the four tap loads
#endif
        gx = bilerp(a.x, b.x, c.x, d.x, ly, lx);
        gy = bilerp(a.y, b.y, c.y, d.y, ly, lx);
        const float* f0 = flow + (n * 2 + 0) * SS;
        const float* f1 = flow + (n * 2 + 1) * SS;
        fx = bilerp(f0[o00] * flow_scale, f0[o01] * flow_scale, f0[o10] * flow_scale, f0[o11] * flow_scale, ly, lx);
        fy = bilerp(f1[o00] * flow_scale, f1[o01] * flow_scale, f1[o10] * flow_scale, f1[o11] * flow_scale, ly, lx);
        const float* mp = ifmask + n * SS;
        mk = bilerp(mp[o00], mp[o01], mp[o10], mp[o11], ly, lx);
    }
    taps_xy(gx, gy, H, W, t.x0[0], t.y0[0], t.w[0]);
    const float wgx = 2.0f * ((float)ox + fx) / (float)(W - 1 > 1 ? W - 1 : 1) - 1.0f;
    const float wgy = 2.0f * ((float)oy + fy) / (float)(H - 1 > 1 ? H - 1 : 1) - 1.0f;
    taps_xy(wgx, wgy, H, W, t.x0[1], t.y0[1], t.w[1]);
    t.keep = mk > 0.5f;
    return t;
}

constexpr int kBwdTileW = 32, kBwdTileH = 16, kBwdPix = kBwdTileW * kBwdTileH;
constexpr int kBwdWin = 1344;       // window floats per channel (8 channels: 42 KiB; two workgroups per CU with the rest)
constexpr int kBwdWinW = 48;        // width of a clipped window
constexpr int kWarpBwdMaxH = 32757, kWarpBwdMaxW = 65525;    // what the 15 + 16 bits of s_xy hold (ap_warp_concat_bwd refuses more)

// ds_add_f32 retires about ONE LANE per clock per CU on gfx950 (measured: 537 M lane-atomics of the 256 x 256 level took
// 1.3 ms of the launch's 2.2 ms), against 32 lanes per clock for plain LDS reads / writes.  So the accumulation is done
// with plain read-modify-writes: each of the four waves OWNS two channel windows (no other wave touches them) and walks
// all 512 pixels of the tile, one tap (branch, corner) of all 512 pixels at a time.  Taps of one batch that hit the same
// window element are found with a claim word (write a unique id per (lane, pixel), read it back: exactly one writer
// wins): the winners' addresses are pairwise distinct, so their reads, adds and writes are issued as batches (two LDS
// round trips per 8 taps instead of one per tap); the rare losers use ds_add_f32 right after, in program order of the
// same wave.  (Measured on the 256 x 256 level, B = 32, smooth maps: 2.14 ms with ds_add_f32, 0.55 ms this way.)  The taps of the tile are computed once by the whole
// workgroup and handed to the waves through LDS.  When the taps' bounding box exceeds the window (noisy or magnifying
// maps) the window is the box's centre part and the taps outside it go to global memory one by one.
// Round 5: (a) the claims are resolved once per workgroup (wave w: batches 2w, 2w + 1; the result per tap in s_q) instead of by
// every wave, and the two channels of a wave are interleaved so that a tap is ONE 8-byte read-modify-write: 56 -> 32 LDS
// instructions per batch and wave; 1743 -> ~1630 us for the three levels of the train step.  (b) Tried and dropped: one window
// per sampling map when the box around both does not fit (the motion map may sample far from the tile): on the bench's maps --
// identity + WHITE noise of 2.5 px per pixel, boxes of 42 x 28 per map -- two half windows clip more taps than one whole one
// (256 x 256 level: 0.96 -> 1.31 ms); on smooth maps both forms take the single-window path (0.54 ms).  What the bench measures
// is the noise: a tile's 4096 taps collide and overflow the window whatever its shape.
// grid: (tiles_x * tiles_y, ceil(C/8), N)
__global__ __launch_bounds__(256) void warp_concat_bwd_tiled_kernel(const float* __restrict__ gout,
                                                                    const float* __restrict__ motion,
                                                                    const float* __restrict__ flow,
                                                                    const float* __restrict__ ifmask,
                                                                    float* __restrict__ dx, int C, int H, int W, int S,
                                                                    float flow_scale, int tiles_x) {
    __shared__ int s_box[4];
    __shared__ float2 win2[kWarpCG / 2][kBwdWin + 64];   // channel PAIRS interleaved (+ 64: a trash element per lane)
    __shared__ int s_xy[2][kBwdPix];                 // (y0 + 8) << 16 | (x0 + 8) of the north-west tap; bit 31: branch live
    __shared__ float s_w[2][4][kBwdPix];             // tap weights: > 0 inside the window, < 0 (negated) outside, 0 dead
    __shared__ unsigned short s_q[8][kBwdPix];       // per batch: the window element a tap adds to (trash: dead, outside, or lost its claim)
    // logical block (tile fastest, then channel group, then image) contiguous per XCD, as in the forward kernel: the tiles whose
    // windows overlap -- and whose flushes add into the same lines of dx -- run on one XCD
    int bx, by, bz;
    {
        const unsigned L = xcd_logical_block(gridDim.x * gridDim.y * gridDim.z,
                                             blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z));
        bx = L % gridDim.x;
        const unsigned t = L / gridDim.x;
        by = t % gridDim.y;
        bz = t / gridDim.y;
    }
    const int tid = threadIdx.x, n = bz, wave = tid >> 6, lane = tid & 63;
    const int ty0 = (bx / tiles_x) * kBwdTileH, tx0 = (bx % tiles_x) * kBwdTileW;
    if (tid == 0) { s_box[0] = W; s_box[1] = H; s_box[2] = -1; s_box[3] = -1; }
    __syncthreads();
    PixelTaps pt[2];
    {
        int xmin = W, ymin = H, xmax = -1, ymax = -1;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int p = tid + 256 * j;
            pt[j] = pixel_taps(n, ty0 + (p >> 5), tx0 + (p & 31), motion, flow, ifmask, H, W, S, flow_scale);
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const bool on = pt[j].live && (b == 0 || pt[j].keep);
                float ws = 0.f;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (!on) pt[j].w[b][k] = 0.f;
                    ws += pt[j].w[b][k];
                }
                if (!(ws != 0.f)) continue;                              // every tap out of range
                const int xa = pt[j].x0[b] < 0 ? 0 : pt[j].x0[b], xb = pt[j].x0[b] + 1 >= W ? W - 1 : pt[j].x0[b] + 1;
                const int ya = pt[j].y0[b] < 0 ? 0 : pt[j].y0[b], yb = pt[j].y0[b] + 1 >= H ? H - 1 : pt[j].y0[b] + 1;
                xmin = xa < xmin ? xa : xmin; xmax = xb > xmax ? xb : xmax;
                ymin = ya < ymin ? ya : ymin; ymax = yb > ymax ? yb : ymax;
            }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            xmin = min(xmin, __shfl_xor(xmin, m)); ymin = min(ymin, __shfl_xor(ymin, m));
            xmax = max(xmax, __shfl_xor(xmax, m)); ymax = max(ymax, __shfl_xor(ymax, m));
        }
        if (lane == 0 && xmax >= 0) {
            atomicMin(&s_box[0], xmin); atomicMin(&s_box[1], ymin);
            atomicMax(&s_box[2], xmax); atomicMax(&s_box[3], ymax);
        }
    }
    __syncthreads();
    if (s_box[2] < 0) return;                                            // the tile scatters nothing
    int bx0 = s_box[0], by0 = s_box[1];
    int bw = s_box[2] - bx0 + 1, bh = s_box[3] - by0 + 1;
    if (bw * bh > kBwdWin) {                                             // keep the centre of the box
        const int nw = bw < kBwdWinW ? bw : kBwdWinW;
        const int nh = bh < kBwdWin / nw ? bh : kBwdWin / nw;
        bx0 += (bw - nw) / 2; by0 += (bh - nh) / 2;
        bw = nw; bh = nh;
    }
    const int c0 = by * kWarpCG;
    const int nc = c0 + kWarpCG <= C ? kWarpCG : C - c0;
    const int HW = H * W, area = bw * bh;
    // the taps in window terms, so that the walk below spends a handful of VALU instructions per tap (it is VALU-bound)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int p = tid + 256 * j;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int x0 = pt[j].x0[b] - bx0, y0 = pt[j].y0[b] - by0;
            bool any = false;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float wk = pt[j].w[b][k];
                const bool inside = (unsigned)(x0 + (k & 1)) < (unsigned)bw && (unsigned)(y0 + (k >> 1)) < (unsigned)bh;
                s_w[b][k][p] = inside ? wk : -wk;
                any |= wk != 0.f;
            }
            s_xy[b][p] = ((pt[j].y0[b] + 8) << 16) | (pt[j].x0[b] + 8) | (any ? (int)0x80000000 : 0);
        }
    }
    __syncthreads();
    // ---- the claims, ONCE per workgroup: every wave walks the 512 pixels in the same (lane, i) order, so which taps of a batch
    // collide is the same for all of them.  Wave w resolves batches 2w and 2w + 1 and leaves, per tap, the element it may add to
    // with a plain read-modify-write (s_q).  (The claim words live in the window's memory, which is cleared afterwards.)
    constexpr int NI = kBwdPix / 64;
    const int trash = kBwdWin + lane;        // window element nobody reads: where dead taps and claim losers write
    {
        typedef __attribute__((address_space(3))) volatile unsigned short lds_vu16;
        lds_vu16* claim = (lds_vu16*)(reinterpret_cast<unsigned short*>(&win2[0][0]) + wave * (kBwdWin + 64));
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int bk = 2 * wave + h, b = bk >> 2, k = bk & 3;
            const int off = (k & 1) + (k >> 1) * bw;
            int a[NI];
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int p = i * 64 + lane;
                const int v = s_xy[b][p];
                const int a0 = (((v >> 16) & 0x7fff) - 8 - by0) * bw + (v & 0xffff) - 8 - bx0;
                a[i] = s_w[b][k][p] > 0.f ? a0 + off : trash;
            }
#pragma unroll
            for (int i = 0; i < NI; ++i) claim[a[i]] = (unsigned short)(lane * NI + i);
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const bool own = claim[a[i]] == (unsigned short)(lane * NI + i);   // (a lane always owns its trash element)
                s_q[bk][i * 64 + lane] = (unsigned short)(own ? a[i] : trash);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < kWarpCG / 2; ++c)
        for (int i = tid; i < area; i += 256) win2[c][i] = make_float2(0.f, 0.f);
    __syncthreads();
    // ---- this wave's two channels over the whole tile: one 8-byte read-modify-write per tap (ds_read_b64 costs what
    // ds_read_b32 does, ds_write_b64 6 LDS cycles against 2 x 4: MI355X_MICROARCH, LDS table)
    const int ca = 2 * wave, cb = 2 * wave + 1;
    if (ca < nc) {
        const bool two = cb < nc;
        // (address-space-3 pointers: through a generic volatile pointer these accesses become FLAT loads / stores)
        typedef __attribute__((address_space(3))) volatile unsigned long long lds_vu64;     // (one 8-byte access per element)
        lds_vu64* wab = (lds_vu64*)&win2[wave][0];
        const float* ga = gout + ((long long)n * 2 * C + c0 + ca) * HW;
        float* pa = dx + ((long long)n * C + c0 + ca) * HW;
        // every gradient value of the wave's walk is requested up front (8 pixels x 2 branches x 2 channels per lane)
        int a0[NI][2];
        float g0[NI][2], g1[NI][2];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int p = i * 64 + lane;
            const int pix = (ty0 + (p >> 5)) * W + tx0 + (p & 31);       // (only dereferenced when the branch is live)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int v = s_xy[b][p];
                a0[i][b] = (((v >> 16) & 0x7fff) - 8 - by0) * bw + (v & 0xffff) - 8 - bx0;
                g0[i][b] = g1[i][b] = 0.f;
                if (v < 0) {                                             // bit 31: some tap of the branch is in range
                    g0[i][b] = ga[(long long)b * C * HW + pix];
                    if (two) g1[i][b] = ga[((long long)b * C + 1) * HW + pix];
                }
            }
        }
        // one batch = tap (b, k) of the lane's 8 pixels (8 different row pairs of the tile: for a locally injective map
        // the 512 addresses of a batch are distinct; taps k and k' of NEIGHBOURING pixels coincide all the time, which
        // is why a batch never mixes them)
#pragma unroll
        for (int bk = 0; bk < 8; ++bk) {
            const int b = bk >> 2, k = bk & 3;
            const int off = (k & 1) + (k >> 1) * bw;
            int q[NI];
            float va[NI], vb[NI];
            float wmin = 0.f;
            bool lost = false;
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const float wk = s_w[b][k][i * 64 + lane];
                q[i] = s_q[bk][i * 64 + lane];
                va[i] = g0[i][b] * wk;
                vb[i] = g1[i][b] * wk;
                wmin = fminf(wmin, wk);
                lost |= wk > 0.f && q[i] == trash;                       // inside the window, but another tap of the batch owns the element
            }
            if (wmin < 0.f) {                                            // taps beyond a clipped window: one by one
#pragma unroll
                for (int i = 0; i < NI; ++i)
                    if (s_w[b][k][i * 64 + lane] < 0.f) {
                        const int v = s_xy[b][i * 64 + lane];
                        const int x = (v & 0xffff) - 8 + (k & 1), y = ((v >> 16) & 0x7fff) - 8 + (k >> 1);
                        atomicAdd(pa + y * W + x, -va[i]);
                        if (two) atomicAdd(pa + HW + y * W + x, -vb[i]);
                    }
            }
            unsigned long long r[NI];
#pragma unroll
            for (int i = 0; i < NI; ++i) r[i] = wab[q[i]];
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const float sa = __uint_as_float((unsigned)r[i]) + va[i], sb = __uint_as_float((unsigned)(r[i] >> 32)) + vb[i];
                wab[q[i]] = (unsigned long long)__float_as_uint(sa) | ((unsigned long long)__float_as_uint(sb) << 32);
            }
            if (lost) {
#pragma unroll
                for (int i = 0; i < NI; ++i)
                    if (s_w[b][k][i * 64 + lane] > 0.f && q[i] == trash) {
                        atomicAdd(&win2[wave][a0[i][b] + off].x, va[i]);
                        if (two) atomicAdd(&win2[wave][a0[i][b] + off].y, vb[i]);
                    }
            }
        }
    }
    __syncthreads();
    // (no integer divisions in this loop: at ~40 VALU instructions each they cost more than the stores)
    const float inv_bw = 1.0f / (float)bw;
    for (int r = tid; r < area; r += 256) {
        const int y = (int)(((float)r + 0.5f) * inv_bw);                 // == r / bw for r < 2^20
        float* q = dx + ((long long)n * C + c0) * HW + (by0 + y) * W + bx0 + (r - y * bw);
        for (int c = 0; c < nc; c += 2) {
            const float2 v = win2[c >> 1][r];
            if (v.x != 0.f) atomicAdd(q + (long long)c * HW, v.x);
            if (c + 1 < nc && v.y != 0.f) atomicAdd(q + (long long)(c + 1) * HW, v.y);
        }
    }
}

}  // namespace apamd

using namespace apamd;

extern "C" int ap_warp_concat_bwd(const float* gout, const float* motion, const float* flow, const float* ifmask,
                                  float* dx, int32_t N, int32_t C, int32_t H, int32_t W, int32_t S, float flow_scale,
                                  ap_stream_t stream) {
    if (!gout || !motion || !flow || !ifmask || !dx) return fail(AP_ERR_INVALID, "warp_concat_bwd: null pointer");
    if (N < 1 || C < 1 || H < 1 || W < 1 || S < 1 || N > 65535) return fail(AP_ERR_INVALID, "warp_concat_bwd: bad sizes");
    // the tiled kernel packs (y0 + 8) << 16 | (x0 + 8) of a north-west tap (y0 <= H + 1, x0 <= W + 1) under a flag in bit 31,
    // and both kernels index a plane with an int
    if (H > kWarpBwdMaxH || W > kWarpBwdMaxW)
        return fail(AP_ERR_UNSUPPORTED, "warp_concat_bwd: H <= %d and W <= %d are served (got %d x %d)", kWarpBwdMaxH, kWarpBwdMaxW, H, W);
    if ((long long)H * W > INT_MAX / 2)
        return fail(AP_ERR_UNSUPPORTED, "warp_concat_bwd: H * W <= %d is served (got %d x %d)", INT_MAX / 2, H, W);
    hipError_t e = hipMemsetAsync(dx, 0, (size_t)N * C * H * W * sizeof(float), (hipStream_t)stream);
    if (e != hipSuccess) return fail(AP_ERR_LAUNCH, "warp_concat_bwd memset: %s", hipGetErrorString(e));
    if (sw(SW_WARP_BWD_PLAIN)) {   // tap-by-tap scatter (kept for comparison); read per call
        hipLaunchKernelGGL(warp_concat_bwd_kernel, warp_grid((H * W + 255) / 256, C, N), dim3(256), 0, (hipStream_t)stream, gout,
                           motion, flow, ifmask, dx, C, H, W, S, flow_scale);
        return check_launch("warp_concat_bwd_kernel");
    }
    const int tiles_x = (W + kBwdTileW - 1) / kBwdTileW, tiles_y = (H + kBwdTileH - 1) / kBwdTileH;
    hipLaunchKernelGGL(warp_concat_bwd_tiled_kernel, warp_grid(tiles_x * tiles_y, C, N), dim3(256), 0, (hipStream_t)stream, gout,
                       motion, flow, ifmask, dx, C, H, W, S, flow_scale, tiles_x);
    return check_launch("warp_concat_bwd_tiled_kernel");
}
