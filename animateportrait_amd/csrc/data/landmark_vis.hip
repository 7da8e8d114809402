// apd_landmark_vis: a batch of landmark sets drawn as coloured contours, the counterpart of vis_landmark
// (main_end2end_module2.py:47-68) and of the marked photo it leaves beside it (include/animateportrait_data.h).
//
// The shape of landmark_map_kernel: one workgroup per (frame, TH rows).  The clamped points, the integer description of
// every segment that can touch those rows (cv_raster.h; a segment that misses them gets an empty box) and the
// segments' colours as frame values are built once in LDS, one lane per segment.  Then every lane finds the primitive on
// top of its pixels by the backward scan of landmark_vis.h and stores the three planes: consecutive lanes write
// consecutive columns -- four columns per lane as one 16-byte store when the rows allow it -- every element of the output
// is written exactly once, nothing is accumulated in memory: neither a memset nor an atomic.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../../include/animateportrait_data.h"
#include "apd_common.h"
#include "landmark_vis.h"

namespace {

using apd::fail;
using namespace apd_raster;

constexpr int TH = 16, THREADS = 256;

struct VisArgs {
    const int32_t* pts;
    const int32_t* seg;
    const uint32_t* seg_rgb;
    const float* bg;
    float* out;
    int bg_shared, P, S, H, W, radius, thickness, rad;
    float disc[3], back[3];
    CircleRows disc_rows, cap;
};

// VEC columns per lane; 4 needs W % 4 == 0 and 16-byte aligned out / bg, which makes every row of every plane aligned
template <int VEC>
__global__ __launch_bounds__(THREADS) void landmark_vis_kernel(VisArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    Segment* segs = reinterpret_cast<Segment*>(smem);                                   // [S]
    int* pts = reinterpret_cast<int*>(smem + (size_t)a.S * sizeof(Segment));            // [P][2]
    float* col = reinterpret_cast<float*>(pts + 2 * a.P);                               // [S][3]
    const int n = blockIdx.y, row0 = blockIdx.x * TH, th = min(TH, a.H - row0);
    const int32_t* src = a.pts + (size_t)n * a.P * 2;
    for (int i = threadIdx.x; i < 2 * a.P; i += THREADS) pts[i] = clamp_coord(src[i]);
    __syncthreads();
    for (int s = threadIdx.x; s < a.S; s += THREADS) {
        const int ia = min(max(a.seg[2 * s], 0), a.P - 1), ib = min(max(a.seg[2 * s + 1], 0), a.P - 1);
        build_segment(segs[s], pts[2 * ia], pts[2 * ia + 1], pts[2 * ib], pts[2 * ib + 1], a.thickness, a.H, a.W, row0, row0 + th);
        const uint32_t rgb = a.seg_rgb[s];
        col[3 * s] = byte_level(rgb >> 16);
        col[3 * s + 1] = byte_level(rgb >> 8);
        col[3 * s + 2] = byte_level(rgb);
    }
    __syncthreads();
    const size_t plane = (size_t)a.H * a.W, first = (size_t)row0 * a.W;
    float* out = a.out + (size_t)n * 3 * plane + first;
    const float* bg = a.bg ? a.bg + (a.bg_shared ? 0 : (size_t)n * 3 * plane) + first : nullptr;
    const int wv = a.W / VEC;
    for (int e = threadIdx.x; e < th * wv; e += THREADS) {
        const int r = e / wv, x0 = (e - r * wv) * VEC, y = row0 + r;
        const size_t at = (size_t)r * a.W + x0;
        float v[3][VEC];
        for (int c = 0; c < 3; ++c) {
            if (!bg) {
                for (int j = 0; j < VEC; ++j) v[c][j] = a.back[c];
            } else if constexpr (VEC == 4) {
                const float4 q = *reinterpret_cast<const float4*>(bg + c * plane + at);
                v[c][0] = q.x; v[c][1] = q.y; v[c][2] = q.z; v[c][3] = q.w;
            } else {
                v[c][0] = bg[c * plane + at];
            }
        }
        for (int j = 0; j < VEC; ++j) {
            const int top = vis_top(pts, a.P, segs, a.S, a.disc_rows, a.radius, a.cap, a.rad, x0 + j, y);
            if (top == VIS_BACKGROUND) continue;
            for (int c = 0; c < 3; ++c) v[c][j] = top == VIS_DISC ? a.disc[c] : col[3 * top + c];
        }
        for (int c = 0; c < 3; ++c) {
            if constexpr (VEC == 4)
                *reinterpret_cast<float4*>(out + c * plane + at) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
            else
                out[c * plane + at] = v[c][0];
        }
    }
}

int check_vis(const int32_t* pts, const int32_t* seg, const int32_t* seg_host, const uint32_t* seg_rgb, const float* bg, int bg_frames,
              int N, int P, int S, int H, int W, int radius, int thickness, const float* out) {
    if (!pts || !out) return fail(APD_ERR_INVALID, "landmark_vis: null pts / out");
    if (N < 1 || N > 65535) return fail(APD_ERR_UNSUPPORTED, "landmark_vis: N = %ld, served: 1..65535", N);
    if (P < 1 || P > APD_MAX_POINTS) return fail(APD_ERR_UNSUPPORTED, "landmark_vis: P = %ld, served: 1..%ld", P, APD_MAX_POINTS);
    if (H < 1 || W < 1 || H > APD_MAX_MAP || W > APD_MAX_MAP)
        return fail(APD_ERR_UNSUPPORTED, "landmark_vis: frame %ld x %ld, served: 1..%ld per axis", H, W, APD_MAX_MAP);
    if (radius < -1 || radius > APD_MAX_RADIUS)
        return fail(APD_ERR_UNSUPPORTED, "landmark_vis: radius = %ld, served: -1 (no discs) and 0..%ld", radius, APD_MAX_RADIUS);
    if (thickness < 1 || thickness > APD_MAX_THICKNESS)
        return fail(APD_ERR_UNSUPPORTED, "landmark_vis: thickness = %ld, served: 1..%ld", thickness, APD_MAX_THICKNESS);
    if (S < 0 || S > APD_MAX_SEGMENTS) return fail(APD_ERR_UNSUPPORTED, "landmark_vis: S = %ld segments, served: 0..%ld", S, APD_MAX_SEGMENTS);
    if (S > 0) {
        if (!seg || !seg_host || !seg_rgb) return fail(APD_ERR_INVALID, "landmark_vis: %ld segments but no segment table / colours", S);
        for (int i = 0; i < 2 * S; ++i)
            if (seg_host[i] < 0 || seg_host[i] >= P)
                return fail(APD_ERR_INVALID, "landmark_vis: segment %ld names landmark %ld of %ld", i / 2, seg_host[i], P);
    }
    if (bg) {
        if (bg_frames != 1 && bg_frames != N)
            return fail(APD_ERR_INVALID, "landmark_vis: bg_frames = %ld, served: 1 (shared) and N = %ld", bg_frames, N);
        const uintptr_t frame = (uintptr_t)3 * H * W * sizeof(float), b0 = (uintptr_t)bg, o0 = (uintptr_t)out;
        if (b0 < o0 + (uintptr_t)N * frame && o0 < b0 + (uintptr_t)bg_frames * frame)
            return fail(APD_ERR_INVALID, "landmark_vis: bg overlaps out");
    }
    return APD_OK;
}

}  // namespace

extern "C" {

int32_t apd_landmark_vis_ok(const int32_t* pts, const int32_t* seg, const int32_t* seg_host, const uint32_t* seg_rgb,
                            const float* bg, int32_t bg_frames, int32_t N, int32_t P, int32_t S, int32_t H, int32_t W,
                            int32_t radius, int32_t thickness, uint32_t disc_rgb, uint32_t bg_rgb, const float* out) {
    (void)disc_rgb; (void)bg_rgb;                    // every colour is served: the low 24 bits are read
    return check_vis(pts, seg, seg_host, seg_rgb, bg, bg_frames, N, P, S, H, W, radius, thickness, out) == APD_OK ? 1 : 0;
}

int apd_landmark_vis(const int32_t* pts, const int32_t* seg, const int32_t* seg_host, const uint32_t* seg_rgb, const float* bg,
                     int32_t bg_frames, int32_t N, int32_t P, int32_t S, int32_t H, int32_t W, int32_t radius,
                     int32_t thickness, uint32_t disc_rgb, uint32_t bg_rgb, float* out, void* stream) {
    const int rc = check_vis(pts, seg, seg_host, seg_rgb, bg, bg_frames, N, P, S, H, W, radius, thickness, out);
    if (rc != APD_OK) return rc;
    VisArgs a;
    a.pts = pts; a.seg = seg; a.seg_rgb = seg_rgb; a.bg = bg; a.out = out;
    a.bg_shared = bg_frames == 1;
    a.P = P; a.S = S; a.H = H; a.W = W; a.radius = radius; a.thickness = thickness;
    a.rad = cap_radius(thickness);
    for (int c = 0; c < 3; ++c) {
        a.disc[c] = byte_level(disc_rgb >> (16 - 8 * c));
        a.back[c] = byte_level(bg_rgb >> (16 - 8 * c));
    }
    a.disc_rows = circle_rows(radius < 0 ? 0 : radius);        // radius -1: the rows are never read
    a.cap = circle_rows(a.rad);
    const size_t lds = (size_t)S * (sizeof(Segment) + 3 * sizeof(float)) + (size_t)2 * P * sizeof(int);   // <= 128 * 348 + 8192 bytes
    const bool wide = W % 4 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)bg % 16 == 0;
    const dim3 grid((H + TH - 1) / TH, N);
    (void)hipGetLastError();
    if (wide)
        hipLaunchKernelGGL(landmark_vis_kernel<4>, grid, dim3(THREADS), lds, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(landmark_vis_kernel<1>, grid, dim3(THREADS), lds, (hipStream_t)stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(apd::g_err, sizeof(apd::g_err), "landmark_vis: launch failed: %s", hipGetErrorString(e));
        return APD_ERR_LAUNCH;
    }
    return APD_OK;
}

}  // extern "C"
