// apd_landmark_map: draw2(op = 0 | 1) of the test-time item for a batch, and apd_landmark_marks: get_lmvis per sample
// (include/animateportrait_data.h).
//
// landmark_map: one workgroup per (sample, TH rows).  The rounded points and, for op 1, the integer description of every
// contour segment that can touch those rows (cv_raster.h) are built once in LDS, one lane per segment; then every
// lane tests its pixels against them and stores hi or lo -- consecutive lanes write consecutive columns, every element of
// the output is written exactly once, and nothing is accumulated in memory, so there is neither a memset nor an atomic.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../../include/animateportrait_data.h"
#include "apd_common.h"
#include "../cv_raster.h"

namespace {

using apd::fail;
using namespace apd_raster;

constexpr int TH = 16, THREADS = 256;
constexpr int MAX_HRADIUS = 64, MAX_MARKS_SIDE = 4096;

struct MapArgs {
    const float* lm;
    const int32_t* seg;
    float* out;
    int P, S, H, W, radius, thickness, rad;
    float lo, hi;
    CircleRows disc, cap;
};

__global__ __launch_bounds__(THREADS) void landmark_map_kernel(MapArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    Segment* segs = reinterpret_cast<Segment*>(smem);                      // [S]
    int* pts = reinterpret_cast<int*>(smem + (size_t)a.S * sizeof(Segment));   // [P][2]
    const int n = blockIdx.y, row0 = blockIdx.x * TH, th = min(TH, a.H - row0);
    const float* lm = a.lm + (size_t)n * a.P * 2;
    for (int i = threadIdx.x; i < 2 * a.P; i += THREADS) pts[i] = round_coord(lm[i]);
    __syncthreads();
    for (int s = threadIdx.x; s < a.S; s += THREADS) {
        const int ia = min(max(a.seg[2 * s], 0), a.P - 1), ib = min(max(a.seg[2 * s + 1], 0), a.P - 1);
        build_segment(segs[s], pts[2 * ia], pts[2 * ia + 1], pts[2 * ib], pts[2 * ib + 1], a.thickness, a.H, a.W, row0, row0 + th);
    }
    __syncthreads();
    float* out = a.out + ((size_t)n * a.H + row0) * a.W;
    for (int e = threadIdx.x; e < th * a.W; e += THREADS) {
        const int y = row0 + e / a.W, x = e % a.W;
        bool hit = false;
        for (int i = 0; i < a.P && !hit; ++i) hit = circle_covers(a.disc, a.radius, pts[2 * i], pts[2 * i + 1], x, y);
        for (int s = 0; s < a.S && !hit; ++s) hit = segment_covers(segs[s], a.cap, a.rad, x, y);
        out[e] = hit ? a.hi : a.lo;
    }
}

int check_map(const float* lm, const int32_t* seg, const int32_t* seg_host, const float* out, int N, int P, int S, int H, int W,
              int radius, int thickness, int op) {
    if (!lm || !out) return fail(APD_ERR_INVALID, "landmark_map: null lm / out");
    if (op != 0 && op != 1) return fail(APD_ERR_UNSUPPORTED, "landmark_map: op = %ld, served: 0 (discs) and 1 (discs and contour lines)", op);
    if (N < 1 || N > 65535) return fail(APD_ERR_UNSUPPORTED, "landmark_map: N = %ld, served: 1..65535", N);
    if (P < 1 || P > APD_MAX_POINTS) return fail(APD_ERR_UNSUPPORTED, "landmark_map: P = %ld, served: 1..%ld", P, APD_MAX_POINTS);
    if (H < 1 || W < 1 || H > APD_MAX_MAP || W > APD_MAX_MAP)
        return fail(APD_ERR_UNSUPPORTED, "landmark_map: map %ld x %ld, served: 1..%ld per axis", H, W, APD_MAX_MAP);
    if (radius < 0 || radius > APD_MAX_RADIUS) return fail(APD_ERR_UNSUPPORTED, "landmark_map: radius = %ld, served: 0..%ld", radius, APD_MAX_RADIUS);
    if (thickness < 1 || thickness > APD_MAX_THICKNESS)
        return fail(APD_ERR_UNSUPPORTED, "landmark_map: thickness = %ld, served: 1..%ld", thickness, APD_MAX_THICKNESS);
    if (S < 0 || S > APD_MAX_SEGMENTS) return fail(APD_ERR_UNSUPPORTED, "landmark_map: S = %ld segments, served: 0..%ld", S, APD_MAX_SEGMENTS);
    if (op == 1 && S > 0) {
        if (!seg || !seg_host) return fail(APD_ERR_INVALID, "landmark_map: op 1 with %ld segments but no segment table", S);
        for (int i = 0; i < 2 * S; ++i)
            if (seg_host[i] < 0 || seg_host[i] >= P)
                return fail(APD_ERR_INVALID, "landmark_map: segment %ld names landmark %ld of %ld", i / 2, seg_host[i], P);
    }
    return APD_OK;
}

// ---------------------------------------------------------------------------------------------------- get_lmvis
struct MarksArgs {
    const float* frames;
    const float* lm;
    const int32_t* win;
    float* out;
    int C, P, H, W, h;
};

__global__ __launch_bounds__(THREADS) void landmark_marks_kernel(MarksArgs a) {
    extern __shared__ int mpts[];          // [P][2] rounded landmarks, then the window
    const int n = blockIdx.y;
    for (int i = threadIdx.x; i < 2 * a.P; i += THREADS) mpts[i] = round_coord(a.lm[(size_t)n * a.P * 2 + i]);
    if (threadIdx.x < 4) mpts[2 * a.P + threadIdx.x] = a.win[4 * n + threadIdx.x];
    __syncthreads();
    const int p = blockIdx.x * THREADS + threadIdx.x;
    if (p >= a.H * a.W) return;
    const int y = p / a.W, x = p % a.W, h = a.h;
    bool hit = false;
    for (int i = 0; i < a.P && !hit; ++i) {
        const int px = mpts[2 * i], py = mpts[2 * i + 1];
        hit = y >= py - h && y < py + h && x >= px - h && x < px + h;
    }
    if (!hit) {
        // (long long: a hostile window must not overflow)
        const long long x1 = mpts[2 * a.P], x2 = mpts[2 * a.P + 1], y1 = mpts[2 * a.P + 2], y2 = mpts[2 * a.P + 3];
        const bool in_x = x >= x1 - h && x < x2 + h, in_y = y >= y1 - h && y < y2 + h;
        hit = (in_x && ((y >= y1 - h && y < y1 + h) || (y >= y2 - h && y < y2 + h))) ||
              (in_y && ((x >= x1 - h && x < x1 + h) || (x >= x2 - h && x < x2 + h)));
    }
    const size_t plane = (size_t)a.H * a.W;
    const float* f = a.frames + (size_t)n * a.C * plane + p;
    float* o = a.out + (size_t)n * 3 * plane + p;
    const float v0 = f[0], v1 = a.C == 3 ? f[plane] : v0, v2 = a.C == 3 ? f[2 * plane] : v0;
    o[0] = hit ? 1.f : v0;
    o[plane] = hit ? -1.f : v1;
    o[2 * plane] = hit ? -1.f : v2;
}

int check_marks(const float* frames, const float* lm, const int32_t* win, const float* out, int N, int C, int P, int H, int W,
                int hradius) {
    if (!frames || !lm || !win || !out) return fail(APD_ERR_INVALID, "landmark_marks: null frames / lm / win / out");
    if (C != 1 && C != 3) return fail(APD_ERR_UNSUPPORTED, "landmark_marks: C = %ld, served: 1 and 3", C);
    if (N < 1 || N > 65535) return fail(APD_ERR_UNSUPPORTED, "landmark_marks: N = %ld, served: 1..65535", N);
    if (P < 1 || P > APD_MAX_POINTS) return fail(APD_ERR_UNSUPPORTED, "landmark_marks: P = %ld, served: 1..%ld", P, APD_MAX_POINTS);
    if (H < 1 || W < 1 || H > MAX_MARKS_SIDE || W > MAX_MARKS_SIDE)
        return fail(APD_ERR_UNSUPPORTED, "landmark_marks: frame %ld x %ld, served: 1..%ld per axis", H, W, MAX_MARKS_SIDE);
    if (hradius < 0 || hradius > MAX_HRADIUS) return fail(APD_ERR_UNSUPPORTED, "landmark_marks: hradius = %ld, served: 0..%ld", hradius, MAX_HRADIUS);
    return APD_OK;
}

int launched(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(apd::g_err, sizeof(apd::g_err), "%s: launch failed: %s", what, hipGetErrorString(e));
        return APD_ERR_LAUNCH;
    }
    return APD_OK;
}

}  // namespace

extern "C" {

int32_t apd_landmark_map_ok(const float* lm, const int32_t* seg, const int32_t* seg_host, const float* out, int32_t N,
                            int32_t P, int32_t S, int32_t H, int32_t W, int32_t radius, int32_t thickness, int32_t op) {
    return check_map(lm, seg, seg_host, out, N, P, S, H, W, radius, thickness, op) == APD_OK ? 1 : 0;
}

int apd_landmark_map(const float* lm, const int32_t* seg, const int32_t* seg_host, int32_t N, int32_t P, int32_t S,
                     int32_t H, int32_t W, int32_t radius, int32_t thickness, int32_t op, float lo, float hi, float* out,
                     void* stream) {
    const int rc = check_map(lm, seg, seg_host, out, N, P, S, H, W, radius, thickness, op);
    if (rc != APD_OK) return rc;
    MapArgs a;
    a.lm = lm; a.seg = seg; a.out = out;
    a.P = P; a.S = op == 1 ? S : 0; a.H = H; a.W = W; a.radius = radius; a.thickness = thickness;
    a.rad = cap_radius(thickness);
    a.lo = lo; a.hi = hi;
    a.disc = circle_rows(radius);
    a.cap = circle_rows(a.rad);
    const size_t lds = (size_t)a.S * sizeof(Segment) + (size_t)2 * P * sizeof(int);     // <= 128 * 336 + 8192 bytes
    (void)hipGetLastError();
    hipLaunchKernelGGL(landmark_map_kernel, dim3((H + TH - 1) / TH, N), dim3(THREADS), lds, (hipStream_t)stream, a);
    return launched("landmark_map");
}

int32_t apd_landmark_marks_ok(const float* frames, const float* lm, const int32_t* win, const float* out, int32_t N,
                              int32_t C, int32_t P, int32_t H, int32_t W, int32_t hradius) {
    return check_marks(frames, lm, win, out, N, C, P, H, W, hradius) == APD_OK ? 1 : 0;
}

int apd_landmark_marks(const float* frames, const float* lm, const int32_t* win, int32_t N, int32_t C, int32_t P,
                       int32_t H, int32_t W, int32_t hradius, float* out, void* stream) {
    const int rc = check_marks(frames, lm, win, out, N, C, P, H, W, hradius);
    if (rc != APD_OK) return rc;
    MarksArgs a;
    a.frames = frames; a.lm = lm; a.win = win; a.out = out;
    a.C = C; a.P = P; a.H = H; a.W = W; a.h = hradius;
    (void)hipGetLastError();
    hipLaunchKernelGGL(landmark_marks_kernel, dim3((H * W + THREADS - 1) / THREADS, N), dim3(THREADS),
                       (size_t)(2 * P + 4) * sizeof(int), (hipStream_t)stream, a);
    return launched("landmark_marks");
}

}  // extern "C"
