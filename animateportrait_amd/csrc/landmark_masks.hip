// landmark_masks.hip -- the two OpenCV rasterisers of libapamd, on the per-pixel predicates of cv_raster.h (the project's
// one statement of OpenCV 4.2's integer drawing rules, shared with libapdata and run on the host under sanitizers by
// tools/raster_host_check.cpp):
//   draw2 op=0 (cv2.circle, filled)     Module2/data/umlvdfw_test_dataset.py:34-41        ap_landmark_discs, ap_circle_rows
//   getlipline (cv2.line(thickness))    Module2/models/geomgm_ifw_fore_model.py:507-515   ap_lip_line_mask
// Both kernels store every output element exactly once: no memset, no atomics, and work proportional to the canvas
// whatever the coordinates are (round_coord / trunc_coord clamp them; NaN lands on the clamp).
// Compiled with -ffp-contract=off: build_segment's rint(dy * r) is OpenCV's unfused product.
#include "common.h"
#include "cv_raster.h"

namespace apamd {

using namespace apd_raster;

// draw2(op=0): union of filled cv2.circle(radius) discs at np.round(lands), value hi on a lo canvas.
// grid: (ceil(H*W/256), N); lm: N x P x 2 (x, y)
__global__ __launch_bounds__(256) void landmark_discs_kernel(const float* __restrict__ lm, int P, int H, int W, int radius,
                                                             CircleRows rows, float lo, float hi, float* __restrict__ out) {
    extern __shared__ int pts[];           // P x 2 rounded coordinates
    const int n = blockIdx.y;
    for (int i = threadIdx.x; i < 2 * P; i += 256) pts[i] = round_coord(lm[(long long)n * P * 2 + i]);
    __syncthreads();
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= H * W) return;
    const int y = p / W, x = p % W;
    bool hit = false;
    for (int i = 0; i < P && !hit; ++i) hit = circle_covers(rows, radius, pts[2 * i], pts[2 * i + 1], x, y);
    out[(long long)n * H * W + p] = hit ? hi : lo;
}

// getlipline: the union of the segments drawn by cv2.line(mask, p0, p1, 255, thickness), thickness >= 2, LINE_8, the float
// coordinates truncated to int as the Python binding does.  One workgroup per (sample, TH rows), shaped like
// landmark_map_kernel: the truncated end points are staged in LDS, one lane per segment builds its integer description for
// those rows, then every lane tests its pixels and stores 1 or 0 -- consecutive lanes write consecutive columns.
// grid: (ceil(S/TH), N); lands: N x P x 2 (x, y)
constexpr int TH = 16, THREADS = 256, MAX_SEGS = 32;
struct LipSegs { int a[MAX_SEGS], b[MAX_SEGS]; };

__global__ __launch_bounds__(THREADS) void lip_mask_kernel(const float* __restrict__ lands, int P, LipSegs idx, int nseg, int S,
                                                           int thickness, int rad, CircleRows cap, float* __restrict__ out) {
    __shared__ Segment segs[MAX_SEGS];
    __shared__ int ends[MAX_SEGS][4];      // x0, y0, x1, y1
    const int n = blockIdx.y, row0 = blockIdx.x * TH, th = min(TH, S - row0);
    const float* l = lands + (size_t)n * P * 2;
    if (threadIdx.x < 4 * nseg) {
        const int s = threadIdx.x >> 2, k = threadIdx.x & 3;
        ends[s][k] = trunc_coord(l[2 * (k < 2 ? idx.a[s] : idx.b[s]) + (k & 1)]);
    }
    __syncthreads();
    if (threadIdx.x < nseg) {
        const int* e = ends[threadIdx.x];
        build_segment(segs[threadIdx.x], e[0], e[1], e[2], e[3], thickness, S, S, row0, row0 + th);
    }
    __syncthreads();
    float* o = out + ((size_t)n * S + row0) * S;
    for (int e = threadIdx.x; e < th * S; e += THREADS) {
        const int y = row0 + e / S, x = e % S;
        bool hit = false;
        for (int s = 0; s < nseg && !hit; ++s) hit = segment_covers(segs[s], cap, rad, x, y);
        o[e] = hit ? 1.f : 0.f;
    }
}

}  // namespace apamd

using namespace apamd;

extern "C" {

int ap_landmark_discs(const float* lm, int32_t N, int32_t P, int32_t H, int32_t W, int32_t radius, float lo, float hi,
                      float* out, ap_stream_t stream) {
    if (!lm || !out) return fail(AP_ERR_INVALID, "landmark_discs: null pointer");
    if (N < 1 || N > 65535 || P < 1 || P > 4096 || H < 1 || W < 1 || radius < 0 || radius > MAX_RADIUS)
        return fail(AP_ERR_INVALID, "landmark_discs: bad sizes (radius <= %d)", MAX_RADIUS);
    hipLaunchKernelGGL(landmark_discs_kernel, dim3((H * W + 255) / 256, N), dim3(256), 2 * P * sizeof(int),
                       (hipStream_t)stream, lm, P, H, W, radius, circle_rows(radius), lo, hi, out);
    return check_launch("landmark_discs_kernel");
}

int ap_lip_line_mask(const float* lands, int32_t N, int32_t P, const int32_t* seg_a, const int32_t* seg_b, int32_t nseg,
                     int32_t size, int32_t thickness, float* out, ap_stream_t stream) {
    if (!lands || !seg_a || !seg_b || !out) return fail(AP_ERR_INVALID, "lip_line_mask: null pointer");
    if (N < 1 || N > 65535 || P < 1 || nseg < 1 || nseg > MAX_SEGS || size < 1 || thickness < 2 || thickness > 16)
        return fail(AP_ERR_INVALID, "lip_line_mask: bad sizes (1..32 segments, thickness 2..16)");
    LipSegs sg;
    for (int i = 0; i < nseg; ++i) {
        if (seg_a[i] < 0 || seg_a[i] >= P || seg_b[i] < 0 || seg_b[i] >= P) return fail(AP_ERR_INVALID, "lip_line_mask: segment %d out of range", i);
        sg.a[i] = seg_a[i];
        sg.b[i] = seg_b[i];
    }
    const int rad = cap_radius(thickness);
    hipLaunchKernelGGL(lip_mask_kernel, dim3((size + TH - 1) / TH, N), dim3(THREADS), 0, (hipStream_t)stream, lands, P, sg, nseg,
                       size, thickness, rad, circle_rows(rad), out);
    return check_launch("lip_mask_kernel");
}

/* host-side table of the filled-circle rows (what ap_landmark_discs rasterises): hw[d], d = 0..radius */
int ap_circle_rows(int32_t radius, int32_t* hw) {
    if (!hw || radius < 0 || radius > MAX_RADIUS) return fail(AP_ERR_INVALID, "circle_rows: bad radius");
    const CircleRows t = circle_rows(radius);
    for (int i = 0; i <= radius; ++i) hw[i] = t.hw[i];
    return AP_OK;
}

}  // extern "C"
