// The detector's box arithmetic (include/animateportrait_face.h): candidates -> boxes, NMS, calibrate, square, round --
// float64 in numpy's operation order (compile with -ffp-contract=off), one workgroup per call.
//
// NMS is the reference's greedy loop restated: boxes are sorted ascending by (score, index) with a bitonic sort in LDS, then
// swept from the top; a box still alive is a pick, and the workgroup evaluates its overlap with every lower-ranked live box.
// Only the rows of the suppression matrix that belong to picks are ever needed, so they are evaluated inside the sweep and
// no n x n matrix is stored; the picks and their order equal the matrix-then-sweep formulation's.
// Scores are fp32 values in [0, 1] held in float64 (that is what the nets give): the sort key is the double's bit pattern
// with the index in its 12 low bits, which such doubles leave zero.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "face_checks.h"

namespace {

using apf::fail;
constexpr int THREADS = 1024;
constexpr int CAP = APF_CAP_SORT;
static_assert(CAP == 4096 && APF_CAP_LEVEL <= CAP && APF_CAP_MERGED <= CAP, "the key keeps the index in 12 bits");

struct Shared {
    uint64_t keys[CAP];
    int32_t picks[CAP];
    uint8_t alive[CAP];
    int32_t n;
};

__device__ __forceinline__ uint64_t score_key(double score, int index) {
    return ((uint64_t)__double_as_longlong(score) & ~(uint64_t)0xFFF) | (uint64_t)index;
}

// ascending bitonic sort of keys[0, n); the tail up to the next power of two is padded with the largest key
__device__ void block_sort(uint64_t* keys, int n) {
    int P = 1;
    while (P < n) P <<= 1;
    for (int i = n + threadIdx.x; i < P; i += THREADS) keys[i] = ~(uint64_t)0;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < P; i += THREADS) {
                const int o = i ^ j;
                if (o > i) {
                    const uint64_t a = keys[i], b = keys[o];
                    if ((a > b) == ((i & k) == 0)) {
                        keys[i] = b;
                        keys[o] = a;
                    }
                }
            }
            __syncthreads();
        }
}

__device__ __forceinline__ double overlap(const double* a, const double* b, int mode) {
    const double area_a = (a[2] - a[0] + 1.0) * (a[3] - a[1] + 1.0);
    const double area_b = (b[2] - b[0] + 1.0) * (b[3] - b[1] + 1.0);
    const double w = fmax(0.0, fmin(a[2], b[2]) - fmax(a[0], b[0]) + 1.0);
    const double h = fmax(0.0, fmin(a[3], b[3]) - fmax(a[1], b[1]) + 1.0);
    const double inter = w * h;
    return mode == APF_NMS_MIN ? inter / fmin(area_a, area_b) : inter / (area_a + area_b - inter);
}

// boxes: n rows of `stride` doubles whose column 4 is the score.  Leaves the picks in s.picks, returns their number.
__device__ int block_nms(Shared& s, const double* boxes, int stride, int n, double threshold, int mode) {
    for (int i = threadIdx.x; i < n; i += THREADS) {
        s.keys[i] = score_key(boxes[(size_t)i * stride + 4], i);
        s.alive[i] = 1;
    }
    __syncthreads();
    block_sort(s.keys, n);
    int np = 0;
    for (int r = n - 1; r >= 0; --r) {
        if (!s.alive[r]) continue;                      // uniform: written before the last barrier
        const int i = (int)(s.keys[r] & 0xFFF);
        if (threadIdx.x == 0) s.picks[np] = i;
        ++np;
        const double* a = boxes + (size_t)i * stride;
        for (int q = threadIdx.x; q < r; q += THREADS)
            if (s.alive[q] && overlap(a, boxes + (size_t)(s.keys[q] & 0xFFF) * stride, mode) > threshold) s.alive[q] = 0;
        __syncthreads();
    }
    __syncthreads();
    return np;
}

__global__ __launch_bounds__(THREADS) void stage1_level_kernel(const int32_t* cand_idx, const float* cand_score, const float* cand_off,
                                                                const int32_t* cand_count, int mw, double scale, double threshold,
                                                                double* cand_boxes, int32_t* level_count, double* merged,
                                                                int32_t* merged_count, int32_t* status) {
    __shared__ Shared s;
    const int found = *cand_count;
    const int n = min(max(found, 0), APF_CAP_LEVEL);
    const int base = min(max(*merged_count, 0), APF_CAP_MERGED);
    // row-major order, as np.where gives it
    for (int i = threadIdx.x; i < n; i += THREADS) s.keys[i] = ((uint64_t)(uint32_t)cand_idx[i] << 32) | (uint32_t)i;
    __syncthreads();
    block_sort(s.keys, n);
    for (int r = threadIdx.x; r < n; r += THREADS) {
        const int slot = (int)(s.keys[r] & 0xFFFFFFFFu), idx = (int)(s.keys[r] >> 32);
        const int iy = idx / mw, ix = idx % mw;
        double* b = cand_boxes + (size_t)r * 9;
        b[0] = rint((2 * ix + 1.0) / scale);
        b[1] = rint((2 * iy + 1.0) / scale);
        b[2] = rint((2 * ix + 1.0 + 12) / scale);
        b[3] = rint((2 * iy + 1.0 + 12) / scale);
        b[4] = (double)cand_score[slot];
        for (int c = 0; c < 4; ++c) b[5 + c] = (double)cand_off[(size_t)slot * 4 + c];
    }
    __syncthreads();
    const int np = block_nms(s, cand_boxes, 9, n, threshold, APF_NMS_UNION);
    const int room = APF_CAP_MERGED - base, take = min(np, room);
    for (int e = threadIdx.x; e < take * 9; e += THREADS) merged[(size_t)(base + e / 9) * 9 + e % 9] = cand_boxes[(size_t)s.picks[e / 9] * 9 + e % 9];
    if (threadIdx.x == 0) {
        *merged_count = base + take;
        if (level_count) *level_count = np;
        if (status) {
            int flags = 0;
            if (found > APF_CAP_LEVEL) flags |= APF_OVF_LEVEL;
            if (np > room) flags |= APF_OVF_MERGED;
            if (flags) atomicOr(status, flags);
        }
    }
}

struct StageArgs {
    const double* in;
    const int32_t* n_in;
    const float *probs, *offsets, *landmarks;
    double score_threshold, nms_threshold;
    double *out, *cal, *sq;
    float* out_landmarks;
    int32_t *n_out, *picks, *status;
    double *fb, *fo;            // workspace: filtered boxes (cap_in, 5), their offsets (cap_in, 4)
    float* flm;                 //            their landmarks (cap_in, 10)
    int32_t* src;               //            their row in `in`
    int in_stride, cap_in, cap_out, mode, late;
};

__global__ __launch_bounds__(THREADS) void box_stage_kernel(StageArgs a) {
    __shared__ Shared s;
    const int n0 = min(max(*a.n_in, 0), a.cap_in);
    // ordered filter: flags in parallel, one lane numbers the survivors
    for (int i = threadIdx.x; i < n0; i += THREADS) s.alive[i] = a.probs ? (a.probs[(size_t)i * 2 + 1] > (float)a.score_threshold) : 1;
    __syncthreads();
    if (threadIdx.x == 0) {
        int m = 0;
        for (int i = 0; i < n0; ++i)
            if (s.alive[i]) a.src[m++] = i;
        s.n = m;
    }
    __syncthreads();
    const int n = s.n;
    for (int k = threadIdx.x; k < n; k += THREADS) {
        const int i = a.src[k];
        const double* row = a.in + (size_t)i * a.in_stride;
        double b[5], o[4];
        for (int c = 0; c < 4; ++c) b[c] = row[c];
        b[4] = a.probs ? (double)a.probs[(size_t)i * 2 + 1] : row[4];
        for (int c = 0; c < 4; ++c) o[c] = a.offsets ? (double)a.offsets[(size_t)i * 4 + c] : (a.in_stride == 9 ? row[5 + c] : 0.0);
        if (a.late) {
            const double w = b[2] - b[0] + 1.0, h = b[3] - b[1] + 1.0;
            for (int c = 0; c < 5; ++c) {
                a.flm[(size_t)k * 10 + c] = (float)(b[0] + w * (double)a.landmarks[(size_t)i * 10 + c]);
                a.flm[(size_t)k * 10 + 5 + c] = (float)(b[1] + h * (double)a.landmarks[(size_t)i * 10 + 5 + c]);
            }
            b[0] = b[0] + w * o[0];
            b[1] = b[1] + h * o[1];
            b[2] = b[2] + w * o[2];
            b[3] = b[3] + h * o[3];
            if (a.cal)
                for (int c = 0; c < 5; ++c) a.cal[(size_t)k * 5 + c] = b[c];
        }
        for (int c = 0; c < 5; ++c) a.fb[(size_t)k * 5 + c] = b[c];
        for (int c = 0; c < 4; ++c) a.fo[(size_t)k * 4 + c] = o[c];
    }
    __syncthreads();
    const int np = block_nms(s, a.fb, 5, n, a.nms_threshold, a.mode);
    const int take = min(np, a.cap_out);
    for (int k = threadIdx.x; k < np; k += THREADS)
        if (a.picks) a.picks[k] = s.picks[k];
    for (int k = threadIdx.x; k < take; k += THREADS) {
        const int p = s.picks[k];
        double b[5];
        for (int c = 0; c < 5; ++c) b[c] = a.fb[(size_t)p * 5 + c];
        if (!a.late) {
            const double* o = a.fo + (size_t)p * 4;
            double w = b[2] - b[0] + 1.0, h = b[3] - b[1] + 1.0;
            b[0] = b[0] + w * o[0];
            b[1] = b[1] + h * o[1];
            b[2] = b[2] + w * o[2];
            b[3] = b[3] + h * o[3];
            if (a.cal)
                for (int c = 0; c < 5; ++c) a.cal[(size_t)k * 5 + c] = b[c];
            h = b[3] - b[1] + 1.0;
            w = b[2] - b[0] + 1.0;
            const double side = fmax(h, w);
            double q[5];
            q[0] = b[0] + w * 0.5 - side * 0.5;
            q[1] = b[1] + h * 0.5 - side * 0.5;
            q[2] = q[0] + side - 1.0;
            q[3] = q[1] + side - 1.0;
            q[4] = 0.0;                                   // convert_to_square starts from zeros and never sets the score
            if (a.sq)
                for (int c = 0; c < 5; ++c) a.sq[(size_t)k * 5 + c] = q[c];
            for (int c = 0; c < 4; ++c) b[c] = rint(q[c]);
            b[4] = q[4];
        } else if (a.out_landmarks) {
            for (int c = 0; c < 10; ++c) a.out_landmarks[(size_t)k * 10 + c] = a.flm[(size_t)p * 10 + c];
        }
        for (int c = 0; c < 5; ++c) a.out[(size_t)k * 5 + c] = b[c];
    }
    if (threadIdx.x == 0) {
        *a.n_out = take;
        if (a.status && np > a.cap_out) atomicOr(a.status, APF_OVF_STAGE);
    }
}

int launched(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return APF_OK;
    snprintf(apf::err_buf(), 256, "%s: launch failed: %s", what, hipGetErrorString(e));
    return APF_ERR_LAUNCH;
}

}  // namespace

extern "C" {

int32_t apf_stage1_level_ok(const int32_t* cand_idx, const int32_t* cand_count, int32_t mw, double scale, const double* cand_boxes,
                            const double* merged, const int32_t* merged_count) {
    return apf::check_stage1_level(cand_idx, cand_count, mw, scale, cand_boxes, merged, merged_count) == APF_OK ? 1 : 0;
}

int apf_stage1_level(const int32_t* cand_idx, const float* cand_score, const float* cand_off, const int32_t* cand_count, int32_t mw,
                     double scale, double nms_threshold, double* cand_boxes, int32_t* level_count, double* merged, int32_t* merged_count,
                     int32_t* status, void* stream) {
    const int rc = apf::check_stage1_level(cand_idx, cand_count, mw, scale, cand_boxes, merged, merged_count);
    if (rc != APF_OK) return rc;
    if (!cand_score || !cand_off) return fail(APF_ERR_INVALID, "stage1_level: null cand_score / cand_off");
    (void)hipGetLastError();
    hipLaunchKernelGGL(stage1_level_kernel, dim3(1), dim3(THREADS), 0, (hipStream_t)stream, cand_idx, cand_score, cand_off, cand_count, mw,
                       scale, nms_threshold, cand_boxes, level_count, merged, merged_count, status);
    return launched("stage1_level");
}

int64_t apf_box_stage_ws_bytes(int32_t cap_in) { return apf::box_stage_ws_bytes(cap_in); }

int32_t apf_box_stage_ok(const double* in, int32_t in_stride, const int32_t* n_in, int32_t cap_in, int32_t mode, int32_t late,
                         const float* landmarks, const double* out, const int32_t* n_out, int32_t cap_out, const void* ws) {
    return apf::check_box_stage(in, in_stride, n_in, cap_in, mode, late, landmarks, out, n_out, cap_out, ws) == APF_OK ? 1 : 0;
}

int apf_box_stage(const double* in, int32_t in_stride, const int32_t* n_in, int32_t cap_in, const float* probs, const float* offsets,
                  const float* landmarks, double score_threshold, double nms_threshold, int32_t mode, int32_t late, double* out,
                  float* out_landmarks, int32_t* n_out, int32_t cap_out, int32_t* picks, double* cal, double* sq, int32_t* status, void* ws,
                  void* stream) {
    const int rc = apf::check_box_stage(in, in_stride, n_in, cap_in, mode, late, landmarks, out, n_out, cap_out, ws);
    if (rc != APF_OK) return rc;
    StageArgs a;
    a.in = in; a.n_in = n_in; a.probs = probs; a.offsets = offsets; a.landmarks = landmarks;
    a.score_threshold = score_threshold; a.nms_threshold = nms_threshold;
    a.out = out; a.cal = cal; a.sq = sq; a.out_landmarks = out_landmarks; a.n_out = n_out; a.picks = picks; a.status = status;
    a.fb = (double*)ws;
    a.fo = a.fb + (size_t)cap_in * 5;
    a.flm = (float*)(a.fo + (size_t)cap_in * 4);
    a.src = (int32_t*)(a.flm + (size_t)cap_in * 10);
    a.in_stride = in_stride; a.cap_in = cap_in; a.cap_out = cap_out; a.mode = mode; a.late = late;
    (void)hipGetLastError();
    hipLaunchKernelGGL(box_stage_kernel, dim3(1), dim3(THREADS), 0, (hipStream_t)stream, a);
    return launched("box_stage");
}

}  // extern "C"
