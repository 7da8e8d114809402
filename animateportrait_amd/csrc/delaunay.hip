// delaunay.hip -- Delaunay triangulation of small planar point sets on the device (ap_delaunay): the triangulation half
// of cal_motion256 (scipy.spatial.Delaunay inside griddata, Module2/data/umlvd_ifw_dataset.py:60-74), so that the
// landmarks of a frame never visit the host.  The contract (include/animateportrait_amd.h) makes the result unique:
// bit-equal later points are dead, a triple is emitted iff its open circumdisc is empty of live points and, where live
// points lie exactly on the circle, the cocircular polygon is fanned from its lowest-index vertex; rows ascending.
//
// One workgroup per point set, everything in LDS, the edge form:
//   1. every live pair (a, b) scans the live points once and keeps, on each side of the line, the apex that subtends the
//      largest angle (the only apex whose circle through a and b can be empty on that side; among apexes on one circle the
//      one next to b).  An apex c > b whose circle does not contain the other side's apex is a candidate (a, b, c);
//   2. the candidates are compacted in pair order (block scan, no atomics: the order is the lexicographic one);
//   3. every candidate is put to the WHOLE contract against all live points -- steps 1-2 only decide what is looked at,
//      never what is emitted;
//   4. the survivors are compacted again and written; rows past the count are -1.
// Predicates are fp64 on coordinate differences, with mul / add unfused (Makefile: -ffp-contract=off), so that a host
// restatement in numpy evaluates the same expressions to the same bits.
#include "common.h"

namespace apamd {

constexpr int kDelMaxP = 128;                               // points per set served
constexpr int kDelThreads = 1024;
constexpr int kDelMaxSlots = kDelMaxP * (kDelMaxP - 1);     // two apexes per pair
constexpr int kDelNone = 0xFF;                              // empty apex slot (point indices are < 128)

// > 0: r lies to the left of p -> q (in the (first, second) coordinate frame); 0: collinear
__device__ __forceinline__ double del_orient(double px, double py, double qx, double qy, double rx, double ry) {
    return (qx - px) * (ry - py) - (qy - py) * (rx - px);
}
// the 3x3 in-circle determinant of a, b, c relative to the query point d: its sign times the sign of orient(a, b, c) is
// > 0 iff d lies strictly inside the circle through a, b, c, and it is 0 iff d lies on it
__device__ __forceinline__ double del_incircle(double ax, double ay, double bx, double by, double cx, double cy, double dx,
                                               double dy) {
    ax -= dx; ay -= dy; bx -= dx; by -= dy; cx -= dx; cy -= dy;
    const double al = ax * ax + ay * ay, bl = bx * bx + by * by, cl = cx * cx + cy * cy;
    return ax * (by * cl - bl * cy) - ay * (bx * cl - bl * cx) + al * (bx * cy - by * cx);
}
// pair number k of L points, pairs (a, b), a < b, counted in lexicographic order
__device__ __forceinline__ void del_pair(int k, int L, int& a, int& b) {
    a = 0;
    while (k >= L - 1 - a) {
        k -= L - 1 - a;
        ++a;
    }
    b = a + 1 + k;
}
// exclusive prefix sum of one value per thread over the workgroup (thread order); *total = the sum.  wsum: 17 ints of LDS
__device__ __forceinline__ int del_scan(int v, int* wsum, int tid, int* total) {
    const int lane = tid & 63, w = tid >> 6;
    int x = v;
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    if (tid == 0) {
        int s = 0;
        for (int i = 0; i < kDelThreads / 64; ++i) {
            const int t = wsum[i];
            wsum[i] = s;
            s += t;
        }
        wsum[kDelThreads / 64] = s;
    }
    __syncthreads();
    const int r = x - v + wsum[w];
    *total = wsum[kDelThreads / 64];
    __syncthreads();                                         // wsum is free again
    return r;
}

// pts: [N][P][2]; tri: [N][Tcap][3]; count: [N].   grid: N, block: kDelThreads.   3 <= P <= kDelMaxP, Tcap >= 1
__global__ __launch_bounds__(kDelThreads) void delaunay_kernel(const float* __restrict__ pts, int P, int Tcap,
                                                               int* __restrict__ tri, int* __restrict__ count) {
    __shared__ double sx[kDelMaxP], sy[kDelMaxP];            // live points, compacted in index order
    __shared__ unsigned rx[kDelMaxP], ry[kDelMaxP];          // raw coordinate bits of all points
    __shared__ unsigned char live[kDelMaxP], orig[kDelMaxP]; // orig: compacted position -> point index
    __shared__ unsigned char cand[kDelMaxSlots];             // per pair: up to two apexes > b, ascending, then kDelNone
    __shared__ unsigned short list[kDelMaxSlots];            // compacted candidate slots; 0xFFFF once refuted
    __shared__ int wsum[kDelThreads / 64 + 1];
    __shared__ int nlive;
    const int n = blockIdx.x, tid = threadIdx.x;
    int* const trin = tri + (long long)n * Tcap * 3;

    // ---- live points: a point bit-equal to an earlier one is dead
    if (tid < P) {
        rx[tid] = __float_as_uint(pts[((long long)n * P + tid) * 2]);
        ry[tid] = __float_as_uint(pts[((long long)n * P + tid) * 2 + 1]);
    }
    __syncthreads();
    if (tid < P) {
        bool l = true;
        for (int j = 0; j < tid; ++j) l = l && !(rx[j] == rx[tid] && ry[j] == ry[tid]);
        live[tid] = l;
    }
    __syncthreads();
    if (tid < P) {
        int pos = 0;
        for (int j = 0; j < tid; ++j) pos += live[j];
        if (live[tid]) {
            orig[pos] = (unsigned char)tid;
            sx[pos] = (double)__uint_as_float(rx[tid]);
            sy[pos] = (double)__uint_as_float(ry[tid]);
        }
        if (tid == P - 1) nlive = pos + live[tid];
    }
    __syncthreads();
    const int L = nlive;
    const int npairs = L * (L - 1) / 2, nslots = 2 * npairs;
    int total = 0;
    if (L >= 3) {
        // ---- 1. per pair: the apex of the largest subtended angle on each side
        for (int k = tid; k < npairs; k += kDelThreads) {
            int a, b;
            del_pair(k, L, a, b);
            const double ax = sx[a], ay = sy[a], bx = sx[b], by = sy[b];
            int bp = -1, bn = -1;                            // best apex left / right of a -> b
            for (int d = 0; d < L; ++d) {
                if (d == a || d == b) continue;
                const double dx = sx[d], dy = sy[d];
                const double o = del_orient(ax, ay, bx, by, dx, dy);
                if (!(o > 0.0) && !(o < 0.0)) continue;      // on the line: no apex
                const bool left = o > 0.0;
                const int cur = left ? bp : bn;
                bool take = cur < 0;
                if (!take) {
                    const double cx = sx[cur], cy = sy[cur];
                    const double det = del_incircle(ax, ay, bx, by, cx, cy, dx, dy);
                    if (left ? det > 0.0 : det < 0.0) {
                        take = true;                         // strictly inside the current apex's circle: larger angle
                    } else if (det == 0.0) {                 // same circle: the one nearer to b along the arc
                        const double od = del_orient(bx, by, cx, cy, dx, dy), oa = del_orient(bx, by, cx, cy, ax, ay);
                        take = (od > 0.0 && oa < 0.0) || (od < 0.0 && oa > 0.0);
                    }
                }
                if (take) {
                    if (left) bp = d; else bn = d;
                }
            }
            int c0 = kDelNone, c1 = kDelNone;
            for (int s = 0; s < 2; ++s) {
                const int c = s ? bn : bp, e = s ? bp : bn;
                bool ok = c > b;                             // a triangle is emitted by its two lowest vertices
                if (ok && e >= 0) {                          // the far apex inside this circle: (a, b) is no edge
                    const double o = del_orient(ax, ay, bx, by, sx[c], sy[c]);
                    const double det = del_incircle(ax, ay, bx, by, sx[c], sy[c], sx[e], sy[e]);
                    ok = !((o > 0.0 ? det : -det) > 0.0);
                }
                if (ok) {
                    if (c0 == kDelNone) c0 = c; else c1 = c;
                }
            }
            if (c1 != kDelNone && c1 < c0) {
                const int t = c0;
                c0 = c1;
                c1 = t;
            }
            cand[2 * k] = (unsigned char)c0;
            cand[2 * k + 1] = (unsigned char)c1;
        }
        __syncthreads();
        // ---- 2. candidates in pair order
        int ncand;
        {
            const int chunk = (nslots + kDelThreads - 1) / kDelThreads;
            const int lo = min(tid * chunk, nslots), hi = min(lo + chunk, nslots);
            int cnt = 0;
            for (int s = lo; s < hi; ++s) cnt += cand[s] != kDelNone;
            int off = del_scan(cnt, wsum, tid, &ncand);
            for (int s = lo; s < hi; ++s)
                if (cand[s] != kDelNone) list[off++] = (unsigned short)s;
        }
        __syncthreads();
        // ---- 3. the contract, for every candidate against every live point
        for (int i = tid; i < ncand; i += kDelThreads) {
            const int slot = list[i], c = cand[slot];
            int a, b;
            del_pair(slot >> 1, L, a, b);
            const double ax = sx[a], ay = sy[a], bx = sx[b], by = sy[b], cx = sx[c], cy = sy[c];
            const double o = del_orient(ax, ay, bx, by, cx, cy), ob = del_orient(bx, by, cx, cy, ax, ay);
            bool ok = o > 0.0 || o < 0.0;                    // (i) not collinear
            for (int d = 0; d < L && ok; ++d) {
                if (d == a || d == b || d == c) continue;
                const double dx = sx[d], dy = sy[d];
                const double det = del_incircle(ax, ay, bx, by, cx, cy, dx, dy);
                const double s = o > 0.0 ? det : -det;
                if (s > 0.0) {
                    ok = false;                              // (ii) strictly inside
                } else if (s == 0.0) {
                    if (d < a) {
                        ok = false;                          // (iii) the polygon is fanned from a lower vertex
                    } else {                                 // (iv) v0 = a: d strictly on a's side of b -> c
                        const double od = del_orient(bx, by, cx, cy, dx, dy);
                        ok = (ob > 0.0 && od > 0.0) || (ob < 0.0 && od < 0.0);
                    }
                }
            }
            if (!ok) list[i] = 0xFFFF;
        }
        __syncthreads();
        // ---- 4. survivors in order
        {
            const int chunk = (ncand + kDelThreads - 1) / kDelThreads;
            const int lo = min(tid * chunk, ncand), hi = min(lo + chunk, ncand);
            int cnt = 0;
            for (int i = lo; i < hi; ++i) cnt += list[i] != 0xFFFF;
            int off = del_scan(cnt, wsum, tid, &total);
            if (total <= Tcap) {
                for (int i = lo; i < hi; ++i) {
                    const int slot = list[i];
                    if (slot == 0xFFFF) continue;
                    int a, b;
                    del_pair(slot >> 1, L, a, b);
                    int* row = trin + (long long)off * 3;
                    row[0] = orig[a];
                    row[1] = orig[b];
                    row[2] = orig[cand[slot]];
                    ++off;
                }
            }
        }
    }
    const int written = total <= Tcap ? total : 0;
    for (int i = written * 3 + tid; i < Tcap * 3; i += kDelThreads) trin[i] = -1;
    if (tid == 0) count[n] = total <= Tcap ? total : -1;
}

}  // namespace apamd

using namespace apamd;

extern "C" int ap_delaunay_ok(int32_t N, int32_t P, int32_t Tcap) {
    return N >= 1 && N <= 65535 && P >= 3 && P <= kDelMaxP && Tcap >= 1 && (long long)Tcap * 12 * 4 <= 60 * 1024;
}

extern "C" int ap_delaunay(const float* pts, int32_t N, int32_t P, int32_t Tcap, int32_t* tri, int32_t* count,
                           ap_stream_t stream) {
    if (!pts || !tri || !count) return fail(AP_ERR_INVALID, "delaunay: null pointer");
    if (N < 1 || N > 65535 || P < 3 || Tcap < 1) return fail(AP_ERR_INVALID, "delaunay: bad sizes");
    if (!ap_delaunay_ok(N, P, Tcap))
        return fail(AP_ERR_UNSUPPORTED, "delaunay: %d points (at most %d) or %d triangle rows (at most %d) are not served", P,
                    kDelMaxP, Tcap, 60 * 1024 / 48);
    hipLaunchKernelGGL(delaunay_kernel, dim3(N), dim3(kDelThreads), 0, (hipStream_t)stream, pts, P, Tcap, tri, count);
    return check_launch("delaunay_kernel");
}
