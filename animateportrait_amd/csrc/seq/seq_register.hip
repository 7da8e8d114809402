// seq_register.hip -- rigid registration of landmark frames on the 9-point "T shape" (include/animateportrait_seq.h:
// apq_rigid_register): Module1/util/icp.py and its three uses, the registration of the identity frame (train_content.py:176-183)
// and the two head-stabilisation switches of the clip (train_audio2landmark.py:312-338), so that a device-resident landmark
// sequence stays on the device.  tests/register_reference.py is the float64 statement.
//
// A wave per frame (a workgroup is one wave).  The frame's geometry -- nine points, a 3x3 covariance, its SVD, up to 50 rounds of
// it -- is a chain of a few thousand dependent fp64 operations with nothing to share out; what can be spread is the 68 points it
// is then applied to.  So every lane of the wave computes the same transform from the same nine points (uniform loads, no
// cross-lane traffic, no divergence: the loop counts are the same in all lanes), and then moves its own point, lanes 0 .. 3 a
// second one.  A lane per frame would put 64 frames with different round and sweep counts into one wave, which runs as long as
// its slowest lane times the divergence, on ten of the device's 1024 SIMDs at the example clip's 625 frames; this way 625 SIMDs
// each run one short chain.  The only cross-lane step is the 68-point mean of APQ_REG_CENTER: a butterfly, which hands every
// lane the same bits.  Nothing depends on the wave's index but its row addresses.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "seq_register_checks.h"

namespace {

constexpr int LMC = APQ_LM_C;
constexpr int NP = apq::kTShapeN;
constexpr int kMaxSweeps = 30;                  // of the Jacobi iteration; a well-posed 3x3 needs 4 .. 6

int launched(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(apq::err_buf(), 256, "%s: launch failed: %s", what, hipGetErrorString(e));
        return APQ_ERR_LAUNCH;
    }
    return APQ_OK;
}

struct Rigid {
    double r[3][3], t[3];
};

// One rotation of the one-sided Jacobi iteration: columns p and q of G (and of V) are turned until they are orthogonal.
__device__ __forceinline__ bool jacobi_pair(double (&g)[3][3], double (&v)[3][3], int p, int q) {
    const double alpha = g[0][p] * g[0][p] + g[1][p] * g[1][p] + g[2][p] * g[2][p];
    const double beta = g[0][q] * g[0][q] + g[1][q] * g[1][q] + g[2][q] * g[2][q];
    const double gamma = g[0][p] * g[0][q] + g[1][p] * g[1][q] + g[2][p] * g[2][q];
    if (!(fabs(gamma) > 2.220446049250313e-16 * sqrt(alpha * beta))) return false;      // (false for NaN too)
    const double zeta = (beta - alpha) / (2.0 * gamma);
    const double tn = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    const double c = 1.0 / sqrt(1.0 + tn * tn), s = c * tn;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double gp = g[i][p], gq = g[i][q], vp = v[i][p], vq = v[i][q];
        g[i][p] = c * gp - s * gq;
        g[i][q] = s * gp + c * gq;
        v[i][p] = c * vp - s * vq;
        v[i][q] = s * vp + c * vq;
    }
    return true;
}

// The rotation of best_fit_transform from H = AA^T BB = U S V^T: R = V U^T, with the direction of the smallest singular value
// mirrored when det(V U^T) < 0.  Both cases are R = v1 u1^T + v2 u2^T + (v1 x v2) (u1 x u2)^T over the two largest singular
// values: the third pair is fixed by them up to the one sign that det R = +1 decides.  One-sided Jacobi: G = H V with
// orthogonal columns, whose lengths are the singular values and whose directions are U.
__device__ __forceinline__ void kabsch_rotation(const double (&h)[3][3], double (&r)[3][3]) {
    double g[3][3], v[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            g[i][j] = h[i][j];
            v[i][j] = i == j ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < kMaxSweeps; ++sweep) {
        bool turned = jacobi_pair(g, v, 0, 1);
        turned |= jacobi_pair(g, v, 0, 2);
        turned |= jacobi_pair(g, v, 1, 2);
        if (!turned) break;
    }
    double s2[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) s2[j] = g[0][j] * g[0][j] + g[1][j] * g[1][j] + g[2][j] * g[2][j];
    // the columns of the two largest singular values, in LAPACK's descending order (the first of equals first)
    auto order = [&](int p, int q) {                 // (selects, so that no index is a run-time value)
        const bool swap = s2[q] > s2[p];
        const double sp = s2[p], sq = s2[q];
        s2[p] = swap ? sq : sp;
        s2[q] = swap ? sp : sq;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double gp = g[i][p], gq = g[i][q], vp = v[i][p], vq = v[i][q];
            g[i][p] = swap ? gq : gp;
            g[i][q] = swap ? gp : gq;
            v[i][p] = swap ? vq : vp;
            v[i][q] = swap ? vp : vq;
        }
    };
    order(0, 1);
    order(0, 2);
    order(1, 2);
    double u1[3], u2[3], v1[3], v2[3];
    const double ia = 1.0 / sqrt(s2[0]), ib = 1.0 / sqrt(s2[1]);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        u1[i] = g[i][0] * ia;
        u2[i] = g[i][1] * ib;
        v1[i] = v[i][0];
        v2[i] = v[i][1];
    }
    const double u3[3] = {u1[1] * u2[2] - u1[2] * u2[1], u1[2] * u2[0] - u1[0] * u2[2], u1[0] * u2[1] - u1[1] * u2[0]};
    const double v3[3] = {v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) r[i][j] = v1[i] * u1[j] + v2[i] * u2[j] + v3[i] * u3[j];
}

// best_fit_transform(a, b): the rigid map of the points a onto the points b
__device__ __forceinline__ void best_fit(const double (&a)[NP][3], const double (&b)[NP][3], Rigid& f) {
    double ca[3], cb[3], h[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double sa = 0.0, sb = 0.0;
#pragma unroll
        for (int n = 0; n < NP; ++n) {
            sa += a[n][k];
            sb += b[n][k];
        }
        ca[k] = sa / NP;
        cb[k] = sb / NP;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double s = 0.0;
#pragma unroll
            for (int n = 0; n < NP; ++n) s += (a[n][i] - ca[i]) * (b[n][j] - cb[j]);
            h[i][j] = s;
        }
    kabsch_rotation(h, f.r);
#pragma unroll
    for (int i = 0; i < 3; ++i) f.t[i] = cb[i] - (f.r[i][0] * ca[0] + f.r[i][1] * ca[1] + f.r[i][2] * ca[2]);
}

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);      // a + b == b + a: every lane ends with the same bits
    return x;
}

// grid: T workgroups of one wave
__global__ __launch_bounds__(apq::kRegThreads) void register_kernel(const float* in, const float* __restrict__ std_face, float* out,
                                                                    double* __restrict__ pose, int flags) {
    const int lane = threadIdx.x;
    const float* const row = in + (long long)blockIdx.x * LMC;
    float* const orow = out + (long long)blockIdx.x * LMC;
    const bool second = lane + 64 < 68;
    // this lane's points and the frame's T shape (every lane reads the same nine points), all before the row's first store
    double p0[3], p1[3], a[NP][3], d[NP][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        p0[k] = (double)row[lane * 3 + k];
        p1[k] = second ? (double)row[(lane + 64) * 3 + k] : 0.0;
    }
#pragma unroll
    for (int n = 0; n < NP; ++n)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            a[n][k] = (double)row[apq::kTShape[n] * 3 + k];
            d[n][k] = (double)std_face[apq::kTShape[n] * 3 + k];
        }
    if (flags & APQ_REG_CENTER) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double ms = wave_sum((double)std_face[lane * 3 + k] + (second ? (double)std_face[(lane + 64) * 3 + k] : 0.0)) / 68.0;
            const double mp = wave_sum(p0[k] + p1[k]) / 68.0;
            p0[k] = p0[k] - mp + ms;
            p1[k] = p1[k] - mp + ms;
#pragma unroll
            for (int n = 0; n < NP; ++n) a[n][k] = a[n][k] - mp + ms;
        }
    }
    if (pose || (flags & (APQ_REG_NO_X_ROT | APQ_REG_REGISTER))) {           // (the same in every lane)
        // icp(a, d) with its correspondences fixed by index
        Rigid f;
        double src[NP][3];
#pragma unroll
        for (int n = 0; n < NP; ++n)
#pragma unroll
            for (int k = 0; k < 3; ++k) src[n][k] = a[n][k];
        double prev = 0.0;
        for (int round = 0; round < APQ_REG_MAX_ROUNDS; ++round) {
            double err = 0.0;
#pragma unroll
            for (int n = 0; n < NP; ++n)
#pragma unroll
                for (int k = 0; k < 3; ++k) err += (src[n][k] - d[n][k]) * (src[n][k] - d[n][k]);
            best_fit(src, d, f);
#pragma unroll
            for (int n = 0; n < NP; ++n) {
                const double x = src[n][0], y = src[n][1], z = src[n][2];
#pragma unroll
                for (int k = 0; k < 3; ++k) src[n][k] = f.r[k][0] * x + f.r[k][1] * y + f.r[k][2] * z + f.t[k];
            }
            if (fabs(prev - err) < 1e-4) break;
            prev = err;
        }
        best_fit(a, src, f);
        if (pose && lane < 12) {
            double val = 0.0;
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (lane == i * 4 + j) val = j < 3 ? f.r[i][j] : f.t[i];
            pose[(long long)blockIdx.x * 12 + lane] = val;
        }
        if (flags & APQ_REG_REGISTER) {
            const double x0 = p0[0], y0 = p0[1], z0 = p0[2], x1 = p1[0], y1 = p1[1], z1 = p1[2];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                p0[k] = f.r[k][0] * x0 + f.r[k][1] * y0 + f.r[k][2] * z0 + f.t[k];
                p1[k] = f.r[k][0] * x1 + f.r[k][1] * y1 + f.r[k][2] * z1 + f.t[k];
            }
        } else if (flags & APQ_REG_NO_X_ROT) {
            // R = Rz(c) Ry(b) Rx(a): cos b = |(R00, R10)| / |column 0|, sin b = -R20 / |column 0|, (cos c, sin c) = (R00, R10)
            // normalised: what atan2 makes of them, without the angles.  At gimbal lock hb = 0 and the quotients are not numbers.
            const double hb = sqrt(f.r[0][0] * f.r[0][0] + f.r[1][0] * f.r[1][0]);
            const double nb = sqrt(hb * hb + f.r[2][0] * f.r[2][0]);
            const double cb = hb / nb, sb = -f.r[2][0] / nb, cc = f.r[0][0] / hb, sc = f.r[1][0] / hb;
            const double q[3][3] = {{cc * cb, -sc, cc * sb}, {sc * cb, cc, sc * sb}, {-sb, 0.0, cb}};
            const double x0 = p0[0] - f.t[0], y0 = p0[1] - f.t[1], z0 = p0[2] - f.t[2];
            const double x1 = p1[0] - f.t[0], y1 = p1[1] - f.t[1], z1 = p1[2] - f.t[2];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                p0[k] = q[k][0] * x0 + q[k][1] * y0 + q[k][2] * z0 + f.t[k];
                p1[k] = q[k][0] * x1 + q[k][1] * y1 + q[k][2] * z1 + f.t[k];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        orow[lane * 3 + k] = (float)p0[k];
        if (second) orow[(lane + 64) * 3 + k] = (float)p1[k];
    }
}

}  // namespace

extern "C" {

int32_t apq_rigid_register_ok(const float* in, const float* std, const float* out, const double* pose, int32_t T, int32_t flags) {
    return apq::check_rigid_register(in, std, out, pose, T, flags) == APQ_OK ? 1 : 0;
}

int apq_rigid_register(const float* in, const float* std, float* out, double* pose, int32_t T, int32_t flags, void* stream) {
    const int rc = apq::check_rigid_register(in, std, out, pose, T, flags);
    if (rc != APQ_OK) return rc;
    (void)hipGetLastError();
    hipLaunchKernelGGL(register_kernel, dim3(T), dim3(apq::kRegThreads), 0, (hipStream_t)stream, in, std, out, pose, flags);
    return launched("rigid_register");
}

}  // extern "C"
