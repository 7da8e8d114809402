// seq_f0.hip -- the clip's f0 track for the AutoVC converter (include/animateportrait_seq.h: apq_f0_candidates, apq_f0_track).
// The reference gets it from pysptk's rapt on the host (extract_f0_func.py:120-125); here it is RAPT as published (Talkin 1995,
// the get_f0 defaults) with one NCCF pass at the full rate, stated in float64 by tests/f0_reference.py, which is the contract:
// every decision the paper leaves open is taken there, and this file follows it statement by statement.
//
// A clip is about a thousand frames, a frame 322 lags of 120 products at most plus two 480-sample LPC frames: the work is tiny,
// so both kernels are laid out for few dependent steps, not for throughput.
//   f0_candidates_kernel  one workgroup per frame, a lane per lag.  The span and both LPC frames are staged in LDS; the NCCF
//                         sums, the autocorrelations (a wave per lag, shuffle-reduced) and Levinson (one lane) run in fp64, so
//                         that a frame's candidate set is the restatement's unless a peak sits on a threshold to 1e-12.  The
//                         19 kept candidates and their order by lag come from rank counting, as in calib_kernel.  The frame
//                         before's LPC is recomputed here: no workgroup waits for another.
//   f0_track_kernel       one wave.  D and the log lags of the frame before sit ping-pong in LDS in fp32 (the minimum is
//                         subtracted after every frame, so the range stays that of one frame); a lane per target state loops
//                         over the predecessors.  The next frame's table row is loaded before the current one is used.  One
//                         lane walks the back-pointers, then all lanes normalise: mean and deviation in fp64, two passes.
// Neither kernel uses atomics, a workspace or a host synchronisation.
//
// The expressions keep the restatement's operation order; nothing may be fused behind its back.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "seq_f0_checks.h"

namespace {

constexpr int HOP = APQ_F0_HOP;
constexpr int NC = apq::kF0Corr;
constexpr int NL = apq::kF0Lpc;
constexpr int ORD = apq::kF0Order;
constexpr int CANDS = APQ_F0_CANDS;
constexpr int STATES = APQ_F0_STATES;
constexpr int NT = apq::kF0Threads;
constexpr int WAVES = NT / 64;

int launched(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(apq::err_buf(), 256, "%s: launch failed: %s", what, hipGetErrorString(e));
        return APQ_ERR_LAUNCH;
    }
    return APQ_OK;
}

__device__ __forceinline__ double wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__device__ __forceinline__ double wave_max(double v) {
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    return v;
}

// ---------------------------------------------------------------------------------------------------------------- candidates
struct CandParams {
    const float* x;
    int32_t* count;
    float *lag, *val, *rr, *s;
    int L, kmin, kmax;
};

// Levinson's recursion on r[0 .. 18] (autocorrelation method): a[0 .. 18] with a[0] = 1; returns the residual energy.
// One lane; the arrays live in LDS, so that their run-time indices cost no scratch memory.
__device__ double levinson(const double* r, double* a, double* prev) {
    for (int i = 1; i <= ORD; ++i) a[i] = 0.0;
    a[0] = 1.0;
    double err = r[0];
    for (int m = 1; m <= ORD; ++m) {
        double acc = 0.0;
        for (int i = 1; i < m; ++i) acc += a[i] * r[m - i];
        const double k = -(r[m] + acc) / err;
        for (int i = 1; i < m; ++i) prev[i] = a[i];
        a[m] = k;
        for (int i = 1; i < m; ++i) a[i] = prev[i] + k * prev[m - i];
        err = err * (1.0 - k * k);
    }
    return err;
}

// grid: T workgroups (frame t = blockIdx.x) of 384 threads
__global__ __launch_bounds__(NT) void f0_candidates_kernel(const CandParams p) {
    __shared__ double sp[apq::kF0Span];          // the frame's span, the reference window's mean removed
    __shared__ double fr[2][NL];                 // the Hann-weighted LPC frames of t - 1 and t
    __shared__ double phi[apq::kF0Lags];         // phi(kmin - 1 + i)
    __shared__ double cval[apq::kF0Lags];        // a candidate's refined value, -1 where there is none
    __shared__ int kept[apq::kF0Lags];
    __shared__ double r[2][ORD + 1];
    __shared__ double red[WAVES];
    __shared__ double lpa[2][ORD + 1], lprev[ORD + 1];

    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int span = NC + p.kmax + 2;            // <= kF0Span: kmax <= APQ_F0_MAX_LAG
    const int nl = p.kmax - p.kmin + 3;          // <= kF0Lags: kmin >= APQ_F0_MIN_LAG

    for (int i = tid; i < span; i += NT) {
        const long long g = (long long)HOP * t - NC / 2 + i;
        sp[i] = (g >= 0 && g < p.L) ? (double)p.x[g] : 0.0;
    }
    for (int e = tid; e < 2 * NL; e += NT) {
        const int w = e / NL, i = e - w * NL;
        const long long g = (long long)HOP * (t - 1 + w) - NL / 2 + i;
        const double v = (g >= 0 && g < p.L) ? (double)p.x[g] : 0.0;
        fr[w][i] = v * (0.5 - 0.5 * cospi(((double)i + 0.5) / (double)(NL / 2)));
    }
    __syncthreads();

    // the autocorrelations r[w][0 .. 18]: a wave per (frame, lag) pair in turn
    for (int pair = wave; pair < 2 * (ORD + 1); pair += WAVES) {
        const int w = pair / (ORD + 1), m = pair - w * (ORD + 1);
        double acc = 0.0;
        for (int j = lane; j < NL - m; j += 64) acc += fr[w][j] * fr[w][j + m];
        acc = wave_sum(acc);
        if (lane == 0) r[w][m] = acc;
    }
    if (wave == 0) {
        double acc = lane < NC ? sp[lane] : 0.0;
        if (lane + 64 < NC) acc += sp[lane + 64];
        acc = wave_sum(acc);
        if (lane == 0) red[0] = acc;
    }
    __syncthreads();
    const double mean = red[0] / (double)NC;
    __syncthreads();                             // (red is written again below)
    for (int i = tid; i < span; i += NT) sp[i] -= mean;
    __syncthreads();

    // NCCF: lane i owns the lag kmin - 1 + i; the largest sample read is sp[NC - 1 + kmax + 1]
    if (tid < nl) {
        const int k = p.kmin - 1 + tid;
        double acc = 0.0, ek = 0.0, e0 = 0.0;
        for (int j = 0; j < NC; ++j) {
            const double a = sp[j], b = sp[j + k];
            acc += a * b;
            ek += b * b;
            e0 += a * a;
        }
        const double floor_a = (100.0 * NC) * (100.0 * NC);
        phi[tid] = acc / sqrt(e0 * ek + floor_a);
    }
    __syncthreads();
    const bool inner = tid >= 1 && tid <= nl - 2;          // the lags kmin .. kmax
    {
        const double m = wave_max(inner ? phi[tid] : -INFINITY);
        if (lane == 0) red[wave] = m;
    }
    __syncthreads();
    double top = red[0];
    for (int w = 1; w < WAVES; ++w) top = fmax(top, red[w]);

    bool cand = false;
    double my_lag = 0.0, my_val = -1.0;
    if (inner) {
        const double a = phi[tid - 1], b = phi[tid], c = phi[tid + 1];
        cand = b > a && b >= c && b > 0.0 && b >= 0.3 * top;
        if (cand) {
            const double d = 0.5 * (a - c) / (a - 2.0 * b + c);        // (a < b and c <= b: the denominator is negative)
            my_lag = (double)(p.kmin - 1 + tid) + d;
            my_val = b - 0.25 * (a - c) * d;                           // >= b > 0
        }
    }
    if (tid < nl) cval[tid] = my_val;
    __syncthreads();
    // rank by (value descending, lag ascending): a permutation whatever the ties; the 19 first are kept
    bool keep = false;
    if (cand) {
        int rank = 0;
        for (int i = 0; i < nl; ++i) {
            const double v = cval[i];
            rank += (v > my_val || (v == my_val && i < tid)) ? 1 : 0;
        }
        keep = rank < CANDS;
    }
    if (tid < nl) kept[tid] = keep ? 1 : 0;
    __syncthreads();
    if (keep || tid < CANDS) {
        int pos = 0, total = 0;
        for (int i = 0; i < nl; ++i) {
            pos += (i < tid) ? kept[i] : 0;
            total += kept[i];
        }
        if (keep) {                                                    // pos < total <= 19
            p.lag[(long long)t * CANDS + pos] = (float)my_lag;
            p.val[(long long)t * CANDS + pos] = (float)my_val;
        }
        if (tid < CANDS && tid >= total) {
            p.lag[(long long)t * CANDS + tid] = 0.f;
            p.val[(long long)t * CANDS + tid] = 0.f;
        }
        if (tid == 0) p.count[t] = total;
    }

    // the transition terms: one lane
    if (tid == 0) {
        double rr = 1.0, s = 1.0;
        if (t > 0) {
            const double rms1 = sqrt(r[1][0] / (double)NL), rms0 = sqrt(r[0][0] / (double)NL);
            r[1][0] = r[1][0] * (1.0 + 1e-7) + 1.0;
            r[0][0] = r[0][0] * (1.0 + 1e-7) + 1.0;
            const double err1 = levinson(r[1], lpa[1], lprev);
            (void)levinson(r[0], lpa[0], lprev);
            rr = (rms1 + 1.0) / (rms0 + 1.0);
            const double* a = lpa[0];
            double num = 0.0;
            for (int m = ORD; m >= 0; --m) {
                double b = 0.0;
                for (int i = 0; i + m <= ORD; ++i) b += a[i] * a[i + m];
                num += (m == 0 ? 1.0 : 2.0) * r[1][m] * b;
            }
            const double it = fmax(num / err1, 1.0);
            s = 0.2 / (it - 0.8);
        }
        p.rr[t] = (float)rr;
        p.s[t] = (float)s;
    }
}

// --------------------------------------------------------------------------------------------------------------------- track
struct TrackParams {
    const int32_t* count;
    const float *lag, *val, *rr, *s;
    uint8_t *back, *path;
    float* f0;
    int T;
    float kmax;
    double fs;
};

__device__ __forceinline__ int clamp_count(int n) { return n < 0 ? 0 : (n > CANDS ? CANDS : n); }

// grid: one workgroup of one wave
__global__ __launch_bounds__(64) void f0_track_kernel(const TrackParams p) {
    __shared__ float Dl[2][STATES], Ll[2][STATES];
    const int lane = threadIdx.x, T = p.T;
    const float LN2 = 0.69314718055994530942f;

    int cn = clamp_count(p.count[0]);
    float lg = lane < CANDS ? p.lag[lane] : 0.f, vl = lane < CANDS ? p.val[lane] : 0.f;
    float rrn = p.rr[0], sn = p.s[0];
    int nprev = 0;
    for (int t = 0; t < T; ++t) {
        const int n = cn, cur = t & 1, prv = cur ^ 1;
        const float l = lg, c = vl, rr = rrn, s = sn;
        if (t + 1 < T) {                                       // the next row is on its way while this one is used
            cn = clamp_count(p.count[t + 1]);
            if (lane < CANDS) {
                lg = p.lag[(long long)(t + 1) * CANDS + lane];
                vl = p.val[(long long)(t + 1) * CANDS + lane];
            }
            rrn = p.rr[t + 1];
            sn = p.s[t + 1];
        }
        float cm = lane < n ? c : -INFINITY;
        for (int off = 32; off > 0; off >>= 1) cm = fmaxf(cm, __shfl_xor(cm, off));
        if (n == 0) cm = 0.f;
        const bool voiced = lane < n, active = lane <= n;
        float d = 0.f, ll = 0.f;
        if (voiced) {
            d = 1.f - c * (1.f - 0.3f * l / p.kmax);
            ll = logf(l);
        } else if (lane == n) {
            d = 0.f + cm;                                      // voice_bias = 0
        }
        float tot = d;
        int bi = 0;
        if (t > 0 && active) {
            const int m = nprev;
            float best = INFINITY;
            if (voiced) {
                for (int i = 0; i < m; ++i) {
                    const float xi = ll - Ll[prv][i];
                    const float delta = 0.02f * fminf(fabsf(xi), 0.35f + fminf(fabsf(xi - LN2), fabsf(xi + LN2)));
                    const float v = Dl[prv][i] + delta;
                    if (v < best) { best = v; bi = i; }
                }
                const float v = Dl[prv][m] + (0.005f + 0.5f * s + 0.5f / rr);
                if (v < best) { best = v; bi = m; }
            } else {
                const float up = 0.005f + 0.5f * s + 0.5f * rr;
                for (int i = 0; i < m; ++i) {
                    const float v = Dl[prv][i] + up;
                    if (v < best) { best = v; bi = i; }
                }
                const float v = Dl[prv][m] + 0.f;
                if (v < best) { best = v; bi = m; }
            }
            tot = d + best;
        }
        float mn = active ? tot : INFINITY;
        for (int off = 32; off > 0; off >>= 1) mn = fminf(mn, __shfl_xor(mn, off));
        if (active) {
            Dl[cur][lane] = tot - mn;
            Ll[cur][lane] = ll;
        }
        if (lane < STATES) p.back[(long long)t * STATES + lane] = (uint8_t)(active ? bi : 0);
        nprev = n;
        __syncthreads();
    }
    __threadfence_block();
    __syncthreads();
    if (lane == 0) {
        const int fin = (T - 1) & 1;
        int j = 0;
        for (int i = 1; i <= nprev; ++i)
            if (Dl[fin][i] < Dl[fin][j]) j = i;
        for (int t = T - 1; t >= 0; --t) {                      // j <= count[t] <= 19: back was written for every such state
            const int n = clamp_count(p.count[t]);
            p.path[t] = (uint8_t)(j < n ? j : APQ_F0_UNVOICED);
            if (t > 0) j = p.back[(long long)t * STATES + j];
        }
    }
    __threadfence_block();
    __syncthreads();

    // speaker_normalization: mean and population deviation of the voiced log-f0 in fp64, two passes as numpy takes them
    auto logf0 = [&](int t, bool& v) {
        const int j = p.path[t];
        v = j != APQ_F0_UNVOICED;
        return v ? log(p.fs / (double)p.lag[(long long)t * CANDS + j]) : 0.0;
    };
    double sum = 0.0, cnt = 0.0;
    for (int t = lane; t < T; t += 64) {
        bool v;
        const double lf = logf0(t, v);
        if (v) { sum += lf; cnt += 1.0; }
    }
    sum = wave_sum(sum);
    cnt = wave_sum(cnt);
    const double mean = cnt > 0.0 ? sum / cnt : 0.0;
    double ss = 0.0;
    for (int t = lane; t < T; t += 64) {
        bool v;
        const double lf = logf0(t, v);
        if (v) ss += (lf - mean) * (lf - mean);
    }
    ss = wave_sum(ss);
    const double sd = cnt > 0.0 ? sqrt(ss / cnt) : 0.0;
    for (int t = lane; t < T; t += 64) {
        bool v;
        const double lf = logf0(t, v);
        float out = -1e10f;
        if (v) {
            if (sd == 0.0) {
                out = 0.5f;
            } else {
                double q = (lf - mean) / sd / 4.0;
                q = fmin(fmax(q, -1.0), 1.0);
                out = (float)((q + 1.0) / 2.0);
            }
        }
        p.f0[t] = out;
    }
}

}  // namespace

extern "C" {

int32_t apq_f0_candidates_ok(const float* x, int32_t L, int32_t T, int32_t kmin, int32_t kmax, const int32_t* count, const float* lag,
                             const float* val, const float* rr, const float* s) {
    return apq::check_f0_candidates(x, L, T, kmin, kmax, count, lag, val, rr, s) == APQ_OK ? 1 : 0;
}

int apq_f0_candidates(const float* x, int32_t L, int32_t T, int32_t kmin, int32_t kmax, int32_t* count, float* lag, float* val,
                      float* rr, float* s, void* stream) {
    const int rc = apq::check_f0_candidates(x, L, T, kmin, kmax, count, lag, val, rr, s);
    if (rc != APQ_OK) return rc;
    CandParams p;
    p.x = x; p.count = count; p.lag = lag; p.val = val; p.rr = rr; p.s = s; p.L = L; p.kmin = kmin; p.kmax = kmax;
    (void)hipGetLastError();
    hipLaunchKernelGGL(f0_candidates_kernel, dim3(T), dim3(NT), 0, (hipStream_t)stream, p);
    return launched("f0_candidates");
}

int32_t apq_f0_track_ok(const int32_t* count, const float* lag, const float* val, const float* rr, const float* s, int32_t T,
                        int32_t kmax, double fs, const uint8_t* back, const uint8_t* path, const float* f0) {
    return apq::check_f0_track(count, lag, val, rr, s, T, kmax, fs, back, path, f0) == APQ_OK ? 1 : 0;
}

int apq_f0_track(const int32_t* count, const float* lag, const float* val, const float* rr, const float* s, int32_t T, int32_t kmax,
                 double fs, uint8_t* back, uint8_t* path, float* f0, void* stream) {
    const int rc = apq::check_f0_track(count, lag, val, rr, s, T, kmax, fs, back, path, f0);
    if (rc != APQ_OK) return rc;
    TrackParams p;
    p.count = count; p.lag = lag; p.val = val; p.rr = rr; p.s = s; p.back = back; p.path = path; p.f0 = f0; p.T = T;
    p.kmax = (float)kmax; p.fs = fs;
    (void)hipGetLastError();
    hipLaunchKernelGGL(f0_track_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, p);
    return launched("f0_track");
}

}  // extern "C"
