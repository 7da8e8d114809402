// Host side of libapstyle.so that needs no device: the argument checks and the launch planners of its three calls.  Plain C++,
// so that tools/style_host_check.cpp can compile it with the host sanitisers.
#pragma once

#include <stdint.h>
#include <stdio.h>

#include "../../../include/animateportrait_style.h"

namespace aps {

inline char* err_buf() {
    static thread_local char buf[256] = "";
    return buf;
}

// writes the message, returns `code`
inline int fail(int code, const char* fmt, long a = 0, long b = 0, long c = 0, long d = 0) {
    snprintf(err_buf(), 256, fmt, a, b, c, d);
    return code;
}

// What a launch over planes needs: the grid (one workgroup per output plane), the workgroup size and the output plane's shape
struct PlanePlan {
    int planes, threads, OH, OW;
};

// 1024 lanes where a plane keeps them busy for several rounds, 256 otherwise (a 4 x 4 plane of the hourglass's centre uses 16)
inline int plane_threads(long hw) { return hw >= 16384 ? 1024 : 256; }

inline int check_shape(const char* what, int N, int C, int H, int W) {
    if (N < 1 || C < 1 || H < 1 || W < 1) return snprintf(err_buf(), 256, "%s: empty tensor %d x %d x %d x %d", what, N, C, H, W), APS_ERR_INVALID;
    if (H > APS_MAX_SIDE || W > APS_MAX_SIDE) return snprintf(err_buf(), 256, "%s: plane %d x %d, served: up to %d", what, H, W, APS_MAX_SIDE), APS_ERR_UNSUPPORTED;
    if ((long long)N * C > APS_MAX_PLANES) return snprintf(err_buf(), 256, "%s: %lld planes, served: up to %d", what, (long long)N * C, APS_MAX_PLANES), APS_ERR_UNSUPPORTED;
    if ((long long)N * C * H * W > APS_MAX_ELEMS) return snprintf(err_buf(), 256, "%s: %lld elements, served: below 2^31", what, (long long)N * C * H * W), APS_ERR_UNSUPPORTED;
    return APS_OK;
}

inline int check_stats_pair(const char* what, const void* mean_out, const void* rstd_out) {
    if ((mean_out == nullptr) != (rstd_out == nullptr))
        return snprintf(err_buf(), 256, "%s: mean_out and rstd_out come together or not at all", what), APS_ERR_INVALID;
    return APS_OK;
}

inline int plan_lin_coeffs(const void* x, const void* rho, const void* gamma, const void* beta, const void* planes, const void* a,
                           const void* b, int N, int C, int H, int W, int per_sample, PlanePlan* pl) {
    if (!x || !rho || !gamma || !beta || !planes || !a || !b) return fail(APS_ERR_INVALID, "lin_coeffs: null pointer");
    if (per_sample != 0 && per_sample != 1) return fail(APS_ERR_INVALID, "lin_coeffs: per_sample = %ld (0: [C], 1: [N * C])", per_sample);
    const int rc = check_shape("lin_coeffs", N, C, H, W);
    if (rc != APS_OK) return rc;
    if ((long)H * W < 2) return fail(APS_ERR_UNSUPPORTED, "lin_coeffs: a plane of %ld x %ld has no unbiased variance", H, W);
    *pl = PlanePlan{N * C, plane_threads((long)H * W), H, W};
    return APS_OK;
}

inline int plan_affine_apply(const void* x, const void* a, const void* b, const void* y, const void* mean_out, const void* rstd_out,
                             int N, int C, int H, int W, int act, PlanePlan* pl) {
    if (!x || !a || !b || !y) return fail(APS_ERR_INVALID, "affine_apply: null pointer");
    if (act != APS_ACT_NONE && act != APS_ACT_RELU) return fail(APS_ERR_UNSUPPORTED, "affine_apply: activation %ld (served: none, ReLU)", act);
    int rc = check_stats_pair("affine_apply", mean_out, rstd_out);
    if (rc != APS_OK) return rc;
    rc = check_shape("affine_apply", N, C, H, W);
    if (rc != APS_OK) return rc;
    *pl = PlanePlan{N * C, plane_threads((long)H * W), H, W};
    return APS_OK;
}

inline int plan_plane_combine(int mode, const void* s0, const void* s1, const void* s2, const void* s3, int N, int C, int H, int W,
                              int Hs, int Ws, int flags, const void* y, const void* mean_out, const void* rstd_out, PlanePlan* pl) {
    if (mode < APS_JOIN || mode > APS_STAT) return fail(APS_ERR_INVALID, "plane_combine: mode %ld", mode);
    if (!s0) return fail(APS_ERR_INVALID, "plane_combine: null s0");
    int rc = check_shape("plane_combine", N, C, H, W);
    if (rc != APS_OK) return rc;
    if (mode == APS_STAT) {
        if (y || rstd_out || !mean_out) return fail(APS_ERR_INVALID, "plane_combine STAT: writes mean_out only (y and rstd_out null)");
        if (flags & ~APS_STAT_RELU) return fail(APS_ERR_INVALID, "plane_combine STAT: flags %ld", flags);
        *pl = PlanePlan{N * C, plane_threads((long)H * W), H, W};
        return APS_OK;
    }
    if (flags != 0) return fail(APS_ERR_INVALID, "plane_combine: flags %ld outside STAT", flags);
    if (!y) return fail(APS_ERR_INVALID, "plane_combine: null y");
    rc = check_stats_pair("plane_combine", mean_out, rstd_out);
    if (rc != APS_OK) return rc;
    int OH = H, OW = W;
    switch (mode) {
    case APS_JOIN:
        if (!s1 || !s2 || !s3) return fail(APS_ERR_INVALID, "plane_combine JOIN: null part");
        if (C % 4 != 0) return fail(APS_ERR_UNSUPPORTED, "plane_combine JOIN: C = %ld is no multiple of 4 (parts C/2, C/4, C/4)", C);
        break;
    case APS_POOL2:
        if (H < 2 || W < 2) return fail(APS_ERR_UNSUPPORTED, "plane_combine POOL2: a %ld x %ld plane has no 2 x 2 window", H, W);
        OH = H / 2; OW = W / 2;
        break;
    case APS_UP2ADD:
        if (s1 && (Hs != 2 * H || Ws != 2 * W))
            return fail(APS_ERR_INVALID, "plane_combine UP2ADD: skip of %ld x %ld for an input of %ld x %ld", Hs, Ws, H, W);
        OH = 2 * H; OW = 2 * W;
        rc = check_shape("plane_combine UP2ADD output", N, C, OH, OW);
        if (rc != APS_OK) return rc;
        break;
    case APS_SUM3:
        if (!s1 || !s2) return fail(APS_ERR_INVALID, "plane_combine SUM3: null term");
        break;
    }
    *pl = PlanePlan{N * C, plane_threads((long)OH * OW), OH, OW};
    return APS_OK;
}

// Luminance (forward: in = frame of 3 planes, out = 1 plane; backward: the other way round).  A launch is (blocks, N) workgroups
// of 256 lanes that walk `items` items per sample: float4 items when every plane of both tensors starts on a 16-byte boundary
// (H W % 4 == 0 and aligned bases), else single floats -- with H W % 4 != 0 the plane starts are misaligned against each other,
// so there is no common vector body to peel a tail from.
struct LumaPlan {
    int vec, blocks;
    long items;
};

inline int plan_luma(const char* what, const void* in, const void* out, int N, int H, int W, LumaPlan* pl) {
    if (!in || !out) return snprintf(err_buf(), 256, "%s: null pointer", what), APS_ERR_INVALID;
    const int rc = check_shape(what, N, 3, H, W);
    if (rc != APS_OK) return rc;
    const long hw = (long)H * W;
    pl->vec = (hw % 4 == 0 && (((uintptr_t)in | (uintptr_t)out) & 15) == 0) ? 4 : 1;
    pl->items = hw / pl->vec;
    pl->blocks = (int)((pl->items + 255) / 256 < 1024 ? (pl->items + 255) / 256 : 1024);
    return APS_OK;
}

}  // namespace aps
