// Host side of apq_rigid_register that needs no device: its argument checks.  Plain C++ like seq_checks.h, so that a stand-alone
// program can compile it with the host sanitisers (tools/register_host_check.py).
#pragma once

#include "seq_checks.h"

namespace apq {

constexpr int kRegThreads = 64;                 // a workgroup is one wave is one frame
constexpr int kTShapeN = 9;
constexpr int kTShape[kTShapeN] = {27, 28, 29, 30, 33, 36, 39, 42, 45};

// [a, a + na) and [b, b + nb) share a byte (addresses compared as integers: the pointers are never dereferenced)
inline bool ranges_overlap(const void* a, long long na, const void* b, long long nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)nb && b0 < a0 + (uintptr_t)na;
}

inline int check_rigid_register(const void* in, const void* std_face, const void* out, const void* pose, int T, int flags) {
    if (!in) return fail(APQ_ERR_INVALID, "rigid_register: null in");
    if (!std_face) return fail(APQ_ERR_INVALID, "rigid_register: null std");
    if (!out) return fail(APQ_ERR_INVALID, "rigid_register: null out");
    if (flags & ~(APQ_REG_CENTER | APQ_REG_NO_X_ROT | APQ_REG_REGISTER)) return fail(APQ_ERR_INVALID, "rigid_register: unknown flags = %lld", flags);
    if ((flags & APQ_REG_REGISTER) && (flags & (APQ_REG_CENTER | APQ_REG_NO_X_ROT)))
        return fail(APQ_ERR_INVALID, "rigid_register: flags = %lld: APQ_REG_REGISTER excludes APQ_REG_CENTER and APQ_REG_NO_X_ROT", flags);
    if (T < 1) return fail(APQ_ERR_INVALID, "rigid_register: T = %lld (at least 1)", T);
    if (T > APQ_MAX_T) return fail(APQ_ERR_UNSUPPORTED, "rigid_register: T = %lld, served: up to %lld (a workgroup per frame)", T, APQ_MAX_T);
    if (misaligned(in, APQ_ALIGN_ELEM)) return fail(APQ_ERR_UNSUPPORTED, "rigid_register: in is not %lld-byte aligned", APQ_ALIGN_ELEM);
    if (misaligned(std_face, APQ_ALIGN_ELEM)) return fail(APQ_ERR_UNSUPPORTED, "rigid_register: std is not %lld-byte aligned", APQ_ALIGN_ELEM);
    if (misaligned(out, APQ_ALIGN_ELEM)) return fail(APQ_ERR_UNSUPPORTED, "rigid_register: out is not %lld-byte aligned", APQ_ALIGN_ELEM);
    if (pose && misaligned(pose, APQ_ALIGN_F64)) return fail(APQ_ERR_UNSUPPORTED, "rigid_register: pose is not %lld-byte aligned", APQ_ALIGN_F64);
    const long long rows = (long long)T * APQ_LM_C * (long long)sizeof(float), row = APQ_LM_C * (long long)sizeof(float);
    const long long poses = (long long)T * 12 * (long long)sizeof(double);
    if (out != in && ranges_overlap(in, rows, out, rows))
        return fail(APQ_ERR_INVALID, "rigid_register: out overlaps in without being in itself (in place means out == in)");
    if (ranges_overlap(std_face, row, out, rows)) return fail(APQ_ERR_INVALID, "rigid_register: out overlaps std");
    if (pose && ranges_overlap(pose, poses, out, rows)) return fail(APQ_ERR_INVALID, "rigid_register: pose overlaps out");
    if (pose && ranges_overlap(pose, poses, in, rows)) return fail(APQ_ERR_INVALID, "rigid_register: pose overlaps in");
    if (pose && ranges_overlap(pose, poses, std_face, row)) return fail(APQ_ERR_INVALID, "rigid_register: pose overlaps std");
    return APQ_OK;
}

}  // namespace apq
