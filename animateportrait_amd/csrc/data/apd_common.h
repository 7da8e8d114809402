// What the translation units of libapdata.so share: the thread-local error message apd_last_error() returns.
#pragma once

namespace apd {

extern thread_local char g_err[256];

// writes the message, returns `code`
int fail(int code, const char* fmt, long a = 0, long b = 0, long c = 0, long d = 0);

#ifdef __HIPCC__
// The byte of apd_frames_to_u8 and apd_png_encode: ((x + 1) / 2 * 255) truncated, as numpy computes it in float32; the files
// that use it are compiled with -ffp-contract=off
__device__ __forceinline__ unsigned to_byte(float x) {
    const float v = (x + 1.0f) / 2.0f * 255.0f;
    if (!(v > 0.0f)) return 0u;              // also NaN
    if (v >= 255.0f) return 255u;
    return (unsigned)(int)v;
}
#endif

}  // namespace apd
