// apd_frames_to_u8: tensor2im for a batch, fp32 NCHW in [-1, 1] -> uint8 NHWC with three channels
// (include/animateportrait_data.h).
//
// The destination of a batch is one contiguous run of N H W 3 bytes, so it is written as packed dwords whatever W is: lane d
// builds bytes 4d .. 4d + 3 (they belong to two neighbouring pixels; consecutive lanes read consecutive columns of each
// channel plane) and stores one dword; the last N H W 3 mod 4 bytes are stored one by one.  The destination may be pinned
// host memory: dword stores keep the traffic over the link in full words.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../../include/animateportrait_data.h"
#include "apd_common.h"

namespace {

using apd::fail;
using apd::to_byte;          // apd_common.h: shared with png_encode.hip

constexpr int THREADS = 256;

// byte b of the destination: pixel b / 3, channel b % 3
__device__ __forceinline__ unsigned byte_at(const float* __restrict__ src, long long b, int C, long long plane) {
    const long long pix = b / 3;
    const int ch = (int)(b - pix * 3);
    const long long n = pix / plane, p = pix - n * plane;
    return to_byte(src[(n * C + (C == 3 ? ch : 0)) * plane + p]);
}

__global__ __launch_bounds__(THREADS) void frames_to_u8_kernel(const float* __restrict__ src, uint8_t* __restrict__ dst, int C,
                                                               long long plane, long long total) {
    const long long d = (long long)blockIdx.x * THREADS + threadIdx.x, words = total >> 2;
    if (d < words) {
        const long long b = d * 4;
        const unsigned w = byte_at(src, b, C, plane) | (byte_at(src, b + 1, C, plane) << 8) |
                           (byte_at(src, b + 2, C, plane) << 16) | (byte_at(src, b + 3, C, plane) << 24);
        reinterpret_cast<uint32_t*>(dst)[d] = w;
    } else if (d - words < (total & 3)) {
        const long long b = words * 4 + (d - words);
        dst[b] = (uint8_t)byte_at(src, b, C, plane);
    }
}

int check_frames(const float* src, const uint8_t* dst, int N, int C, int H, int W) {
    if (!src || !dst) return fail(APD_ERR_INVALID, "frames_to_u8: null src / dst");
    if (C != 1 && C != 3) return fail(APD_ERR_UNSUPPORTED, "frames_to_u8: C = %ld, served: 1 and 3", C);
    if (N < 1 || H < 1 || W < 1) return fail(APD_ERR_INVALID, "frames_to_u8: empty batch %ld x %ld x %ld", N, H, W);
    if ((long long)N * H * W * 3 >= (1LL << 31)) return fail(APD_ERR_UNSUPPORTED, "frames_to_u8: %ld x %ld x %ld x 3 bytes, served: below 2^31", N, H, W);
    if (((uintptr_t)dst & 3) != 0) return fail(APD_ERR_INVALID, "frames_to_u8: dst is not 4-byte aligned");
    return APD_OK;
}

}  // namespace

extern "C" {

int32_t apd_frames_to_u8_ok(const float* src, const uint8_t* dst, int32_t N, int32_t C, int32_t H, int32_t W) {
    return check_frames(src, dst, N, C, H, W) == APD_OK ? 1 : 0;
}

int apd_frames_to_u8(const float* src, int32_t N, int32_t C, int32_t H, int32_t W, uint8_t* dst, void* stream) {
    const int rc = check_frames(src, dst, N, C, H, W);
    if (rc != APD_OK) return rc;
    // where does dst live?  Device memory is written as it is; pinned host memory through the address the device maps it at;
    // anything else (pageable host memory) would fault and is refused.
    hipPointerAttribute_t attr;
    (void)hipGetLastError();
    const hipError_t pe = hipPointerGetAttributes(&attr, dst);
    uint8_t* target = nullptr;
    if (pe == hipSuccess && attr.type == hipMemoryTypeDevice) target = dst;
    else if (pe == hipSuccess && attr.type == hipMemoryTypeHost) target = static_cast<uint8_t*>(attr.devicePointer);
    if (pe != hipSuccess) (void)hipGetLastError();
    if (!target || ((uintptr_t)target & 3) != 0)
        return fail(APD_ERR_INVALID, "frames_to_u8: dst is neither device memory nor pinned host memory mapped for the device");
    const long long plane = (long long)H * W, total = (long long)N * plane * 3;
    const long long lanes = (total >> 2) + (total & 3);
    hipLaunchKernelGGL(frames_to_u8_kernel, dim3((unsigned)((lanes + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream,
                       src, target, C, plane, total);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(apd::g_err, sizeof(apd::g_err), "frames_to_u8: launch failed: %s", hipGetErrorString(e));
        return APD_ERR_LAUNCH;
    }
    return APD_OK;
}

}  // extern "C"
