// The face library's resamplers (include/animateportrait_face.h): pyramid levels and padded cut-outs by Pillow's 8-bit
// BILINEAR (bit-exact: both passes, the uint8 intermediate, coefficients in double tap by tap -- data/pil_resample.h), and the
// aligned picture by OpenCV's 8-bit INTER_CUBIC rule.  One thread per output pixel, its three channels together.
//
// A pixel's vertical taps each need the horizontally resampled, ROUNDED value of their row, so the thread runs the horizontal
// taps once per vertical tap.  Taps that fall outside the image read zero and add zero: they are skipped, which also bounds the
// work of a box far larger than the image by the image itself.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "face_checks.h"
#include "../data/pil_resample.h"

namespace {

using apf::fail;
constexpr int THREADS = 256;
constexpr int MAX_WINDOW = 4 * APF_MAX_SIDE;      // a box wider than this yields a black cut-out

struct Window {
    int x0, y0, w, h;
};

// Pillow's resize of the window (zero outside the H x W image) to ow x oh, at output pixel (ox, oy)
__device__ void bilinear_pixel(const uint8_t* img, int H, int W, Window win, int oh, int ow, int oy, int ox, uint8_t* dst) {
    const pil::BilinearAxis ax = pil::bilinear_axis(win.w, ow, ox), ay = pil::bilinear_axis(win.h, oh, oy);
    const int half = 1 << (pil::PRECISION_BITS - 1);
    // taps whose source lies inside the image
    const int tx0 = max(0, -win.x0 - ax.lo), tx1 = min(ax.n, W - win.x0 - ax.lo);
    const int ty0 = max(0, -win.y0 - ay.lo), ty1 = min(ay.n, H - win.y0 - ay.lo);
    int acc0 = half, acc1 = half, acc2 = half;
    for (int ty = ty0; ty < ty1; ++ty) {
        const int wy = pil::bilinear_weight(ay, ty);
        if (wy == 0) continue;
        const uint8_t* row = img + ((size_t)(win.y0 + ay.lo + ty) * W + (win.x0 + ax.lo)) * 3;
        int h0 = half, h1 = half, h2 = half;
        for (int tx = tx0; tx < tx1; ++tx) {
            const int wx = pil::bilinear_weight(ax, tx);
            const uint8_t* p = row + 3 * tx;
            h0 += (int)p[0] * wx;
            h1 += (int)p[1] * wx;
            h2 += (int)p[2] * wx;
        }
        acc0 += pil::clip8(h0) * wy;
        acc1 += pil::clip8(h1) * wy;
        acc2 += pil::clip8(h2) * wy;
    }
    dst[0] = (uint8_t)pil::clip8(acc0);
    dst[1] = (uint8_t)pil::clip8(acc1);
    dst[2] = (uint8_t)pil::clip8(acc2);
}

__global__ __launch_bounds__(THREADS) void resize_level_kernel(const uint8_t* img, int H, int W, int oh, int ow, uint8_t* out) {
    const int e = blockIdx.x * THREADS + threadIdx.x;
    if (e >= oh * ow) return;
    bilinear_pixel(img, H, W, Window{0, 0, W, H}, oh, ow, e / ow, e % ow, out + (size_t)e * 3);
}

__global__ __launch_bounds__(THREADS) void cutouts_kernel(const uint8_t* img, int H, int W, const double* boxes, const int32_t* count,
                                                           int cap, int size, uint8_t* out) {
    const int n = blockIdx.y;
    if (n >= min(*count, cap)) return;
    const int e = blockIdx.x * THREADS + threadIdx.x;
    if (e >= size * size) return;
    const double* b = boxes + (size_t)n * 5;
    const double w = b[2] - b[0] + 1.0, h = b[3] - b[1] + 1.0;
    uint8_t* dst = out + ((size_t)n * size * size + e) * 3;
    const double lim = (double)MAX_WINDOW;
    if (!(w >= 1.0 && h >= 1.0 && w <= lim && h <= lim && b[0] >= -lim && b[0] <= lim && b[1] >= -lim && b[1] <= lim)) {
        dst[0] = dst[1] = dst[2] = 0;                 // (also a NaN corner)
        return;
    }
    bilinear_pixel(img, H, W, Window{(int)b[0], (int)b[1], (int)w, (int)h}, size, size, e / size, e % size, dst);
}

// correct_bboxes writes through views of the caller's columns: the boxes leave get_image_boxes clipped to the image
__global__ void clip_boxes_kernel(double* boxes, const int32_t* count, int cap, int H, int W) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= min(*count, cap)) return;
    double* b = boxes + (size_t)n * 5;
    if (b[2] > W - 1.0) b[2] = W - 1.0;
    if (b[3] > H - 1.0) b[3] = H - 1.0;
    if (b[0] < 0.0) b[0] = 0.0;
    if (b[1] < 0.0) b[1] = 0.0;
}

// OpenCV's cubic taps of destination index d: first source index and four 11-bit weights
__device__ __forceinline__ int cubic_axis(int src, int dst, int d, int* wq) {
    const double scale = 1.0 / ((double)dst / (double)src);
    const float f = (float)((d + 0.5) * scale - 0.5);
    const float fl = floorf(f);
    const float x = f - fl;
    const float A = -0.75f;
    float c[4];
    c[0] = ((A * (x + 1.f) - 5.f * A) * (x + 1.f) + 8.f * A) * (x + 1.f) - 4.f * A;
    c[1] = ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f;
    c[2] = ((A + 2.f) * (1.f - x) - (A + 3.f)) * (1.f - x) * (1.f - x) + 1.f;
    c[3] = 1.f - c[0] - c[1] - c[2];
    for (int k = 0; k < 4; ++k) {
        const float q = rintf(c[k] * 2048.f);
        wq[k] = (int)fminf(fmaxf(q, -32768.f), 32767.f);
    }
    return (int)fl - 1;
}

__global__ __launch_bounds__(THREADS) void crop_resize_cubic_kernel(const uint8_t* img, int H, int W, int x0, int y0, int size,
                                                                     int fill, int out_size, uint8_t* out) {
    const int e = blockIdx.x * THREADS + threadIdx.x;
    if (e >= out_size * out_size) return;
    int wx[4], wy[4];
    const int sx = cubic_axis(size, out_size, e % out_size, wx), sy = cubic_axis(size, out_size, e / out_size, wy);
    long long acc[3] = {0, 0, 0};
    for (int ky = 0; ky < 4; ++ky) {
        const int cy = pil::clampi(sy + ky, 0, size - 1) + y0;
        int row[3] = {0, 0, 0};
        for (int kx = 0; kx < 4; ++kx) {
            const int cx = pil::clampi(sx + kx, 0, size - 1) + x0;
            const bool inside = cy >= 0 && cy < H && cx >= 0 && cx < W;
            const uint8_t* p = img + ((size_t)(inside ? cy : 0) * W + (inside ? cx : 0)) * 3;
            for (int c = 0; c < 3; ++c) row[c] += (inside ? (int)p[c] : fill) * wx[kx];
        }
        for (int c = 0; c < 3; ++c) acc[c] += (long long)row[c] * wy[ky];
    }
    for (int c = 0; c < 3; ++c) {
        const long long v = (acc[c] + (1 << 21)) >> 22;
        out[(size_t)e * 3 + c] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
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

int32_t apf_abi_version(void) { return APF_ABI_VERSION; }

const char* apf_last_error(void) { return apf::err_buf(); }

int32_t apf_resize_level_ok(const uint8_t* img, int32_t H, int32_t W, int32_t oh, int32_t ow, const uint8_t* out) {
    return apf::check_resize_level(img, H, W, oh, ow, out) == APF_OK ? 1 : 0;
}

int apf_resize_level(const uint8_t* img, int32_t H, int32_t W, int32_t oh, int32_t ow, uint8_t* out, void* stream) {
    const int rc = apf::check_resize_level(img, H, W, oh, ow, out);
    if (rc != APF_OK) return rc;
    (void)hipGetLastError();
    hipLaunchKernelGGL(resize_level_kernel, dim3((oh * ow + THREADS - 1) / THREADS), dim3(THREADS), 0, (hipStream_t)stream, img, H, W, oh, ow, out);
    return launched("resize_level");
}

int32_t apf_cutouts_ok(const uint8_t* img, int32_t H, int32_t W, const double* boxes, const int32_t* count, int32_t cap, int32_t size,
                       const uint8_t* out) {
    return apf::check_cutouts(img, H, W, boxes, count, cap, size, out) == APF_OK ? 1 : 0;
}

int apf_cutouts(const uint8_t* img, int32_t H, int32_t W, double* boxes, const int32_t* count, int32_t cap, int32_t size, uint8_t* out,
                void* stream) {
    const int rc = apf::check_cutouts(img, H, W, boxes, count, cap, size, out);
    if (rc != APF_OK) return rc;
    (void)hipGetLastError();
    hipLaunchKernelGGL(cutouts_kernel, dim3((size * size + THREADS - 1) / THREADS, cap), dim3(THREADS), 0, (hipStream_t)stream, img, H, W,
                       (const double*)boxes, count, cap, size, out);
    hipLaunchKernelGGL(clip_boxes_kernel, dim3((cap + THREADS - 1) / THREADS), dim3(THREADS), 0, (hipStream_t)stream, boxes, count, cap, H, W);
    return launched("cutouts");
}

int32_t apf_crop_resize_cubic_ok(const uint8_t* img, int32_t H, int32_t W, int32_t x0, int32_t y0, int32_t size, int32_t out_size,
                                 const uint8_t* out) {
    return apf::check_crop_resize_cubic(img, H, W, x0, y0, size, out_size, out) == APF_OK ? 1 : 0;
}

int apf_crop_resize_cubic(const uint8_t* img, int32_t H, int32_t W, int32_t x0, int32_t y0, int32_t size, int32_t fill, int32_t out_size,
                          uint8_t* out, void* stream) {
    const int rc = apf::check_crop_resize_cubic(img, H, W, x0, y0, size, out_size, out);
    if (rc != APF_OK) return rc;
    if (fill < 0 || fill > 255) return fail(APF_ERR_INVALID, "crop_resize_cubic: fill %ld is no byte", fill);
    (void)hipGetLastError();
    hipLaunchKernelGGL(crop_resize_cubic_kernel, dim3((out_size * out_size + THREADS - 1) / THREADS), dim3(THREADS), 0, (hipStream_t)stream,
                       img, H, W, x0, y0, size, fill, out_size, out);
    return launched("crop_resize_cubic");
}

}  // extern "C"
