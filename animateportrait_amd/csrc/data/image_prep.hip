// apd_image_prep_u8: [Grayscale ->] Resize(BICUBIC) -> crop -> flip -> ToTensor [-> Normalize] of a batch of decoded 8-bit
// images in one launch, bit-exact against Pillow's 8-bit resampler (include/animateportrait_data.h).
//
// One workgroup per TH x TW tile of the crop window.  Stage 1 resamples, horizontally, the source rows the tile's vertical
// taps need (mirrored columns when the image is flipped), rounds and clips to uint8 and keeps them in LDS: that uint8 image
// is Pillow's intermediate, and the rounding in it is part of the result.  Stage 2 runs the vertical taps from LDS, clips,
// looks the byte up in the caller's 256-entry table and stores fp32 NCHW.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <math.h>

#include "../../../include/animateportrait_data.h"
#include "apd_common.h"
#include "pil_resample.h"

namespace apd {

thread_local char g_err[256];

int fail(int code, const char* fmt, long a, long b, long c, long d) {
    snprintf(g_err, sizeof(g_err), fmt, a, b, c, d);
    return code;
}

}  // namespace apd

namespace {

using apd::fail;
using apd::g_err;

constexpr int TW = 64, TH = 16, THREADS = 256;
using pil::PRECISION_BITS;                       // Pillow: Resample.c (pil_resample.h, shared with the face library)
using pil::clampi;
using pil::clip8;
constexpr int MAX_LDS_BYTES = 48 * 1024;

// Pillow's ksize for one axis; 0 when the axis keeps its size (the pass is skipped)
int expected_taps(int in, int out) {
    if (in == out) return 0;
    double scale = (double)in / (double)out;
    if (scale < 1.0) scale = 1.0;
    return (int)ceil(2.0 * scale) * 2 + 1;
}

// rows of the horizontally resampled intermediate one tile can need: the centres of TH output rows span (TH - 1) * scale
// source rows, the taps of the first and last reach half a kernel beyond, and both ends round
int tile_rows(int Hs, int load_h, int kv) {
    if (kv == 0) return TH;
    double scale = (double)Hs / (double)load_h;
    return (int)ceil((TH - 1) * scale) + kv + 2;
}

struct Args {
    const uint8_t* src;
    const int32_t* params;
    const int32_t *hb, *hw, *vb, *vw;
    const float* lut;
    float* out;
    int Hs, Ws, C, OC, gray, load_w, load_h, crop, kh, kv, rows_cap;
};

// one 8-bit sample of channel ch at column col of an interleaved row
__device__ __forceinline__ int fetch(const uint8_t* row, int col, int C, int ch, int gray) {
    if (C == 1) return row[col];
    const uint8_t* p = row + 3 * col;
    if (gray) return (19595 * (int)p[0] + 38470 * (int)p[1] + 7471 * (int)p[2] + 0x8000) >> 16;
    return p[ch];
}

__global__ __launch_bounds__(THREADS) void image_prep_kernel(Args a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t tile[];       // [rows][OC][TW]
    const int n = blockIdx.z, ox0 = blockIdx.x * TW, oy0 = blockIdx.y * TH;
    const int tw = min(TW, a.crop - ox0), th = min(TH, a.crop - oy0);
    const int cx = clampi(a.params[3 * n], 0, a.load_w - a.crop);
    const int cy = clampi(a.params[3 * n + 1], 0, a.load_h - a.crop);
    const int flip = a.params[3 * n + 2] != 0;
    const int ry0 = cy + oy0;                                              // first resized row of the tile

    int r0, rows;                                                          // source rows [r0, r0 + rows) go to LDS
    if (a.kv) {
        const int last = ry0 + th - 1;
        r0 = clampi(a.vb[2 * ry0], 0, a.Hs);
        int end = clampi(a.vb[2 * last], 0, a.Hs) + clampi(a.vb[2 * last + 1], 0, a.kv);
        end = min(end, a.Hs);
        rows = clampi(end - r0, 0, a.rows_cap);
    } else {
        r0 = ry0;                                                          // Hs == load_h: r0 + th <= Hs
        rows = th;
    }

    const uint8_t* img = a.src + (size_t)n * a.Hs * a.Ws * a.C;
    for (int e = threadIdx.x; e < rows * a.OC * TW; e += THREADS) {
        const int c = e % TW, ch = (e / TW) % a.OC, r = e / (TW * a.OC);
        if (c >= tw) continue;
        const int ox = ox0 + c;
        const int rx = cx + (flip ? a.crop - 1 - ox : ox);                 // column of the resized image
        const uint8_t* row = img + (size_t)(r0 + r) * a.Ws * a.C;
        int v;
        if (a.kh) {
            const int xmin = clampi(a.hb[2 * rx], 0, a.Ws);
            const int cnt = min(clampi(a.hb[2 * rx + 1], 0, a.kh), a.Ws - xmin);
            const int32_t* w = a.hw + (size_t)rx * a.kh;
            int acc = 1 << (PRECISION_BITS - 1);
            for (int t = 0; t < cnt; ++t) acc += fetch(row, xmin + t, a.C, ch, a.gray) * w[t];
            v = clip8(acc);
        } else {
            v = fetch(row, rx, a.C, ch, a.gray);                           // Ws == load_w: rx < Ws
        }
        tile[e] = (uint8_t)v;
    }
    __syncthreads();

    for (int e = threadIdx.x; e < th * a.OC * TW; e += THREADS) {
        const int c = e % TW, ch = (e / TW) % a.OC, orow = e / (TW * a.OC);
        if (c >= tw) continue;
        int v;
        if (a.kv) {
            const int ry = ry0 + orow;
            const int s = clampi(a.vb[2 * ry], 0, a.Hs) - r0;              // LDS row of the first tap
            const int cnt = clampi(a.vb[2 * ry + 1], 0, a.kv);
            const int tlo = max(0, -s), thi = min(cnt, rows - s);          // (whole range for tables that ascend, as Pillow's do)
            const int32_t* w = a.vw + (size_t)ry * a.kv;
            int acc = 1 << (PRECISION_BITS - 1);
            for (int t = tlo; t < thi; ++t) acc += (int)tile[((s + t) * a.OC + ch) * TW + c] * w[t];
            v = clip8(acc);
        } else {
            v = tile[(orow * a.OC + ch) * TW + c];
        }
        a.out[(((size_t)n * a.OC + ch) * a.crop + (oy0 + orow)) * a.crop + ox0 + c] = a.lut[v];
    }
}

int check_desc(const apd_image_prep* d) {
    if (!d) return fail(APD_ERR_INVALID, "image_prep: null description");
    if (d->C != 1 && d->C != 3) return fail(APD_ERR_UNSUPPORTED, "image_prep: C = %ld, served: 1 and 3", d->C);
    if (d->N < 1 || d->N > APD_MAX_IMAGES) return fail(APD_ERR_UNSUPPORTED, "image_prep: N = %ld, served: 1..%ld", d->N, APD_MAX_IMAGES);
    if (d->Hs < 1 || d->Ws < 1 || d->Hs > APD_MAX_SOURCE || d->Ws > APD_MAX_SOURCE)
        return fail(APD_ERR_UNSUPPORTED, "image_prep: source %ld x %ld, served: 1..%ld per axis", d->Hs, d->Ws, APD_MAX_SOURCE);
    if (d->load_w < 1 || d->load_h < 1 || d->load_w > APD_MAX_LOAD || d->load_h > APD_MAX_LOAD)
        return fail(APD_ERR_UNSUPPORTED, "image_prep: load size %ld x %ld, served: 1..%ld per axis", d->load_h, d->load_w, APD_MAX_LOAD);
    if (d->crop < 1 || d->crop > d->load_w || d->crop > d->load_h)
        return fail(APD_ERR_INVALID, "image_prep: crop %ld does not fit the load size %ld x %ld", d->crop, d->load_h, d->load_w);
    if (d->max_x < 0 || d->max_y < 0 || d->max_x > d->load_w - d->crop || d->max_y > d->load_h - d->crop)
        return fail(APD_ERR_INVALID, "image_prep: crop offset (%ld, %ld) + crop %ld leaves the resized image", d->max_x, d->max_y, d->crop);
    const int kh = expected_taps(d->Ws, d->load_w), kv = expected_taps(d->Hs, d->load_h);
    if (kh > APD_MAX_TAPS || kv > APD_MAX_TAPS)
        return fail(APD_ERR_UNSUPPORTED, "image_prep: %ld x %ld taps, served: up to %ld per axis", kv, kh, APD_MAX_TAPS);
    if (d->kh != kh || d->kv != kv)
        return fail(APD_ERR_INVALID, "image_prep: tables of %ld x %ld taps, these sizes need %ld x %ld", d->kv, d->kh, kv, kh);
    const int oc = (d->C == 3 && !d->to_gray) ? 3 : 1;
    const long lds = (long)tile_rows(d->Hs, d->load_h, kv) * oc * TW;
    if (lds > MAX_LDS_BYTES)
        return fail(APD_ERR_UNSUPPORTED, "image_prep: a tile needs %ld bytes of LDS, served: up to %ld", lds, MAX_LDS_BYTES);
    return APD_OK;
}

}  // namespace

extern "C" {

int32_t apd_abi_version(void) { return APD_ABI_VERSION; }

const char* apd_last_error(void) { return g_err; }

int32_t apd_image_prep_ok(const apd_image_prep* d) { return check_desc(d) == APD_OK ? 1 : 0; }

int apd_image_prep_u8(const apd_image_prep* d, const uint8_t* src, const int32_t* params, const int32_t* hbounds,
                      const int32_t* hweights, const int32_t* vbounds, const int32_t* vweights, const float* lut, float* out,
                      void* stream) {
    const int rc = check_desc(d);
    if (rc != APD_OK) return rc;
    if (!src || !params || !lut || !out) return fail(APD_ERR_INVALID, "image_prep: null src / params / lut / out");
    if (d->kh && (!hbounds || !hweights)) return fail(APD_ERR_INVALID, "image_prep: the width changes but there is no horizontal table");
    if (d->kv && (!vbounds || !vweights)) return fail(APD_ERR_INVALID, "image_prep: the height changes but there is no vertical table");
    Args a;
    a.src = src; a.params = params; a.hb = hbounds; a.hw = hweights; a.vb = vbounds; a.vw = vweights; a.lut = lut; a.out = out;
    a.Hs = d->Hs; a.Ws = d->Ws; a.C = d->C; a.gray = d->to_gray != 0;
    a.OC = (d->C == 3 && !d->to_gray) ? 3 : 1;
    a.load_w = d->load_w; a.load_h = d->load_h; a.crop = d->crop; a.kh = d->kh; a.kv = d->kv;
    a.rows_cap = tile_rows(d->Hs, d->load_h, d->kv);
    const size_t lds = ((size_t)a.rows_cap * a.OC * TW + 15) & ~(size_t)15;
    dim3 grid((d->crop + TW - 1) / TW, (d->crop + TH - 1) / TH, d->N);
    (void)hipGetLastError();      // an error an earlier, unrelated call left on this thread is not this launch's
    hipLaunchKernelGGL(image_prep_kernel, grid, dim3(THREADS), lds, (hipStream_t)stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(g_err, sizeof(g_err), "image_prep: launch failed: %s", hipGetErrorString(e));
        return APD_ERR_LAUNCH;
    }
    return APD_OK;
}

}  // extern "C"
