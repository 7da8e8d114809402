/*
 * animateportrait_data.h -- C ABI of libapdata.so: batch preparation for the umlvd_ifw dataset on the MI355X (gfx950).
 *
 * This library is NOT part of the model boundary (include/animateportrait_amd.h, libapamd.so): an integrator of the
 * model binds that one and feeds it tensors from whatever data layer they have.  libapdata.so serves this project's own
 * data layer (animateportrait_amd/data/umlvd_ifw_dataset.py), where the reference runs torchvision / PIL on the CPU
 * (Module2/data/base_dataset.py:153-213).
 *
 * Conventions: as in animateportrait_amd.h -- device pointers, caller-owned buffers, calls only enqueue on `stream`
 * (a hipStream_t as void*), 0 = ok, negative = error with a thread-local message (apd_last_error()).  A refused call
 * launches nothing and writes nothing.
 */
#ifndef ANIMATEPORTRAIT_DATA_H
#define ANIMATEPORTRAIT_DATA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define APD_ABI_VERSION 1

enum { APD_OK = 0, APD_ERR_INVALID = -1, APD_ERR_UNSUPPORTED = -2, APD_ERR_LAUNCH = -3 };

/* served region of apd_image_prep_u8 */
#define APD_MAX_TAPS 64        /* taps per output pixel and axis: bicubic down-scaling by up to ~15x */
#define APD_MAX_SOURCE 8192    /* source height / width */
#define APD_MAX_LOAD 4096      /* resized height / width */
#define APD_MAX_IMAGES 65535   /* images per launch */

int32_t apd_abi_version(void);
const char* apd_last_error(void);

/* [Grayscale ->] Resize(load, BICUBIC) -> crop -> horizontal flip -> ToTensor [-> Normalize] of a batch of decoded 8-bit
 * images (Module2/data/base_dataset.py:153-213 get_transform / get_transform_mask), bit-exact against Pillow:
 * its 8-bit resampler is integer arithmetic -- weights rounded to 22 fractional bits, the horizontal pass rounded and
 * clipped to uint8, then the vertical pass, rounded and clipped again.
 *
 * Tables (one per axis, built by the caller as Pillow's precompute_coeffs + normalize_coeffs_8bpc build them):
 *   bounds  (load, 2) int32: first source index, number of taps (<= k)
 *   weights (load, k) int32: the taps, zero past the count
 * An axis whose size does not change has k == 0 and no table: its pass is skipped, as Pillow skips it.
 * The kernel clamps every index it reads from a table or from `params` into the source, so wrong tables give wrong
 * pixels, never a wild access. */
typedef struct apd_image_prep {
    int32_t N, Hs, Ws, C;     /* source: (N, Hs, Ws, C) uint8, interleaved; C = 1 or 3 */
    int32_t load_w, load_h;   /* size after the resize */
    int32_t crop;             /* output height = width */
    int32_t to_gray;          /* C == 3: convert to L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16 BEFORE resampling */
    int32_t kh, kv;           /* taps per row of the horizontal / vertical table; 0 iff Ws == load_w / Hs == load_h,
                                 else Pillow's ksize = 2 ceil(2 max(1, in / out)) + 1 */
    int32_t max_x, max_y;     /* the largest crop offsets in `params`: max_x + crop <= load_w, max_y + crop <= load_h */
} apd_image_prep;

/* 1 when apd_image_prep_u8 serves the description, else 0 with the reason in apd_last_error().  Needs no device. */
int32_t apd_image_prep_ok(const apd_image_prep* d);

/* src     (N, Hs, Ws, C) uint8
 * params  (N, 3) int32: crop x, crop y (in the resized image), flip (0 / 1)
 * lut     256 floats: the value written for each 8-bit result ((v/255 - 0.5)/0.5 for images, v/255 for masks)
 * out     (N, OC, crop, crop) float32, OC = 3 when C == 3 and !to_gray, else 1
 * One launch; only the crop window is computed. */
int apd_image_prep_u8(const apd_image_prep* d, const uint8_t* src, const int32_t* params,
                      const int32_t* hbounds, const int32_t* hweights, const int32_t* vbounds, const int32_t* vweights,
                      const float* lut, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
