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

/* ---- the test-time item (data/umlvdfw_test_dataset.py) and the PNG sink of test.py.  Added without changing any call
 * above, so APD_ABI_VERSION stays 1; a binding finds a library that predates them by the missing symbol. */

#define APD_MAX_SEGMENTS 128   /* contour segments per landmark map */
#define APD_MAX_RADIUS 31      /* disc radius */
#define APD_MAX_THICKNESS 16   /* line thickness */
#define APD_MAX_MAP 1024       /* landmark map height / width */
#define APD_MAX_POINTS 1024    /* landmarks per sample */

/* draw2(height, width, lands, radius, thickness, op = 0 | 1) (Module2/data/umlvdfw_test_dataset.py:34-52) for a batch.
 *   lm        device (N, P, 2) float32 (x, y); rounded half-to-even to int as np.round(...).astype(int) does, then clamped
 *             to +-2^20 (NaN goes to -2^20)
 *   seg       device (S, 2) int32 landmark indices (faceLmarkLookup.npy); may be null when S == 0 or op == 0
 *   seg_host  the same table on the host: every index is checked against P here, before the launch.  The kernel clamps
 *             what it reads from `seg` into [0, P), so a device table that differs gives wrong pixels, never a wild access.
 *   out       device (N, 1, H, W) float32, every element written: `hi` on a mark, `lo` elsewhere (no memset needed)
 * op 0: the union of filled cv2.circle(radius) discs -- bit-equal to ap_landmark_discs, which tests pixels through the same
 *       header (csrc/cv_raster.h: round_coord, circle_rows, circle_covers).
 * op 1: the discs, then the union of cv2.line(start, end, color, thickness) over the segments by OpenCV 4.2's ThickLine
 *       rule as oracle/cv_raster.thick_line restates it: the quad through FillConvexPoly at 16.16 fixed point plus a filled
 *       circle of radius (thickness + 1) >> 1 at both ends.  thickness 1 follows the same quad rule (cv2 itself draws a
 *       Bresenham line there; the reference uses 2 and 4).
 * Marks are clipped to the image; a point or segment wholly outside draws nothing.
 * Served: N 1..65535, P 1..APD_MAX_POINTS, S 0..APD_MAX_SEGMENTS, H, W 1..APD_MAX_MAP, radius 0..APD_MAX_RADIUS,
 * thickness 1..APD_MAX_THICKNESS.  apd_landmark_map_ok needs no device and checks everything but the device pointers'
 * contents. */
int32_t apd_landmark_map_ok(const float* lm, const int32_t* seg, const int32_t* seg_host, const float* out, int32_t N,
                            int32_t P, int32_t S, int32_t H, int32_t W, int32_t radius, int32_t thickness, int32_t op);
int apd_landmark_map(const float* lm, const int32_t* seg, const int32_t* seg_host, int32_t N, int32_t P, int32_t S,
                     int32_t H, int32_t W, int32_t radius, int32_t thickness, int32_t op, float lo, float hi, float* out,
                     void* stream);

/* get_lmvis (Module2/models/geomcgt_ifw_test_model.py:232-251) per sample.
 *   frames  device (N, C, H, W) float32, C = 1 or 3     lm  device (N, P, 2) float32 (x, y)
 *   win     device (N, 4) int32: x1, x2, y1, y2          out device (N, 3, H, W) float32, must not overlap frames
 * out = frames (grey tiled to 3 channels) with channel 0 = 1 and channels 1, 2 = -1 inside
 *   [y - h, y + h) x [x - h, x + h) around every rounded (half to even) landmark, h = hradius, and the four bars
 *   rows [y1 - h, y1 + h) and [y2 - h, y2 + h) over columns [x1 - h, x2 + h); columns [x1 - h, x1 + h) and
 *   [x2 - h, x2 + h) over rows [y1 - h, y2 + h).  Every box is clipped to the image.
 * Served: N 1..65535, P 1..APD_MAX_POINTS, H, W 1..4096, hradius 0..64. */
int32_t apd_landmark_marks_ok(const float* frames, const float* lm, const int32_t* win, const float* out, int32_t N,
                              int32_t C, int32_t P, int32_t H, int32_t W, int32_t hradius);
int apd_landmark_marks(const float* frames, const float* lm, const int32_t* win, int32_t N, int32_t C, int32_t P,
                       int32_t H, int32_t W, int32_t hradius, float* out, void* stream);

/* tensor2im (Module2/util/util.py:9-29) for a batch: src device (N, C, H, W) float32, C = 1 or 3 -> dst (N, H, W, 3) uint8,
 * grey tiled to three channels.  byte = (uint8)((x + 1) / 2 * 255) in unfused float32, truncated.  Results below 0 (and
 * NaN) give 0, results of 255 and above give 255: numpy's cast is undefined there, this contract is not.
 * dst is 4-byte aligned and is either device memory or pinned host memory mapped for the device (hipHostMalloc): the
 * call asks the runtime which (hipPointerGetAttributes) and refuses any other pointer.  The host sees the bytes once the
 * stream has been synchronised.  Served: N, H, W >= 1 with N H W 3 < 2^31. */
int32_t apd_frames_to_u8_ok(const float* src, const uint8_t* dst, int32_t N, int32_t C, int32_t H, int32_t W);
int apd_frames_to_u8(const float* src, int32_t N, int32_t C, int32_t H, int32_t W, uint8_t* dst, void* stream);

/* ---- PNG files encoded on the device: the opt-in sink of test.py / end2end.py (--png_encoder device).  Added as above:
 * APD_ABI_VERSION stays 1. */

#define APD_MAX_PNG_SIDE 2048  /* frame height / width */

/* One complete PNG file per frame of src, device (N, C, H, W) float32: 8-bit samples, no interlace; channels 3 = colour
 * type 2 with grey tiled to RGB, channels 1 = colour type 0 (needs C == 1).  The pixel bytes are apd_frames_to_u8's.
 *   dst      N slots of slot_bytes each; frame n's file is dst[n slot_bytes .. n slot_bytes + sizes[n]): signature, IHDR, IDAT
 *            chunks, IEND.  Bytes of a slot past sizes[n] are not written.
 *   sizes    N int32
 *   ws       device workspace of at least apd_png_workspace_bytes(N, H, W, channels) bytes, owned by the caller; its
 *            contents mean nothing between calls
 * dst and sizes are 4-byte aligned and each either device memory or pinned host memory mapped for the device (the rule of
 * apd_frames_to_u8: pageable memory is refused).  The call enqueues two launches on `stream` and does not synchronise; no
 * atomics touch the output, and the same input gives the same bytes.
 * Stream: the frame is cut into bands of R = min(16, 16384 / (W channels + 1)) rows; a band is filtered on its own (first row
 * Sub, the others Up against the image's row above) and is one fixed-Huffman deflate block -- literals and runs at distance
 * 1 -- closed by an empty stored block, in an IDAT chunk of its own; a last 9-byte IDAT chunk ends the zlib stream with the
 * Adler-32.  Any PNG decoder reads it; it is larger than what zlib's search would give.
 * apd_png_bound: bytes of a slot that hold any frame of that shape, a multiple of 4, at most
 *   9/8 H (W channels + 1) + 64 H + 256; -1 (with a message) outside the served region.
 * Served: N 1..65535, C 1 or 3, channels 1 or 3 (1 only with C == 1), H, W 1..APD_MAX_PNG_SIDE, slot_bytes a multiple of 4
 * and >= apd_png_bound, N slot_bytes < 2^31.  apd_png_encode_ok needs no device and checks everything but where the
 * pointers live. */
int64_t apd_png_bound(int32_t H, int32_t W, int32_t channels);
int64_t apd_png_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t channels);
int32_t apd_png_encode_ok(const float* src, const uint8_t* dst, const int32_t* sizes, const void* ws, int32_t N, int32_t C,
                          int32_t H, int32_t W, int32_t channels, int64_t slot_bytes, int64_t ws_bytes);
int apd_png_encode(const float* src, int32_t N, int32_t C, int32_t H, int32_t W, int32_t channels, uint8_t* dst,
                   int64_t slot_bytes, int32_t* sizes, void* ws, int64_t ws_bytes, void* stream);

/* ---- baseline JPEG files encoded on the device: the frames of an MJPEG clip (end2end.py --video avi, util/avi.py).  Added
 * as above: APD_ABI_VERSION stays 1. */

#define APD_MAX_JPEG_SIDE 2048  /* frame height / width */

/* One complete baseline JPEG file per frame of src, device (N, C, H, W) float32.  The sample bytes are apd_frames_to_u8's.
 * channels 1 (needs C == 1): one component.  channels 3: Y Cb Cr, every component sampled 1x1 (4:4:4), grey tiled to RGB
 * first when C == 1.
 *   dst      N slots of slot_bytes each; frame n's file is dst[n slot_bytes .. n slot_bytes + sizes[n]).  Bytes of a slot past
 *            sizes[n] are not written.
 *   sizes    N int32
 *   quality  1..100: the tables of ITU T.81 Annex K.1 / K.2 scaled by the IJG rule, s = quality < 50 ? 5000 / quality :
 *            200 - 2 quality, t = clamp((base s + 50) / 100, 1, 255) -- the tables PIL's save(quality=) writes
 *   ws       device workspace of at least apd_jpeg_workspace_bytes(N, H, W, channels) bytes, owned by the caller; its
 *            contents mean nothing between calls
 * dst and sizes are 4-byte aligned and each either device memory or pinned host memory mapped for the device (the rule of
 * apd_frames_to_u8: pageable memory is refused).  The call enqueues three launches on `stream`, starts no stream of its own
 * and does not synchronise; no atomics touch global memory, and the same input gives the same bytes.
 * File: SOI, JFIF APP0, DQT (one table for channels 1, two for 3), SOF0 (8 bit, the true H and W), DHT (always the four
 * tables of Annex K.3), DRI, SOS, the scan, EOI at sizes[n] - 2.  Edges are padded to a multiple of 8 by replicating the
 * last column / row.  The restart interval is ceil(W / 8) MCUs, one MCU row: every row is a byte-aligned segment with its
 * DC prediction reset, padded with 1-bits and followed by RSTm (m = row mod 8) unless it is the last; a segment is encoded
 * by one workgroup, independently of every other.
 * Arithmetic, integers only (csrc/data/jpeg_core.h; a host build gives the same bytes):
 *   colour    Y = (19595 R + 38470 G + 7471 B + 2^15) >> 16, Cb = (-11059 R - 21709 G + 32768 B + 128 2^16 + 2^15 - 1) >> 16,
 *             Cr = (32768 R - 27439 G - 5329 B + 128 2^16 + 2^15 - 1) >> 16: the JFIF matrix at 16 fractional bits; grey
 *             gives Cb = Cr = 128 exactly
 *   DCT       separable, on samples - 128, cosines C(u) / 2 cos((2 x + 1) u pi / 16) rounded to 20 fractional bits: the row
 *             pass in int32, kept whole; the column pass accumulated in int64 and rounded half up to 20 fractional bits
 *             (an int32); the DC term is not taken from the passes, it is the sum of the samples / 8 exactly
 *   quantise  sign(v) ((|v| + q 2^19) / (q 2^20)): round half away from zero; AC levels clamped to +-1023
 * apd_jpeg_bound: bytes of a slot that hold any frame of that shape, a multiple of 4: a symbol is at most 26 bits, a block
 * 64 symbols = 208 bytes, 416 once every byte is stuffed, so header (613 bytes at most) + ceil(H / 8) (416 blocks per row
 * + 2) + 2, rounded up; -1 (with a message) outside the served region.
 * Served: N 1..65535, C 1 or 3, channels 1 or 3 (1 only with C == 1), H, W 1..APD_MAX_JPEG_SIDE, quality 1..100, slot_bytes
 * a multiple of 4 and >= apd_jpeg_bound, N slot_bytes < 2^31.  apd_jpeg_encode_ok needs no device and checks everything but
 * where the pointers live. */
int64_t apd_jpeg_bound(int32_t H, int32_t W, int32_t channels);
int64_t apd_jpeg_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t channels);
int32_t apd_jpeg_encode_ok(const float* src, const uint8_t* dst, const int32_t* sizes, const void* ws, int32_t N, int32_t C,
                           int32_t H, int32_t W, int32_t channels, int32_t quality, int64_t slot_bytes, int64_t ws_bytes);
int apd_jpeg_encode(const float* src, int32_t N, int32_t C, int32_t H, int32_t W, int32_t channels, int32_t quality,
                    uint8_t* dst, int64_t slot_bytes, int32_t* sizes, void* ws, int64_t ws_bytes, void* stream);

/* ---- the landmark preview: landmark sets drawn as coloured contours (end2end.py --landmark_video avi, --side_outputs).
 * Added as above: APD_ABI_VERSION stays 1. */

/* vis_landmark (main_end2end_module2.py:47-68) for a batch, and with S == 0 and `bg` the photo marked with its landmarks.
 *   pts       device (N, P, 2) int32 (x, y): the caller has made them integers by the rule of the call site it mirrors
 *             (astype(int32) truncation in vis_landmark, Python round for the marked photo); clamped to +-2^20 here
 *   seg       device (S, 2) int32 landmark indices in draw order; seg_host the same table on the host: every index is checked
 *             against P here, before the launch, and the kernel clamps what it reads from `seg` into [0, P) -- the contract of
 *             apd_landmark_map.  Both, and seg_rgb, may be null when S == 0
 *   seg_rgb   device (S,) uint32, 0x00RRGGBB: one colour per segment
 *   bg        null: the background is the constant bg_rgb.  Else device (bg_frames, 3, H, W) float32 with bg_frames == 1 (one
 *             picture shared by every frame) or N; where nothing is drawn its values pass through bit for bit.  It must not
 *             overlap out (refused)
 *   out       device (N, 3, H, W) float32, planes R, G, B; every element is written exactly once: no memset is needed, no
 *             atomic is used, and the same input gives the same bits
 * Draw order, a later primitive overwriting an earlier one: the background; segments 0 .. S-1, each as
 * cv2.line(p0, p1, colour, thickness) by the rule apd_landmark_map states for op 1 (thickness 1 included); then all P discs
 * cv2.circle(p, radius, disc_rgb, -1).  radius -1 draws no disc.  Primitives are clipped to the frame.
 * A drawn byte v is stored as (2 v + 1) / 255 - 1 (evaluated in double, rounded to float32 once): the middle of v's bucket under
 * apd_frames_to_u8's (uint8)((x + 1) / 2 * 255), which therefore returns v for every v in 0..255 -- the PNG and JPEG encoders and
 * tensor2im all see exactly the colour bytes.
 * One launch on `stream`.  Served: N 1..65535, P 1..APD_MAX_POINTS, S 0..APD_MAX_SEGMENTS, H, W 1..APD_MAX_MAP, radius
 * -1..APD_MAX_RADIUS, thickness 1..APD_MAX_THICKNESS.  apd_landmark_vis_ok needs no device and checks everything but the device
 * pointers' contents. */
int32_t apd_landmark_vis_ok(const int32_t* pts, const int32_t* seg, const int32_t* seg_host, const uint32_t* seg_rgb,
                            const float* bg, int32_t bg_frames, int32_t N, int32_t P, int32_t S, int32_t H, int32_t W,
                            int32_t radius, int32_t thickness, uint32_t disc_rgb, uint32_t bg_rgb, const float* out);
int apd_landmark_vis(const int32_t* pts, const int32_t* seg, const int32_t* seg_host, const uint32_t* seg_rgb,
                     const float* bg, int32_t bg_frames, int32_t N, int32_t P, int32_t S, int32_t H, int32_t W,
                     int32_t radius, int32_t thickness, uint32_t disc_rgb, uint32_t bg_rgb, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
