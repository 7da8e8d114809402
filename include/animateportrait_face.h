/*
 * animateportrait_face.h -- C ABI of libapface.so: the MTCNN face detector of the reference's end-to-end driver
 * (MTCNN/detector.py, first_stage.py, box_utils.py, get_nets.py; align_mtcnn in main_end2end_module2.py:12-45) on the
 * MI355X (gfx950): image pyramid, P-Net, box arithmetic, padded cut-outs, R-Net, O-Net and the aligned 512 x 512 picture.
 *
 * Like libapdata.so and libapstyle.so this library is NOT part of the model boundary (include/animateportrait_amd.h).
 *
 * Conventions: as in animateportrait_amd.h -- device pointers, caller-owned buffers and workspaces, calls only enqueue on
 * `stream` (a hipStream_t as void*), 0 = ok, negative = error with a thread-local message (apf_last_error()).  A refused
 * call launches nothing and writes nothing; every *_ok function needs no device.  Images are interleaved 8-bit RGB
 * (H, W, 3).  Box arrays are float64 rows (x1, y1, x2, y2, score) as in the reference; every count is an int32 in device
 * memory, so that a whole detection is enqueued without a read-back.
 *
 * Capacities are fixed per image and stage.  A stage that meets more boxes than its output holds keeps the first
 * `capacity` of them in the order defined below, sets its bit in the caller's status word and never writes past a buffer:
 *   APF_CAP_LEVEL    candidates of one pyramid level above the P-Net threshold
 *   APF_CAP_MERGED   boxes of all levels after the per-level NMS
 *   APF_CAP_RNET     boxes after the first NMS (R-Net's batch)
 *   APF_CAP_ONET     boxes after the second NMS (O-Net's batch, and the final result)
 */
#ifndef ANIMATEPORTRAIT_FACE_H
#define ANIMATEPORTRAIT_FACE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define APF_ABI_VERSION 1

enum { APF_OK = 0, APF_ERR_INVALID = -1, APF_ERR_UNSUPPORTED = -2, APF_ERR_LAUNCH = -3 };

#define APF_MAX_SIDE 8192      /* height / width of a photo, a level or a cut */
#define APF_MIN_LEVEL 12       /* P-Net's receptive field */
#define APF_CAP_LEVEL 4096
#define APF_CAP_MERGED 4096
#define APF_CAP_RNET 2048
#define APF_CAP_ONET 512
#define APF_CAP_SORT 4096      /* most boxes one NMS sorts: apf_box_stage's cap_in */

/* bits of the status word */
#define APF_OVF_LEVEL 1
#define APF_OVF_MERGED 2
#define APF_OVF_STAGE 4        /* apf_box_stage: more picks than cap_out */

/* packed fp32 parameters of a net, in named_parameters() order; conv weights (O, I, k, k), PReLU slopes [C].  The first
 * fully connected layer's weight is stored (in, out) with `in` running over (c, h, w): the reference's Flatten (which
 * transposes h and w) is folded into it.  The heads' weights are (out, in). */
#define APF_PNET_PARAMS 6632
#define APF_RNET_PARAMS 100178
#define APF_ONET_PARAMS 389040

enum { APF_NMS_UNION = 0, APF_NMS_MIN = 1 };
enum { APF_NET_R = 0, APF_NET_O = 1 };

int32_t apf_abi_version(void);
const char* apf_last_error(void);

/* Image.resize((ow, oh), BILINEAR) of the whole image, bit-exact against Pillow's 8-bit resampler (both passes, the uint8
 * intermediate included).  out (oh, ow, 3) uint8. */
int32_t apf_resize_level_ok(const uint8_t* img, int32_t H, int32_t W, int32_t oh, int32_t ow, const uint8_t* out);
int apf_resize_level(const uint8_t* img, int32_t H, int32_t W, int32_t oh, int32_t ow, uint8_t* out, void* stream);

/* P-Net over one level (h, w, 3) uint8, (v - 127.5) / 128 applied on load.  Output map (mh, mw) = (ceil((h-2)/2) - 4,
 * ceil((w-2)/2) - 4).  prob (mh, mw) and off (4, mh, mw): the face probability and the offsets, either may be null.
 * Positions with prob > threshold are appended (in no fixed order) to the candidate arrays while *cand_count <
 * APF_CAP_LEVEL; *cand_count goes on counting.  The caller zeroes *cand_count.
 *   cand_idx [cap] row-major index, cand_score [cap], cand_off [cap * 4] */
int32_t apf_pnet_ok(const uint8_t* level, int32_t h, int32_t w, const float* params, const int32_t* cand_count);
int apf_pnet(const uint8_t* level, int32_t h, int32_t w, const float* params, float threshold, float* prob, float* off,
             int32_t* cand_idx, float* cand_score, float* cand_off, int32_t* cand_count, void* stream);

/* One level's candidates -> boxes (_generate_bboxes: row-major order, np.round half to even) -> NMS (union, nms_threshold)
 * -> appended to merged (APF_CAP_MERGED, 9) float64 = box, score, 4 offsets, in pick order, at *merged_count.
 * cand_boxes (APF_CAP_LEVEL, 9) workspace holds the level's candidates in row-major order afterwards; mw: width of the map.
 * One workgroup. */
int32_t apf_stage1_level_ok(const int32_t* cand_idx, const int32_t* cand_count, int32_t mw, double scale,
                            const double* cand_boxes, const double* merged, const int32_t* merged_count);
int apf_stage1_level(const int32_t* cand_idx, const float* cand_score, const float* cand_off, const int32_t* cand_count,
                     int32_t mw, double scale, double nms_threshold, double* cand_boxes, int32_t* level_count,
                     double* merged, int32_t* merged_count, int32_t* status, void* stream);

/* The box arithmetic of one stage, in float64 and numpy's operation order, one workgroup:
 *   filter   probs (n, 2) not null: keep rows with probs[:, 1] > score_threshold, in order; their score becomes that prob
 *   offsets  (n, 4) fp32, or null: columns 5..8 of `in` (in_stride 9)
 *   late == 0 (stages 1 and 2): NMS -> gather picks -> calibrate -> square -> np.round; the squared boxes' score is 0 as
 *             in the reference.  cal / sq (cap_out, 5), either may be null, keep the steps.
 *   late == 1 (stage 3): landmarks (n, 10) placed in the box (stored fp32), calibrate, NMS, gather; cal keeps the
 *             calibrated boxes before the NMS (n rows, so cap_in rows)
 * NMS: sort by (score, index) ascending, sweep from the top; a pick suppresses lower-ranked boxes whose overlap exceeds
 * nms_threshold.  picks [cap_in] are indices into the filtered list, in pick order.  *n_in <= cap_in <= APF_CAP_SORT.
 * ws: apf_box_stage_ws_bytes(cap_in) bytes. */
int64_t apf_box_stage_ws_bytes(int32_t cap_in);
int32_t apf_box_stage_ok(const double* in, int32_t in_stride, const int32_t* n_in, int32_t cap_in, int32_t mode, int32_t late,
                         const float* landmarks, const double* out, const int32_t* n_out, int32_t cap_out, const void* ws);
int apf_box_stage(const double* in, int32_t in_stride, const int32_t* n_in, int32_t cap_in, const float* probs,
                  const float* offsets, const float* landmarks, double score_threshold, double nms_threshold, int32_t mode,
                  int32_t late, double* out, float* out_landmarks, int32_t* n_out, int32_t cap_out, int32_t* picks,
                  double* cal, double* sq, int32_t* status, void* ws, void* stream);

/* get_image_boxes: for each of *count boxes (cap rows, stride 5) its window of the image, zero outside it, resized to
 * size x size (24 or 48) with Pillow's BILINEAR, bit-exact; coefficients are computed per box on the device, tap by tap.
 * out (cap, size, size, 3) uint8.  Then the boxes are clipped to the image in place, as correct_bboxes leaves them. */
int32_t apf_cutouts_ok(const uint8_t* img, int32_t H, int32_t W, const double* boxes, const int32_t* count, int32_t cap,
                       int32_t size, const uint8_t* out);
int apf_cutouts(const uint8_t* img, int32_t H, int32_t W, double* boxes, const int32_t* count, int32_t cap, int32_t size,
                uint8_t* out, void* stream);

/* R-Net (net == APF_NET_R, cuts of 24) or O-Net (APF_NET_O, cuts of 48) over *count cut-outs (cap, size, size, 3) uint8.
 * probs (cap, 2) after softmax, offsets (cap, 4), landmarks (cap, 10) (O-Net only, null for R-Net).
 * ws: apf_net_ws_bytes(net, cap) bytes.  fp32 FMA throughout. */
int64_t apf_net_ws_bytes(int32_t net, int32_t cap);
int32_t apf_net_ok(int32_t net, const uint8_t* cuts, const int32_t* count, int32_t cap, const float* params, const void* ws,
                   const float* probs, const float* offsets, const float* landmarks);
int apf_net(int32_t net, const uint8_t* cuts, const int32_t* count, int32_t cap, const float* params, void* ws, float* probs,
            float* offsets, float* landmarks, void* stream);

/* The size x size cut at (x0, y0) of the image, `fill` where it leaves it, resized to (out_size, out_size) by OpenCV's
 * 8-bit INTER_CUBIC rule: a = -0.75, replicated border, 11-bit coefficients, one rounded >> 22 after both passes.
 * out (out_size, out_size, 3) uint8, RGB like the input. */
int32_t apf_crop_resize_cubic_ok(const uint8_t* img, int32_t H, int32_t W, int32_t x0, int32_t y0, int32_t size,
                                 int32_t out_size, const uint8_t* out);
int apf_crop_resize_cubic(const uint8_t* img, int32_t H, int32_t W, int32_t x0, int32_t y0, int32_t size, int32_t fill,
                          int32_t out_size, uint8_t* out, void* stream);

/* ---- the photo's 68 landmarks: input and output side of the FAN network (fan.py; face_alignment's get_landmarks).
 * A face box d = (x0, y0, x1, y1) fixes, in float64 and this operation order,
 *     cx = x1 - (x1 - x0) / 2     cy = y1 - (y1 - y0) / 2 - (y1 - y0) * 0.12     scale = (x1 - x0 + y1 - y0) / 195
 * and transform(p, S) = the inverse of [[a, 0, bx], [0, a, by], [0, 0, 1]] applied to (px, py, 1), with h = 200 scale, a = S / h,
 * bx = S (0.5 - cx / h), by = S (0.5 - cy / h):  X = (1 / a) px + (-bx / a),  Y = (1 / a) py + (-by / a), nothing fused.
 * Boxes are passed BY VALUE / from HOST memory: the arithmetic that decides a window's size runs in the launcher. */
#define APF_FAN_POINTS 68
#define APF_FAN_MAX_RES 1024    /* R of apf_fan_crop, Hm of apf_fan_decode */
#define APF_FAN_MAX_B 16        /* images of one apf_fan_decode call */
enum { APF_FAN_RGB = 0, APF_FAN_BGR = 1 };

/* The network's input.  ul = trunc(transform((1, 1), R)), br = trunc(transform((R, R), R)); the (br.y - ul.y) x (br.x - ul.x)
 * window holds image pixel (wy + ul.y, wx + ul.x) at (wy, wx) where that lies in the image and zero elsewhere; it is resized to
 * R x R by OpenCV's 8-bit INTER_LINEAR rule (source index floor((d + 0.5) ratio - 0.5) with float weights rounded to 11 bits, a
 * tap left of the window -> (0, weight 0), at or past its last pixel -> (last, weight 0); the vertical pass is
 * (((b0 (S0 >> 4)) >> 16) + ((b1 (S1 >> 4)) >> 16) + 2) >> 2).  out (1 + flip, 3, R, R) fp32 = byte / 255; row 1 (flip == 1) is
 * row 0 mirrored in x.  order APF_FAN_RGB: plane c is the image's channel c; APF_FAN_BGR: plane c is channel 2 - c.
 * A window side outside 1 .. 4 * APF_MAX_SIDE is refused. */
int32_t apf_fan_crop_ok(const uint8_t* img, int32_t H, int32_t W, double x0, double y0, double x1, double y1, int32_t R, int32_t flip,
                        int32_t order, const float* out);
int apf_fan_crop(const uint8_t* img, int32_t H, int32_t W, double x0, double y0, double x1, double y1, int32_t R, int32_t flip,
                 int32_t order, float* out, void* stream);

/* Heat maps -> landmarks.  hm (B, 68, Hm, Hm) fp32; hm_flipped: null, or the maps of the mirrored inputs, and the map that is read
 * is then hm[b, j] + mirror_x(hm_flipped[b, pair[j]]) (fp32, in that order; pair: the 68-point mirror table).  Per (b, j): argmax
 * (lowest flat index on ties), x = idx % Hm + 1, y = idx / Hm + 1; a peak strictly inside the map moves by a quarter pixel
 * towards its larger neighbour on either axis (equal neighbours: not at all); minus 0.5; transform(., Hm) of box b in float64;
 * truncate != 0 truncates toward zero; stored as fp32 in out (B, 68, 2).  boxes: B rows (x0, y0, x1, y1) in HOST memory, read
 * before the call returns.  One workgroup per (b, j); the reduction's order is fixed. */
int32_t apf_fan_decode_ok(const float* hm, const float* hm_flipped, int32_t B, int32_t Hm, const double* boxes, const float* out);
int apf_fan_decode(const float* hm, const float* hm_flipped, int32_t B, int32_t Hm, const double* boxes, int32_t truncate, float* out,
                   void* stream);

#ifdef __cplusplus
}
#endif

#endif
