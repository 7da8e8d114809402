/*
 * animateportrait_style.h -- C ABI of libapstyle.so: the element-wise and statistics kernels of the static cartoon
 * generator (Photo2Cartoon, Module2/models/photo2cartoon.py:166-525) on the MI355X (gfx950).
 *
 * Like libapdata.so this library is NOT part of the model boundary (include/animateportrait_amd.h, libapamd.so): the
 * convolutions of the cartoon generator run through that one, and this one supplies what its U-GAT-IT-style layers need
 * around them -- LIN / adaLIN folded to one affine pair per plane, and the hourglass's joins, pools and up-sampling adds.
 *
 * Conventions: as in animateportrait_amd.h -- device pointers to contiguous fp32 NCHW tensors, caller-owned buffers, calls
 * only enqueue on `stream` (a hipStream_t as void*), 0 = ok, negative = error with a thread-local message
 * (aps_last_error()).  A refused call launches nothing and writes nothing; every *_ok function needs no device.
 */
#ifndef ANIMATEPORTRAIT_STYLE_H
#define ANIMATEPORTRAIT_STYLE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define APS_ABI_VERSION 1

enum { APS_OK = 0, APS_ERR_INVALID = -1, APS_ERR_UNSUPPORTED = -2, APS_ERR_LAUNCH = -3 };

/* served region of every call: planes (N * C) per launch, height / width of a plane, elements of a tensor */
#define APS_MAX_PLANES 65535
#define APS_MAX_SIDE 4096
#define APS_MAX_ELEMS 0x7fffffffLL

enum { APS_ACT_NONE = 0, APS_ACT_RELU = 1 };

int32_t aps_abi_version(void);
const char* aps_last_error(void);

/* LIN / adaLIN (photo2cartoon.py:488-525) folded to y = a[n,c] x + b[n,c]:
 *   a[n,c] = gamma (rho rstd_in + (1 - rho) rstd_ln)
 *   b[n,c] = beta - gamma (rho mean_in rstd_in + (1 - rho) mean_ln rstd_ln)
 * with the per-(n,c) mean and UNBIASED variance over H W, the per-n mean and UNBIASED variance over C H W (torch.var's
 * defaults) and rstd = 1 / sqrt(var + eps).  rho is used as given (no clamp).
 *   x        (N, C, H, W)
 *   rho      [C]
 *   gamma, beta   [C] (per_sample == 0: LIN) or [N * C] (per_sample == 1: adaLIN)
 *   planes   [N * C * 2] workspace: per plane (mean, M2 = sum (x - mean)^2), count H W; two passes over the plane, and
 *            the layer variance is combined from them with the parallel (Chan) formula
 *   a, b     [N * C]
 * H W < 2 is refused: the unbiased variance is undefined there.  Two launches: one workgroup per plane, one per sample. */
int32_t aps_lin_coeffs_ok(const float* x, const float* rho, const float* gamma, const float* beta, const float* planes,
                          const float* a, const float* b, int32_t N, int32_t C, int32_t H, int32_t W, int32_t per_sample);
int aps_lin_coeffs(const float* x, int32_t N, int32_t C, int32_t H, int32_t W, const float* rho, const float* gamma,
                   const float* beta, int32_t per_sample, float eps, float* planes, float* a, float* b, void* stream);

/* y = act(a[n,c] x + b[n,c]) (+ residual);  act: APS_ACT_NONE / APS_ACT_RELU; residual (N, C, H, W) or null.
 * mean_out / rstd_out [N * C], both or neither: the biased InstanceNorm statistics of y (eps 1e-5), for a consumer that
 * normalises y while it loads it.  a may be zero or negative. */
int32_t aps_affine_apply_ok(const float* x, const float* a, const float* b, const float* y, const float* mean_out,
                            const float* rstd_out, int32_t N, int32_t C, int32_t H, int32_t W, int32_t act);
int aps_affine_apply(const float* x, const float* a, const float* b, int32_t act, const float* residual, int32_t N, int32_t C,
                     int32_t H, int32_t W, float* y, float* mean_out, float* rstd_out, void* stream);

/* The hourglass's element-wise producers, one pass over the output each (one workgroup per output plane).
 * (N, C, H, W) is the shape of s0 except for JOIN, where C is the OUTPUT's channel count.
 *   JOIN    y = s0 + cat(s1, s2, s3) over channels, widths C/2, C/4, C/4 (ConvBlock.forward); C % 4 == 0
 *   POOL2   y = avg_pool2d(s0, 2): (N, C, H/2, W/2), an odd last row / column is dropped; H, W >= 2
 *   UP2ADD  y = s1 + nearest_up2(s0): (N, C, 2H, 2W); s1 null: plain up-sampling; a skip that is not (Hs, Ws) = (2H, 2W)
 *           is refused
 *   SUM3    y = s0 + s1 + s2
 *   STAT    no y: mean_out[n,c] = mean of s0 (flags bit 0: of relu(s0)) -- adaptive_avg_pool2d(x, 1); rstd_out null
 * mean_out / rstd_out (other modes): both or neither, the biased InstanceNorm statistics of y (eps 1e-5). */
enum { APS_JOIN = 0, APS_POOL2 = 1, APS_UP2ADD = 2, APS_SUM3 = 3, APS_STAT = 4 };
#define APS_STAT_RELU 1

int32_t aps_plane_combine_ok(int32_t mode, const float* s0, const float* s1, const float* s2, const float* s3, int32_t N,
                             int32_t C, int32_t H, int32_t W, int32_t Hs, int32_t Ws, int32_t flags, const float* y,
                             const float* mean_out, const float* rstd_out);
int aps_plane_combine(int32_t mode, const float* s0, const float* s1, const float* s2, const float* s3, int32_t N, int32_t C,
                      int32_t H, int32_t W, int32_t Hs, int32_t Ws, int32_t flags, float* y, float* mean_out, float* rstd_out,
                      void* stream);

/* Luminance of a 3-channel cartoon frame, the input of the identity loss of cartoon TRAINING
 * (geomgm_ifw_cartoon_fore_model.py:745-748):  y = 0.299 x[:, 0] + 0.587 x[:, 1] + 0.114 x[:, 2], each product rounded and the
 * sum taken left to right in fp32, as the ATen chain does (same bits).
 *   x (N, 3, H, W) -> y (N, 1, H, W);   aps_luma_bwd: g (N, 1, H, W) -> gx (N, 3, H, W), gx[:, c] = k_c g
 * One pass over HBM each.  128-bit loads and stores when H W % 4 == 0 and both pointers are 16-byte aligned (every plane then
 * starts on a 16-byte boundary), element by element otherwise.
 * Added without changing an existing call, so APS_ABI_VERSION stays 1; a binding finds a library that predates them by the
 * missing symbol. */
int32_t aps_luma_ok(const float* in, const float* out, int32_t N, int32_t H, int32_t W);
int aps_luma_fwd(const float* x, int32_t N, int32_t H, int32_t W, float* y, void* stream);
int aps_luma_bwd(const float* g, int32_t N, int32_t H, int32_t W, float* gx, void* stream);

#ifdef __cplusplus
}
#endif

#endif
