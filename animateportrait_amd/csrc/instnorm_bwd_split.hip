// instnorm_bwd_split.hip -- ap_instnorm_bwd_split: the InstanceNorm backward that writes the operands of the bf16 matrix
// kernels (the split copy of the data-gradient convolution, the M-role operand and the strip of the weight gradient) itself.
#include "bwd_stream.h"
#include <cstring>
#include <type_traits>

namespace apamd {

// ---- instnorm_bwd_split: the InstanceNorm backward of a layer whose gradient goes straight into the bf16 matrix kernels.
// The fp32 gradient dy of such a layer was written once (4 B / element) and read twice -- by the split pass in front of the
// data-gradient convolution and by the transposition in front of the weight gradient -- to be rounded to bf16 head (+ tail)
// planes both times.  Here a workgroup owns the EIGHT channels of a channel octet of one image (a thread: 4 consecutive pixels
// of each), so after the plane reductions it holds whole slots of both operand layouts and writes them itself:
//   xs  [n][part][C / 8][HW + 1][8 channels]      the split copy conv_bf16x3 stages (conv_bf16x3.h), zero slot included;
//   gt  [n][part][GHp * GX8][Mp][8 pixels]        the M-role operand of wgrad_bf16x3 (wgrad_bf16x3.h): a lane pair holds the two
//                                                 quads of a pixel octet and swaps channel halves (8 shuffles per part);
//   strip [n][c][2][H]  fp32                      columns W - 2, W - 1 transposed: the operand of ops.conv2d_dgrad_strip.
// dy itself is written only on request.  2 reads + (1/2 + 1/2 | 1 + 1) writes per element instead of 4 + (2 | 3).
// grid: min(N * C / 8, resident workgroups), persistent; NT threads >= H * W / 4; needs W % 8 == 0, H >= 3.
struct InBwdSplitParams {
    const float* g1;
    const float* g2;
    const float* y;
    const float* mean;
    const float* rstd;
    int p1, act, N, C, H, W;
    uint4* xs;
    uint4* gt;
    int GHp, GX8, Mp;
    float* strip;
    float* dy;
    int heads_only;
};

__device__ __forceinline__ float bf16_tail(float v) { return v - (float)(__bf16)v; }

// YB16: y holds bf16 values (the raw output ap_conv2d_fwd_bf16out stored); G16: g1 holds bf16 values (a data gradient stored by
// ap_conv2d_fwd_view_bf16out) -- same element offsets, 2-byte elements
// FOLD: g1 is the gradient of a reflection-padded (pad 1) layer, still in padded coordinates (p.p1 == 1)
template <int NT, bool YB16 = false, bool G16 = false, bool FOLD = false>
__global__ __launch_bounds__(NT) void instnorm_bwd_split_kernel(const InBwdSplitParams p) {
    constexpr int NW = NT / 64;
    __shared__ float red[16][NW];
    __shared__ float tot[16];
    const int tid0 = threadIdx.x;
    const int H = p.H, W = p.W, HW = H * W, W4 = W >> 2;
    const bool live = tid0 < HW / 4;
    const int CG = p.C >> 3, items = p.N * CG;
    // A workgroup holds one (image, channel octet) in registers -- a CU has room for one such workgroup -- so it walks several of
    // them: the loads of the next item are issued right behind the stores of the current one (which are not waited for), so reads
    // and writes of a CU overlap and there is no drain + dispatch gap between items (first version, one item per workgroup:
    // 2.7 TB/s, profiles/r04x_train_bf16_bygrid.md; an explicit prefetch in front of the stores spilled 150-300 registers).
    // Also tried: the slots staged through LDS so that every store instruction writes whole lines (as norm_split_kernel does for
    // its 64-byte lane stride) -- 84.6 -> 95.2 us per launch (gpurun_out/r04ag_call.log): with ONE workgroup per CU the two extra
    // barriers and 130 KB of LDS traffic cost more than the four-piece line writes, which the L2 merges anyway.
    for (int item = blockIdx.x; item < items; item += (int)gridDim.x) {
    const int n = item / CG, cg = item - n * CG, c0 = cg * 8;
    // (per-lane addresses are recomputed in every iteration from an opaque copy of the lane id: hoisted out of the loop they
    // occupied registers across it)
    int tid = tid0;
    asm volatile("" : "+v"(tid));
    const int row = tid / W4, x4 = (tid - row * W4) * 4;
    float xh[32], gv[32];
    float rvl;                   // lane c (< 8) holds rstd of channel c0 + c
    {
        // ---- load phase (round 6): NOTHING but loads -- raw words into registers, addresses clamped instead of branched on, the
        // fold's border terms taken from a 6-element window of the padded row (its two outer elements ARE the reflected columns of
        // the first / last group) and, in the two waves that hold rows 1 and H - 2, from a second window of padded row 0 / H + 1.
        // Before, every channel's loads were followed by their conversion (bf16 -> fp32 shifts) or sat in the arms of the
        // run-time `fold1` branch, and the compiler waited for each channel before it asked for the next: 16 serial memory round
        // trips per item plus one per border term, 2.8-3.9 TB/s (profiles/r06_stream_readers.md).
        typedef unsigned u32x3 __attribute__((ext_vector_type(3), aligned(4)));
        typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
        using YRaw = std::conditional_t<YB16, u32x2, float4>;
        using GRaw = std::conditional_t<G16, std::conditional_t<FOLD, u32x3, u32x2>, std::conditional_t<FOLD, float4u, float4>>;
        const int ltid = live ? tid : 0;
        const int lrow = ltid / W4, lx4 = (ltid - lrow * W4) * 4;
        const long long nc0 = (long long)n * p.C + c0;
        const int PW = W + 2, PHW = (H + 2) * PW;
        // lanes of rows 1 / H - 2 fold padded row 0 / H + 1 in; everybody else reads its own row again (a cache hit), masked out later
        const bool brow = FOLD && (lrow == 1 || lrow == H - 2);
        const bool wave_brow = FOLD && __builtin_amdgcn_readfirstlane((int)(__ballot(brow && live) != 0ull));
        const int prow = lrow == 1 ? 0 : (lrow == H - 2 ? H + 1 : lrow + 1);
        const int ecol = lx4 == 0 ? 0 : (lx4 == W - 4 ? W + 1 : lx4 + 1);          // fp32 fold: the reflected column of the group, if any
        YRaw yr[8];
        GRaw gr[8], br[8];
        float ge[8], be[8];
        const float mvl = p.mean[nc0 + (tid & 7)];
        rvl = p.rstd[nc0 + (tid & 7)];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            if constexpr (YB16) yr[c] = reinterpret_cast<const u32x2*>(reinterpret_cast<const unsigned short*>(p.y) + (nc0 + c) * HW)[ltid];
            else yr[c] = reinterpret_cast<const float4*>(p.y + (nc0 + c) * HW)[ltid];
        }
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            if constexpr (G16 && FOLD) {
                gr[c] = *reinterpret_cast<const u32x3*>(reinterpret_cast<const unsigned short*>(p.g1) + (nc0 + c) * PHW + (lrow + 1) * PW + lx4);
            } else if constexpr (G16) {
                gr[c] = reinterpret_cast<const u32x2*>(reinterpret_cast<const unsigned short*>(p.g1) + (nc0 + c) * HW)[ltid];
            } else if constexpr (FOLD) {
                const float* rp = p.g1 + (nc0 + c) * PHW + (lrow + 1) * PW;
                gr[c] = *reinterpret_cast<const float4u*>(rp + lx4 + 1);
                ge[c] = rp[ecol];
            } else {
                gr[c] = reinterpret_cast<const float4*>(p.g1 + (nc0 + c) * HW)[ltid];
            }
        }
        constexpr bool BR_EARLY = false;      // (with the border windows in the first phase the bf16 form spilled 11 registers between its loads: a second phase for the two waves that hold rows 1 and H - 2)
        auto load_border = [&]() __attribute__((always_inline)) {
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                if constexpr (!FOLD) {
                } else if constexpr (G16) {
                    br[c] = *reinterpret_cast<const u32x3*>(reinterpret_cast<const unsigned short*>(p.g1) + (nc0 + c) * PHW + prow * PW + lx4);
                } else {
                    const float* rp = p.g1 + (nc0 + c) * PHW + prow * PW;
                    br[c] = *reinterpret_cast<const float4u*>(rp + lx4 + 1);
                    be[c] = rp[ecol];
                }
            }
        };
        if constexpr (BR_EARLY) {
            if (wave_brow) load_border();
        }
        // ---- conversion and arithmetic
        const bool first = lx4 == 0, last = lx4 == W - 4;
        auto window = [&](const GRaw& w, float e) -> float4 {          // the folded group of a padded row from its raw words
            float4 v;
            if constexpr (G16) {
                const float e0 = __uint_as_float(w[0] << 16), e5 = __uint_as_float(w[2] & 0xffff0000u);
                v = make_float4(__uint_as_float(w[0] & 0xffff0000u), __uint_as_float(w[1] << 16), __uint_as_float(w[1] & 0xffff0000u),
                                __uint_as_float(w[2] << 16));
                v.y += first ? e0 : 0.f;
                v.z += last ? e5 : 0.f;
            } else {
                v = make_float4(w[0], w[1], w[2], w[3]);
                v.y += first ? e : 0.f;
                v.z += last ? e : 0.f;
            }
            return v;
        };
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const float m = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mvl), c)), r = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rvl), c));
            float4 yv, gq;
            if constexpr (YB16) yv = make_float4(__uint_as_float(yr[c][0] << 16), __uint_as_float(yr[c][0] & 0xffff0000u),
                                                 __uint_as_float(yr[c][1] << 16), __uint_as_float(yr[c][1] & 0xffff0000u));
            else yv = yr[c];
            if constexpr (FOLD) {
                gq = window(gr[c], G16 ? 0.f : ge[c]);
                if constexpr (BR_EARLY) {
                    if (wave_brow) {
                        const float4 t = window(br[c], 0.f);
                        gq.x += brow ? t.x : 0.f; gq.y += brow ? t.y : 0.f; gq.z += brow ? t.z : 0.f; gq.w += brow ? t.w : 0.f;
                    }
                }
            } else if constexpr (G16) {
                gq = make_float4(__uint_as_float(gr[c][0] << 16), __uint_as_float(gr[c][0] & 0xffff0000u),
                                 __uint_as_float(gr[c][1] << 16), __uint_as_float(gr[c][1] & 0xffff0000u));
            } else {
                gq = gr[c];
            }
            const float yy[4] = {yv.x, yv.y, yv.z, yv.w}, gg[4] = {gq.x, gq.y, gq.z, gq.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float x = live ? (yy[j] - m) * r : 0.f;
                xh[c * 4 + j] = x;
                gv[c * 4 + j] = live ? gg[j] * act_grad_from_xhat(x, p.act) : 0.f;
            }
        }
        // ---- second phases (their own round trip, taken by few launches / few waves): the border rows where they did not fit the
        // first phase, and a second gradient contribution
        if constexpr (FOLD && !BR_EARLY) {
            if (wave_brow) {
                load_border();
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const float4 t = window(br[c], G16 ? 0.f : be[c]);
                    const float tt[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
                    for (int j = 0; j < 4; ++j) gv[c * 4 + j] += (brow && live) ? tt[j] * act_grad_from_xhat(xh[c * 4 + j], p.act) : 0.f;
                }
            }
        }
        if (p.g2 != nullptr) {
            float4 g2r[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) g2r[c] = reinterpret_cast<const float4*>(p.g2 + (nc0 + c) * HW)[ltid];
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const float tt[4] = {g2r[c].x, g2r[c].y, g2r[c].z, g2r[c].w};
#pragma unroll
                for (int j = 0; j < 4; ++j) gv[c * 4 + j] += live ? tt[j] * act_grad_from_xhat(xh[c * 4 + j], p.act) : 0.f;
            }
        }
    }
    // plane sums of g and g * xhat, per channel: wave butterflies, then a fixed-order sum over the waves
    {
        float s[16];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            s[c] = (gv[c * 4] + gv[c * 4 + 1]) + (gv[c * 4 + 2] + gv[c * 4 + 3]);
            s[8 + c] = (gv[c * 4] * xh[c * 4] + gv[c * 4 + 1] * xh[c * 4 + 1]) + (gv[c * 4 + 2] * xh[c * 4 + 2] + gv[c * 4 + 3] * xh[c * 4 + 3]);
        }
        // 16 values per lane -> wave totals by halving (common.h: wave_sums_to_lds): at lane bits 32, 16, 8, 4 a lane keeps one half
        // of its values and receives the partner's sums of that half, then two plain steps: 17 exchanges instead of 96
        const int lane = tid & 63;
        int cnt = 16;
#pragma unroll
        for (int bit = 32; bit >= 4; bit >>= 1) {
            const int hcnt = cnt >> 1;
            const bool up = (lane & bit) != 0;
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < hcnt) {
                    const float keep = up ? s[hcnt + j] : s[j], give = up ? s[j] : s[hcnt + j];
                    s[j] = keep + __shfl_xor(give, bit, 64);
                }
            cnt = hcnt;
        }
        s[0] += __shfl_xor(s[0], 2, 64);
        s[0] += __shfl_xor(s[0], 1, 64);
        if ((lane & 3) == 0) red[((lane >> 5) & 1) * 8 + ((lane >> 4) & 1) * 4 + ((lane >> 3) & 1) * 2 + ((lane >> 2) & 1)][tid >> 6] = s[0];
        __syncthreads();
        if (tid < 16) {
            float t = 0.f;
#pragma unroll
            for (int w = 0; w < NW; ++w) t += red[tid][w];
            tot[tid] = t * (1.f / (float)HW);
        }
        __syncthreads();
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const float r = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rvl), c)), a1 = tot[c], a2 = tot[8 + c];
#pragma unroll
        for (int j = 0; j < 4; ++j) gv[c * 4 + j] = r * (gv[c * 4 + j] - a1 - xh[c * 4 + j] * a2);
    }
    const int nparts = p.heads_only ? 1 : 2;
    if (p.dy != nullptr && live) {
#pragma unroll
        for (int c = 0; c < 8; ++c)
            reinterpret_cast<float4*>(p.dy + ((long long)n * p.C + c0 + c) * HW)[tid] =
                make_float4(gv[c * 4], gv[c * 4 + 1], gv[c * 4 + 2], gv[c * 4 + 3]);
    }
    if (p.strip != nullptr && live && x4 == W - 4) {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            float* d = p.strip + (((long long)n * p.C + c0 + c) * 2) * H + row;
            d[0] = gv[c * 4 + 2];
            d[H] = gv[c * 4 + 3];
        }
    }
    if (p.xs != nullptr) {
        const int CG = p.C >> 3;
        for (int part = 0; part < nparts; ++part) {
            uint4* plane = p.xs + ((long long)(n * 2 + part) * CG + cg) * (HW + 1);
            if (live) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float v[8];
#pragma unroll
                    for (int c = 0; c < 8; ++c) v[c] = part ? bf16_tail(gv[c * 4 + j]) : gv[c * 4 + j];
                    plane[tid * 4 + j] = make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]),
                                                    pack_bf16x2(v[6], v[7]));
                }
            }
            if (tid == 0) plane[HW] = make_uint4(0u, 0u, 0u, 0u);
        }
    }
    if (p.gt != nullptr) {
        const bool odd = tid & 1;                  // the high quad of the pixel octet (W % 8 == 0: the pair shares a row)
        const long long noct = (long long)p.GHp * p.GX8;
        const long long oct = (long long)row * p.GX8 + (x4 >> 3);
        for (int part = 0; part < nparts; ++part) {
            unsigned lo[8], hi[8];                 // per channel: pixels (0, 1), (2, 3) of this lane's quad
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                float v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = part ? bf16_tail(gv[c * 4 + j]) : gv[c * 4 + j];
                lo[c] = pack_bf16x2(v[0], v[1]);
                hi[c] = pack_bf16x2(v[2], v[3]);
            }
            uint4* dst = p.gt + ((long long)(n * 2 + part) * noct + oct) * p.Mp + c0 + (odd ? 4 : 0);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                // the even lane keeps channels 0..3 and gives 4..7, the odd lane the other way round
                const unsigned give_lo = odd ? lo[k] : lo[4 + k], give_hi = odd ? hi[k] : hi[4 + k];
                const unsigned keep_lo = odd ? lo[4 + k] : lo[k], keep_hi = odd ? hi[4 + k] : hi[k];
                const unsigned got_lo = (unsigned)__shfl_xor((int)give_lo, 1, 64), got_hi = (unsigned)__shfl_xor((int)give_hi, 1, 64);
                if (live) dst[k] = odd ? make_uint4(got_lo, got_hi, keep_lo, keep_hi) : make_uint4(keep_lo, keep_hi, got_lo, got_hi);
            }
        }
    }
    }
}

}  // namespace apamd

using namespace apamd;

extern "C" {

int ap_instnorm_bwd_split_ok(int32_t C, int32_t H, int32_t W, int32_t g1_pad) {
    // H >= 4 for the fold: the kernel adds padded row 0 into row 1 and padded row H + 1 into row H - 2 in the lanes of those rows,
    // one border row per lane -- with H = 3 both land in row 1 and the second would be dropped
    return !sw(SW_NO_INBWD_SPLIT) && C >= 8 && C % 8 == 0 && H >= 3 + g1_pad && W >= 8 && W % 8 == 0 && H <= 4096 && W <= 4096 &&
           H * W <= 4096 && (g1_pad == 0 || g1_pad == 1) ? 1 : 0;
}

int ap_instnorm_bwd_split(const float* g1, int32_t g1_pad, const float* g2, const float* y, const float* mean, const float* rstd,
                          int32_t act, int32_t N, int32_t C, int32_t H, int32_t W, void* xs, void* gt, const int32_t* gt_dims,
                          float* strip, float* dy, int32_t heads_only, ap_stream_t stream) {
    int rc = fold_args_ok(g1, g1_pad, H, W, "instnorm_bwd_split");
    if (rc) return rc;
    if (!y || !mean || !rstd) return fail(AP_ERR_INVALID, "instnorm_bwd_split: null pointer");
    if (!xs && !gt && !dy) return fail(AP_ERR_INVALID, "instnorm_bwd_split: no output requested");
    if (act < 0 || act > 2) return fail(AP_ERR_INVALID, "instnorm_bwd_split: act %d", act);
    if (!ap_instnorm_bwd_split_ok(C, H, W, g1_pad))
        return fail(AP_ERR_UNSUPPORTED, "instnorm_bwd_split: C=%d %dx%d fold %d (needs C %% 8 == 0, W %% 8 == 0, H >= 3 + fold, H*W <= 4096)", C, H, W, g1_pad);
    if (N < 1 || N > 65535) return fail(AP_ERR_UNSUPPORTED, "instnorm_bwd_split: N=%d", N);
    InBwdSplitParams p;
    memset(&p, 0, sizeof(p));
    p.g1 = g1; p.g2 = g2; p.y = y; p.mean = mean; p.rstd = rstd;
    p.p1 = g1_pad; p.act = act; p.C = C; p.H = H; p.W = W;
    p.xs = reinterpret_cast<uint4*>(xs);
    p.gt = reinterpret_cast<uint4*>(gt);
    if (gt) {
        if (!gt_dims) return fail(AP_ERR_INVALID, "instnorm_bwd_split: gt without its dimensions");
        p.GHp = gt_dims[0]; p.GX8 = gt_dims[1]; p.Mp = gt_dims[2];
        if (p.GHp < H || p.GX8 * 8 < W || p.Mp < C)
            return fail(AP_ERR_INVALID, "instnorm_bwd_split: operand %d x %d x %d smaller than the gradient", p.GHp, p.GX8, p.Mp);
    }
    // heads_only: bit 0 = only head planes are written; bit 1 = y holds bf16 values; bit 2 = g1 holds bf16 values
    p.strip = strip; p.dy = dy; p.heads_only = (heads_only & 1) ? 1 : 0;
    const bool yb16 = (heads_only & 2) != 0, g16 = (heads_only & 4) != 0;
    p.N = N;
    const int items = N * (C / 8);
    const bool small = H * W / 4 <= 256;
    const int slots = num_cus() * (small ? 4 : 1);          // resident workgroups: registers hold one 1024-thread item per CU, four of 256
    const dim3 grid(items < slots ? items : slots);
    auto launch = [&](auto nt) {
        constexpr int NTH = decltype(nt)::value;
        auto go = [&](auto yt, auto gt_, auto ft) {
            hipLaunchKernelGGL((instnorm_bwd_split_kernel<NTH, decltype(yt)::value, decltype(gt_)::value, decltype(ft)::value>), grid, dim3(NTH), 0,
                               (hipStream_t)stream, p);
        };
        using T = std::true_type;
        using F = std::false_type;
        const int sel = (yb16 ? 4 : 0) | (g16 ? 2 : 0) | (g1_pad == 1 ? 1 : 0);
        switch (sel) {
            case 0: go(F{}, F{}, F{}); break;
            case 1: go(F{}, F{}, T{}); break;
            case 2: go(F{}, T{}, F{}); break;
            case 3: go(F{}, T{}, T{}); break;
            case 4: go(T{}, F{}, F{}); break;
            case 5: go(T{}, F{}, T{}); break;
            case 6: go(T{}, T{}, F{}); break;
            default: go(T{}, T{}, T{}); break;
        }
    };
    if (small) launch(std::integral_constant<int, 256>{});
    else launch(std::integral_constant<int, 1024>{});
    return check_launch("instnorm_bwd_split_kernel");
}

}  // extern "C"
