// conv_plan.h -- the plan of one convolution layer, shared by the host files of the forward side (internal).
//
// A descriptor (ap_conv_desc) is turned into one launch (Conv2d) or four launches (ConvTranspose2d stride 2 as sub-pixel phases);
// the same plan drives the weight packer and the launchers, so that the packed image and the kernel always agree.  Who relies on
// which fields:
//   packer    (conv_pack.hip)  the family flags small / direct_cop / bf3, k (CI, CO_TILE, wfloats) or bk (CO_TILE), Cin, nchunks,
//                              chunk_begin, co_tiles, head_w_off, packed_floats, and of every launch its taps' (ky, kx) and wp_off
//   launchers (conv_fwd.hip)   all of the above but packed_floats, and the rest: tsmall / head / fused_phases / ph4 / k0_small,
//                              cin_pad, Hout / Wout, stat_tiles, and of every launch its taps' (ly, lx), output grid (OH, OW, os*,
//                              o*_off), origin (dy0, dx0), tile grid and stat_tile_off
// Only make_plan (conv_plan.hip) writes a Plan; Geom and the plan_* / pick_* steps are private to that file.
#pragma once
#include "common.h"
// the kernel descriptors a Plan points to (ConvKernelInfo, Bf3Kernel); kMaxSeg, kMaxTaps and ConvKParams come with them
#include "conv_registry.h"
#include "conv_bf3_registry.h"

#include <vector>

namespace apamd {

struct Tap { int ky, kx, ly, lx; };  // (ky,kx): index into the caller's weight; (ly,lx): LDS tile offset

struct Launch {
    std::vector<Tap> taps;
    int OH, OW, dy0, dx0;
    int osy, osx, oy_off, ox_off;
    int tiles_x, tiles_y;
    long long wp_off;      // float offset of this launch's weights in the packed buffer
    int stat_tile_off;
};

struct Plan {
    const ConvKernelInfo* k = nullptr;
    int direct_cop = 0;            // > 0: conv_direct_f32<K, direct_cop> instead of the implicit-GEMM kernel
    bool small = false;            // conv_small_f32: narrow 3x3 layers on the vector ALUs
    bool head = false;             // conv_head_fwd_kernel: one output channel, 4x4, narrow map
    bool tsmall = false;           // conv_tsmall_f32: transposed 4x4 stride 2 with 1..4 output channels
    long long head_w_off = -1;     // >= 0: plain copy of the caller's weights at this offset of the packed image
    bool bf3 = false;              // split-bf16 matrix path
    bool fused_phases = false;     // transposed, split-bf16: the four sub-pixel phases are one launch
    int ph4 = 0;                   // 3 / 4: ... and one TILE (conv_ph4.h)
    bool k0_small = false;         // run-time-tap family: the half-height 4-tap instantiation (two workgroups per CU)
    const Bf3Kernel* bk = nullptr;
    std::vector<Launch> launches;
    int Cin = 0, nchunks = 0, cin_pad = 0, co_tiles = 0;
    int chunk_begin[kMaxSeg] = {0, 0, 0};
    int Hout = 0, Wout = 0, stat_tiles = 0;
    long long packed_floats = 0;
};

int make_plan(const ap_conv_desc* d, Plan& pl);
// the tables make_plan picks from (ap_conv2d_fwd_route_names lists them; ph4_kernel: conv_bf3_registry.h)
const std::vector<ConvKernelInfo>& registry();
const std::vector<Bf3Kernel>& bf3_registry();
// the kernel of one launch: K == 0 kernels are instantiated per tap count
const Bf3Kernel* bf3_for_taps(const Bf3Kernel* k, int ntaps);
// which plans take the channel-octet / the bf16-output form (ap_conv2d_octet_ok, ap_conv2d_bf16out_ok; the launchers refuse the rest)
bool octet_plan_ok(const ap_conv_desc* d, const Plan& pl);
bool ob16_plan_ok(const ap_conv_desc* d, const Plan& pl);

}  // namespace apamd
