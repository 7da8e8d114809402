// wgrad_plan.h -- the plan of one layer's weight gradient, shared by the planner (wgrad_plan.hip) and the launchers
// (wgrad_launch.hip, wgrad_operand.hip) of the general family (internal).  The edge layers (wgrad_edge_host.hip) have plans of their own.
//
// The kernel tables take kernel addresses and so instantiate the kernels: they live in wgrad_launch.hip, and the planner reads
// their entries (tile sizes, names) through the accessors below.  Only make_wgrad_plan writes a WgradPlan; the launchers read it.
#pragma once
#include "common.h"
#include "conv_igemm.h"     // kMaxSeg

namespace apamd {

// ------------------------------------------------------------------ kernel table entries
struct WgradKernel {
    int S, K, M_TILE, Q_TILE, PR;
    const void* fn;
    size_t lds_bytes;
};

// split-bf16 instantiations by kernel size (stride 1) and form
enum { BF3_SPLIT, BF3_HEADS, BF3_WIDE };
struct WgradBf3Kernel {
    int K, form;
    const void* fn;
    size_t lds_bytes;
    int threads;
};

// streaming kernels for 1..2 input channels, by (K, S, Cin, ppt); cob = output channels per workgroup
struct WgradNarrowKernel {
    int K, S, Cin, ppt, cob;
    const void* fn;
};

// both operands from the split copies (wgrad_xs.h), by (kernel size the GEMM sees, staged parts, wave rows)
struct WgradXsParams;
struct WgradXsKernel {
    int Kb, parts, wm;
    int (*launch)(const WgradXsParams&, unsigned, hipStream_t);
};

// the tables (wgrad_launch.hip), and the entry of a layer or null
template <class T>
struct KernelTable {
    const T *first, *last;
    const T* begin() const { return first; }
    const T* end() const { return last; }
};
KernelTable<WgradKernel> wgrad_igemm_kernels();
KernelTable<WgradBf3Kernel> wgrad_bf3_kernels();
KernelTable<WgradNarrowKernel> wgrad_narrow_kernels();
KernelTable<WgradXsKernel> wgrad_xs_kernels();
const WgradNarrowKernel* narrow_kernel(int K, int S, int Cin, int ppt);

// ------------------------------------------------------------------ the plan: one family per layer
enum class WgradFamily { Narrow, Bf16Gemm, Igemm };

// streaming kernel for 1..2 input channels (wgrad_narrow.h)
struct NarrowPlan {
    const WgradNarrowKernel* k = nullptr;
    int gwc = 0, gwc_shift = 0, rpi = 0, rows_per_block = 0;
};
// split-bf16 kernel (wgrad_bf16x3.h): operands as [n][part][row][x/8][channel] pixel-octet slots
struct Bf16GemmPlan {
    bool s2d = false;       // the space-to-depth form of a stride-2 layer: a 2 x 2 stride-1 layer over 4 Cin channels
    bool rows = false;      // the row form of a 7x7 stem: a 1 x 7 layer over 7 Cin channels (channel ci * 7 + ky = the input shifted by ky rows)
    bool wide = false;      // the 8-wave workgroup: 128-channel M tiles (split-bf16 arithmetic, K <= 3, M % 128 == 0)
    int Kb = 0, Cb = 0, Hb = 0, Wb = 0;     // kernel size, channels and operand size the kernel sees
    int c_tiles = 0, Mp = 0, Cp = 0, GHp = 0, GX8 = 0, Hp = 0, AX8 = 0;
    int taps = 0;                           // taps per accumulator tile
    long long sum_floats = 0;               // one workgroup's partial sums = what the reduction adds up (accumulator-order tiles)
};
// exact-fp32 implicit GEMM (wgrad_igemm.h)
struct IgemmPlan {
    int q_tiles = 0, GHp = 0, GWp = 0, Hp = 0, Wp = 0;
    bool g_direct = false;
};
struct WgradPlan {
    WgradFamily family = WgradFamily::Igemm;
    int Cin = 0, Q = 0, P = 0;
    int tiles_x = 0, tiles_y = 0, nstages = 0, m_tiles = 0;          // pixel and M tiling of the two GEMM families
    long long a_floats = 0, g_floats = 0, part_floats = 0;           // the workspace
    const WgradKernel* k = nullptr;         // the fp32 kernel of the layer's (stride, K): a layer without one is not served at all
    NarrowPlan narrow;
    Bf16GemmPlan bf;
    IgemmPlan ig;
    bool bf16_gemm() const { return family == WgradFamily::Bf16Gemm; }
};

// the kernel table entry of a bf16 GEMM plan (b16: plain-bf16 arithmetic) / of its route straight from the split copies
const WgradBf3Kernel* bf3_kernel(const Bf16GemmPlan& b, bool b16);
const WgradXsKernel* xs_kernel(const ap_wgrad_desc* d, const Bf16GemmPlan& b);

// ------------------------------------------------------------------ the planner (wgrad_plan.hip)
int make_wgrad_plan(const ap_wgrad_desc* d, WgradPlan& pl);
// the shifted operand re-tiled from the forward pass's split copies / both operands read straight from them
bool wgrad_xs_route(const ap_wgrad_desc* d, const WgradPlan& pl);
bool wgrad_xs_direct_ok(const ap_wgrad_desc* d, const WgradPlan& pl);

// which of the four operand-preparation kernels re-tiles an operand (launch_split_transpose launches it, ap_conv2d_wgrad_route names
// it), or one of the two refusals.  any_b16: a segment holds bf16 values (ap_src.act bit 8); W: the source's width
enum SplitTForm { ST_GENERAL, ST_VEC, ST_PAD_ROWS, ST_S2D_ROWS, ST_NO_ROW_VIEW = -1, ST_B16_NEEDS_PAD_ROWS = -2 };
bool split_transpose_whole_rows(int W, int s2d_c);
int split_transpose_form(int nseg, bool any_b16, int C, int W, int pad, int X8, int Cp, int s2d_c, int rows_k);
int split_transpose_refusal(int form);
bool any_bf16_segment(const ap_src* segs, int nseg);
// the operand passes of the bf16 GEMM (wgrad_operand.hip): an operand from fp32 / bf16 tensors, the shifted operand re-tiled from
// the forward pass's split copies (C = channels of the view), and the shifted operand of a plan by whichever of the two serves it
int launch_split_transpose(const ap_src* segs, int nseg, int N, int C, int H, int W, int pad, int pad_mode, int Hp, int X8, int Cp,
                           uint4* out, hipStream_t stream, int s2d_c, int heads_only, int rows_k = 0);
int launch_xs_transpose(const void* const* xs, const int* seg_c, int nseg, int N, int H, int W, int pad, int pad_mode, int Hp, int X8,
                        int Cp, int parts, uint4* out, hipStream_t stream, int s2d_c = 0, int H0 = 0, int W0 = 0);
int launch_bf16_gemm_operand(const ap_wgrad_desc* d, const WgradPlan& pl, bool from_xs, uint4* at, hipStream_t stream);

}  // namespace apamd
