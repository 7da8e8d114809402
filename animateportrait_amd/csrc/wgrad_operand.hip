// wgrad_operand.hip -- the operand passes of the bf16 weight-gradient GEMM: the kernels of wgrad_operand.h (this is the one
// translation unit that includes them) and their launchers, declared in wgrad_plan.h and called by the family launcher
// (wgrad_launch.hip: launch_bf16_gemm).  The igemm family's operand pass (launch_pad) stays with its kernel's translation unit.
#include "wgrad_plan.h"
#include "wgrad_operand.h"

#include <cstring>

namespace apamd {

int launch_split_transpose(const ap_src* segs, int nseg, int N, int C, int H, int W, int pad, int pad_mode, int Hp, int X8, int Cp,
                           uint4* out, hipStream_t stream, int s2d_c, int heads_only, int rows_k) {
    SplitTParams p;
    memset(&p, 0, sizeof(p));
    p.nseg = nseg;
    int cbeg = 0;
    for (int s = 0; s < nseg; ++s) {
        fill_seg(p.seg[s], segs[s], cbeg);
        // ap_src.act bit 8: the segment's data are bf16 values (a raw output of ap_conv2d_fwd_bf16out); only the padded-row kernel reads those
        p.seg[s].act = segs[s].act & 0xff;
        p.seg[s].pad_ = (segs[s].act >> 8) & 1;
        cbeg += segs[s].C;
    }
    p.N = N; p.C = C; p.H = H; p.W = W; p.pad = pad; p.pad_mode = pad_mode; p.Hp = Hp; p.X8 = X8; p.Cp = Cp; p.out = out;
    p.s2d_c = s2d_c;
    p.heads_only = heads_only;
    p.rows_k = rows_k;
    const bool whole_rows = split_transpose_whole_rows(W, s2d_c);
    const int form = split_transpose_form(nseg, any_bf16_segment(segs, nseg), C, W, pad, X8, Cp, s2d_c, rows_k);
    if (form < 0) return split_transpose_refusal(form);
    if (N > 65535 || Cp / 64 > 65535) return fail(AP_ERR_UNSUPPORTED, "split_transpose: N=%d C=%d", N, C);
    const int R = whole_rows ? 256 / W : 1;                                       // source rows per workgroup of the row forms
    const size_t row_lds = (size_t)64 * (R * X8 * 8 + 1) * sizeof(float);
    int rc = AP_OK;
    switch (form) {
    case ST_VEC: {      // unpadded operand with whole octet rows: 16-byte loads, 1 KiB per wave
        const size_t lds = 64 * 257 * sizeof(float);
        if ((rc = ensure_dyn_lds(reinterpret_cast<const void*>(&split_transpose_vec_kernel), (int)lds))) return rc;
        hipLaunchKernelGGL(split_transpose_vec_kernel, dim3((Hp * X8 + 31) / 32, Cp / 64, N), dim3(256), lds, stream, p);
        return check_launch("split_transpose_vec_kernel");
    }
    case ST_PAD_ROWS:   // padded rows, 16-byte loads
        if ((rc = ensure_dyn_lds(reinterpret_cast<const void*>(&split_transpose_pad_kernel), 96 * 1024))) return rc;
        hipLaunchKernelGGL(split_transpose_pad_kernel, dim3((Hp + R - 1) / R, Cp / 64, N), dim3(256), row_lds, stream, p);
        return check_launch("split_transpose_pad_kernel");
    case ST_S2D_ROWS:   // space-to-depth view, whole source rows
        if ((rc = ensure_dyn_lds(reinterpret_cast<const void*>(&split_transpose_s2d_kernel), 96 * 1024))) return rc;
        hipLaunchKernelGGL(split_transpose_s2d_kernel, dim3(((Hp + R - 1) / R) * 2, s2d_c / 32, N), dim3(256), row_lds, stream, p);
        return check_launch("split_transpose_s2d_kernel");
    default:
        hipLaunchKernelGGL(split_transpose_kernel, dim3((Hp * X8 + 7) / 8, Cp / 64, N), dim3(256), 0, stream, p);
        return check_launch("split_transpose_kernel");
    }
}

// the shifted operand re-tiled from the forward pass's split copies (xs_transpose_kernel); C = channels of the view
int launch_xs_transpose(const void* const* xs, const int* seg_c, int nseg, int N, int H, int W, int pad, int pad_mode, int Hp, int X8,
                        int Cp, int parts, uint4* out, hipStream_t stream, int s2d_c, int H0, int W0) {
    XsTParams p;
    memset(&p, 0, sizeof(p));
    p.nseg = nseg;
    int cg = 0;
    for (int s = 0; s < nseg; ++s) {
        p.xs[s] = reinterpret_cast<const uint4*>(xs[s]);
        p.cg_begin[s] = cg;
        cg += seg_c[s] / 8;
    }
    p.cg_begin[nseg] = cg;
    p.N = N; p.H = H; p.W = W; p.pad = pad; p.pad_mode = pad_mode; p.Hp = Hp; p.X8 = X8; p.Cp = Cp; p.parts = parts; p.out = out;
    p.s2d_c = s2d_c; p.H0 = H0; p.W0 = W0;
    if (N > 65535 || Cp / 8 > 65535) return fail(AP_ERR_UNSUPPORTED, "xs_transpose: N=%d Cp=%d", N, Cp);
    hipLaunchKernelGGL(xs_transpose_kernel, dim3((Hp * X8 + 31) / 32, (Cp / 8 + kXsCgPerThread - 1) / kXsCgPerThread, N), dim3(256), 0,
                       stream, p);
    return check_launch("xs_transpose_kernel");
}

// the shifted operand of a bf16 GEMM plan in pixel-octet slots: from the forward pass's split copies or from the fp32 tensors
int launch_bf16_gemm_operand(const ap_wgrad_desc* d, const WgradPlan& pl, bool from_xs, uint4* at, hipStream_t stream) {
    const Bf16GemmPlan& b = pl.bf;
    const bool b16 = d->precision == AP_PRECISION_BF16;
    if (!from_xs)
        return launch_split_transpose(d->src, d->nsrc, d->N, b.Cb, d->H, d->W, b.s2d ? 0 : d->pad, d->pad_mode, b.Hp, b.AX8, b.Cp, at,
                                      stream, b.s2d ? pl.Cin : 0, b16, b.rows ? b.Kb : 0);
    const int parts = b16 ? 1 : 2;
    if (b.s2d) {
        // the forward pass staged the space-to-depth copy (2 x 2 form) or, where it ran the stride-2 kernel, the plain one
        const void* xs[1] = {d->src_xs_s2d ? d->src_xs_s2d : d->src_xs[0]};
        const int cs[1] = {b.Cb};
        return launch_xs_transpose(xs, cs, 1, d->N, b.Hb, b.Wb, 0, AP_PAD_ZERO, b.Hp, b.AX8, b.Cp, parts, at, stream,
                                   d->src_xs_s2d ? 0 : pl.Cin, d->H, d->W);
    }
    int cs[kMaxSeg];
    for (int s = 0; s < d->nsrc; ++s) cs[s] = d->src[s].C;
    return launch_xs_transpose(d->src_xs, cs, d->nsrc, d->N, d->H, d->W, d->pad, d->pad_mode, b.Hp, b.AX8, b.Cp, parts, at, stream);
}

}  // namespace apamd
