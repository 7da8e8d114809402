// conv_pack.hip -- the weight packer: a layer's weights into the image its plan's kernel stages (conv_plan.h), per launch.
#include "conv_plan.h"
#include "conv_pack.h"

#include <algorithm>
#include <cstring>

namespace apamd {

// ------------------------------------------------------------------ weight packer
struct PackParams {
    const float* w;
    float* out;
    int Cin, Cout, K, layout;
    int nseg, segC[kMaxSeg], chunk_begin[kMaxSeg];
    int CI, CO_TILE, nchunks, co_tiles, ntaps, wfloats;
    int tap_ky[kMaxTaps], tap_kx[kMaxTaps];
};

__global__ void pack_weights_kernel(const PackParams p) {
    const long long total = (long long)p.co_tiles * p.nchunks * p.wfloats;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        const int within = (int)(idx % p.wfloats);
        const long long blk = idx / p.wfloats;
        const int chunk = (int)(blk % p.nchunks);
        const int cot = (int)(blk / p.nchunks);
        float v = 0.f;
        if (within < p.ntaps * p.CI * p.CO_TILE) {
            const int col = within % p.CO_TILE;
            const int ci = (within / p.CO_TILE) % p.CI;
            const int t = within / (p.CO_TILE * p.CI);
            const int co = cot * p.CO_TILE + col;
            int s = 0;
            if (p.nseg > 1 && chunk >= p.chunk_begin[1]) s = 1;
            if (p.nseg > 2 && chunk >= p.chunk_begin[2]) s = 2;
            const int cs = (chunk - p.chunk_begin[s]) * p.CI + ci;
            if (cs < p.segC[s] && co < p.Cout) {
                int cin = cs;
                for (int j = 0; j < s; ++j) cin += p.segC[j];
                const int ky = p.tap_ky[t], kx = p.tap_kx[t];
                const long long off = p.layout == AP_W_OIHW
                                          ? (((long long)co * p.Cin + cin) * p.K + ky) * p.K + kx
                                          : (((long long)cin * p.Cout + co) * p.K + ky) * p.K + kx;
                v = p.w[off];
            }
        }
        p.out[idx] = v;
    }
}

struct PackDirectParams {
    const float* w;
    float* out;
    int Cin, Cout, K, layout, flip, COP, CI, nchunks;
    int nseg, segC[kMaxSeg], chunk_begin[kMaxSeg];
};

// out[cin_pad][K][K][COP]
__global__ void pack_direct_kernel(const PackDirectParams p) {
    const int total = p.nchunks * p.CI * p.K * p.K * p.COP;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const int co = idx % p.COP;
        int t = idx / p.COP;
        int kx = t % p.K; t /= p.K;
        int ky = t % p.K; t /= p.K;
        const int ci = t % p.CI;
        const int chunk = t / p.CI;
        int s = 0;
        if (p.nseg > 1 && chunk >= p.chunk_begin[1]) s = 1;
        if (p.nseg > 2 && chunk >= p.chunk_begin[2]) s = 2;
        const int cs = (chunk - p.chunk_begin[s]) * p.CI + ci;
        float v = 0.f;
        if (cs < p.segC[s] && co < p.Cout) {
            int cin = cs;
            for (int j = 0; j < s; ++j) cin += p.segC[j];
            if (p.flip) { ky = p.K - 1 - ky; kx = p.K - 1 - kx; }
            const long long off = p.layout == AP_W_OIHW ? (((long long)co * p.Cin + cin) * p.K + ky) * p.K + kx
                                                        : (((long long)cin * p.Cout + co) * p.K + ky) * p.K + kx;
            v = p.w[off];
        }
        p.out[idx] = v;
    }
}

// the packer's parameters for one launch of a split-bf16 plan; `v` (nullable): the weight as a strided / derived view
static PackBf3Params bf3_pack_params(const ap_conv_desc* d, const Plan& pl, const Launch& L, const float* weight,
                                     const ap_weight_view* v, float* packed) {
    PackBf3Params p;
    memset(&p, 0, sizeof(p));
    p.w = v ? v->w : weight;
    p.out = reinterpret_cast<unsigned short*>(packed + L.wp_off);
    p.Cin = pl.Cin; p.Cout = d->Cout; p.K = d->KW; p.layout = d->w_layout; p.flip = 0;
    p.KH = d->KH != d->KW ? d->KH : 0;
    p.nseg = d->nsrc;
    for (int s = 0; s < d->nsrc; ++s) { p.segC[s] = d->src[s].C; p.chunk_begin[s] = pl.chunk_begin[s]; }
    p.CO_TILE = pl.bk->CO_TILE; p.nchunks = pl.nchunks; p.co_tiles = pl.co_tiles;
    p.ntaps = (int)L.taps.size();
    for (int t = 0; t < p.ntaps; ++t) { p.tap_ky[t] = L.taps[t].ky; p.tap_kx[t] = L.taps[t].kx; }
    if (v) {
        p.view = 1;
        p.s_co = v->s_co; p.s_ci = v->s_ci; p.s_ky = v->s_ky; p.s_kx = v->s_kx;
        p.s2d_c = v->s2d_c; p.rows_c = v->rows_c; p.ksrc = v->ksrc;
    }
    return p;
}

}  // namespace apamd

using namespace apamd;

extern "C" {

int ap_conv2d_pack_weights(const ap_conv_desc* d, const float* weight, float* packed, ap_stream_t stream) {
    Plan pl;
    int rc = make_plan(d, pl);
    if (rc) return rc;
    if (!weight || !packed) return fail(AP_ERR_INVALID, "null weight/packed pointer");
    if (pl.small) {
        hipError_t e = hipMemcpyAsync(packed, weight, (size_t)pl.packed_floats * sizeof(float), hipMemcpyDeviceToDevice,
                                      (hipStream_t)stream);
        if (e != hipSuccess) return fail(AP_ERR_LAUNCH, "pack (copy) weights: %s", hipGetErrorString(e));
        return AP_OK;
    }
    if (pl.direct_cop) {
        PackDirectParams p;
        memset(&p, 0, sizeof(p));
        p.w = weight; p.out = packed;
        p.Cin = pl.Cin; p.Cout = d->Cout; p.K = d->KH; p.layout = d->w_layout; p.flip = d->w_flip;
        p.COP = pl.direct_cop; p.CI = 4; p.nchunks = pl.nchunks; p.nseg = d->nsrc;
        for (int s = 0; s < d->nsrc; ++s) { p.segC[s] = d->src[s].C; p.chunk_begin[s] = pl.chunk_begin[s]; }
        hipLaunchKernelGGL(pack_direct_kernel, dim3(64), dim3(256), 0, (hipStream_t)stream, p);
        return check_launch("pack_direct_kernel");
    }
    if (pl.bf3) {
        for (const auto& L : pl.launches) {
            const PackBf3Params p = bf3_pack_params(d, pl, L, weight, nullptr, packed);
            hipLaunchKernelGGL(pack_bf16x3_kernel, dim3(1024), dim3(256), 0, (hipStream_t)stream, p);
            rc = check_launch("pack_bf16x3_kernel");
            if (rc) return rc;
        }
        return AP_OK;
    }
    for (const auto& L : pl.launches) {
        PackParams p;
        memset(&p, 0, sizeof(p));
        p.w = weight;
        p.out = packed + L.wp_off;
        p.Cin = pl.Cin; p.Cout = d->Cout; p.K = d->KH; p.layout = d->w_layout;
        p.nseg = d->nsrc;
        for (int s = 0; s < d->nsrc; ++s) { p.segC[s] = d->src[s].C; p.chunk_begin[s] = pl.chunk_begin[s]; }
        p.CI = pl.k->CI; p.CO_TILE = pl.k->CO_TILE; p.nchunks = pl.nchunks; p.co_tiles = pl.co_tiles;
        p.ntaps = (int)L.taps.size();
        p.wfloats = pl.k->wfloats(p.ntaps);
        for (int t = 0; t < p.ntaps; ++t) { p.tap_ky[t] = L.taps[t].ky; p.tap_kx[t] = L.taps[t].kx; }
        const long long total = (long long)p.co_tiles * p.nchunks * p.wfloats;
        int blocks = (int)std::min<long long>((total + 255) / 256, 2048);
        hipLaunchKernelGGL(pack_weights_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p);
        rc = check_launch("pack_weights_kernel");
        if (rc) return rc;
    }
    if (pl.head_w_off >= 0) {
        hipError_t e = hipMemcpyAsync(packed + pl.head_w_off, weight, (size_t)pl.Cin * d->Cout * d->KH * d->KW * sizeof(float),
                                      hipMemcpyDeviceToDevice, (hipStream_t)stream);
        if (e != hipSuccess) return fail(AP_ERR_LAUNCH, "pack (head copy) weights: %s", hipGetErrorString(e));
    }
    return AP_OK;
}

int32_t ap_conv2d_pack_entry_bytes(void) { return (int32_t)sizeof(PackBf3Params); }

int32_t ap_conv2d_pack_entries(const ap_conv_desc* d, const ap_weight_view* v, float* packed, void* entries, int32_t max_entries) {
    Plan pl;
    int rc = make_plan(d, pl);
    if (rc) return rc;
    if (!v || !v->w || !packed) return fail(AP_ERR_INVALID, "pack_entries: null view / packed pointer");
    if (!pl.bf3) return 0;                                   // not a split-bf16 plan: use ap_conv2d_pack_weights
    if ((int)pl.launches.size() > max_entries || !entries) return fail(AP_ERR_INVALID, "pack_entries: room for %d entries, plan has %d", max_entries, (int)pl.launches.size());
    if ((v->s2d_c > 0 || v->rows_c > 0) && v->ksrc < 1) return fail(AP_ERR_INVALID, "pack_entries: derived views need ksrc");
    PackBf3Params* out = reinterpret_cast<PackBf3Params*>(entries);
    int n = 0;
    for (const auto& L : pl.launches) out[n++] = bf3_pack_params(d, pl, L, nullptr, v, packed);
    return n;
}

int ap_conv2d_pack_run(const void* entries_dev, int32_t count, ap_stream_t stream) {
    if (!entries_dev || count < 1 || count > 65535) return fail(AP_ERR_INVALID, "pack_run: bad table");
    hipLaunchKernelGGL(pack_bf16x3_table_kernel, dim3(48, count), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const PackBf3Params*>(entries_dev));
    return check_launch("pack_bf16x3_table_kernel");
}

}  // extern "C"
