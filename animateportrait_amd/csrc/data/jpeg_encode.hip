// apd_jpeg_encode: a batch of fp32 NCHW frames -> one complete baseline JPEG file per frame, on the device
// (include/animateportrait_data.h; the file layout and every piece of arithmetic are in jpeg_core.h).
//
// Three launches, no atomics on global memory, no synchronisation:
//   jpeg_transform_kernel  one lane per 8x8 block of one component: the bytes of apd_frames_to_u8 (edges replicated), the
//                          colour conversion, the level shift, the DCT with quantisation; 64 zigzag int16 to the workspace.
//   jpeg_segment_kernel    one workgroup per (MCU row, frame): a restart interval.  CHUNK_BLOCKS blocks at a time: bit counts,
//                          a workgroup scan (wave64 shuffles, the four wave sums through LDS), the bits OR-ed into an LDS
//                          word buffer, then the chunk's whole bytes copied to the workspace with 0xFF stuffed -- a second
//                          scan over the 0xFF counts places every lane's run.  The last chunk pads with 1-bits; RSTm follows
//                          every segment but the last.
//   jpeg_frame_kernel      a few workgroups per frame: prefix sum of the segment sizes, the header, then the slot's dwords --
//                          header, segments, EOI -- each in exactly one lane, the last 1..3 bytes singly so that nothing
//                          past sizes[n] is written.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../../include/animateportrait_data.h"
#include "apd_common.h"
#include "jpeg_core.h"

namespace {

using apd::fail;
using namespace apd_jpeg;

constexpr int THREADS = CHUNK_BLOCKS;
constexpr int WAVES = THREADS / 64;
constexpr int HEADER_MAX = 616;
static_assert(THREADS == 256, "the scan is written for four waves");

struct Shape {
    int C, H, W, channels, quality, rows, mcus, bpr;     // bpr: blocks per MCU row
    long long stride;                                     // bytes of a segment's slot in the workspace
};

__global__ __launch_bounds__(THREADS) void jpeg_transform_kernel(const float* __restrict__ src, int16_t* __restrict__ coef, Shape sh,
                                                                 long long total) {
    __shared__ uint16_t qt[2][64];
    const int t = threadIdx.x;
    if (t < 128) qt[t >> 6][t & 63] = (uint16_t)scaled_quant(t >> 6, t & 63, sh.quality);
    __syncthreads();
    const long long idx = (long long)blockIdx.x * THREADS + t;
    if (idx >= total) return;
    const int b = (int)(idx % sh.bpr), row = (int)((idx / sh.bpr) % sh.rows);
    const long long n = idx / ((long long)sh.bpr * sh.rows);
    const int comp = b % sh.channels, mcu = b / sh.channels;
    const long long plane = (long long)sh.H * sh.W;
    const float* p = src + n * sh.C * plane;
    int s[64];
#pragma unroll
    for (int y = 0; y < 8; ++y) {
        const int yy = min(row * 8 + y, sh.H - 1);
#pragma unroll
        for (int x = 0; x < 8; ++x) {
            const int xx = min(mcu * 8 + x, sh.W - 1);
            const long long at = (long long)yy * sh.W + xx;
            const int r = (int)apd::to_byte(p[at]);
            int v = r;
            if (sh.channels == 3 && sh.C == 3)
                v = component_sample(r, (int)apd::to_byte(p[plane + at]), (int)apd::to_byte(p[2 * plane + at]), comp);
            else if (sh.channels == 3)
                v = component_sample(r, r, r, comp);
            s[y * 8 + x] = v - 128;
        }
    }
    int16_t zz[64];
    fdct_quant_block(s, qt[comp ? 1 : 0], zz);
    uint32_t* out = reinterpret_cast<uint32_t*>(coef + idx * 64);
#pragma unroll
    for (int i = 0; i < 32; ++i) out[i] = (uint32_t)(uint16_t)zz[2 * i] | ((uint32_t)(uint16_t)zz[2 * i + 1] << 16);
}

// exclusive scan of v over the workgroup; *total = the sum.  wsum: WAVES words of LDS.
__device__ __forceinline__ uint32_t block_scan(uint32_t* wsum, uint32_t v, uint32_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    __syncthreads();                                       // the last scan's readers are done with wsum
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint32_t base = 0, all = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const uint32_t s = wsum[w];
        base += w < wave ? s : 0u;
        all += s;
    }
    *total = all;
    return base + inc - v;
}

__global__ __launch_bounds__(THREADS) void jpeg_segment_kernel(const int16_t* __restrict__ coef, uint32_t* __restrict__ seg_sizes,
                                                               uint8_t* __restrict__ segs, Shape sh) {
    extern __shared__ uint32_t bitbuf[];                   // bitbuf_words(min(CHUNK_BLOCKS, bpr))
    __shared__ uint32_t dc_tab[2][16], ac_tab[2][256];
    __shared__ uint32_t wsum[WAVES];
    const int t = threadIdx.x, row = blockIdx.x, n = blockIdx.y;
    if (t < 4) build_huffman(t, t < 2 ? dc_tab[t] : ac_tab[t - 2]);
    const long long seg_index = (long long)n * sh.rows + row;
    const int16_t* row_coef = coef + seg_index * sh.bpr * 64;
    uint8_t* seg = segs + seg_index * sh.stride;
    uint32_t out_pos = 0, carry_bits = 0, carry_byte = 0;
    __syncthreads();
    for (int b0 = 0; b0 < sh.bpr; b0 += THREADS) {
        const int b = b0 + t;
        const bool mine = b < sh.bpr, last = b0 + THREADS >= sh.bpr;
        const int tab = mine && sh.channels == 3 && b % 3 != 0 ? 1 : 0;
        const int pred = mine ? dc_prediction(row_coef, b, sh.channels) : 0;
        const uint32_t bits = mine ? encode_block<false>(row_coef + (long long)b * 64, pred, dc_tab[tab], ac_tab[tab], nullptr) : 0u;
        uint32_t chunk_bits;
        const uint32_t first = carry_bits + block_scan(wsum, bits, &chunk_bits);
        uint32_t tot = carry_bits + chunk_bits;
        const uint32_t words = (tot + 31) / 32 + 2;        // <= bitbuf_words(blocks of this chunk)
        for (uint32_t w = t; w < words; w += THREADS) bitbuf[w] = w == 0 ? carry_byte << 24 : 0u;
        __syncthreads();
        if (mine) {
            BitWriter bw = bit_writer(bitbuf, first);
            encode_block<true>(row_coef + (long long)b * 64, pred, dc_tab[tab], ac_tab[tab], &bw);
            finish_bits(bw);
        }
        const uint32_t pad = last ? (8u - (tot & 7u)) & 7u : 0u;
        if (t == 0 && pad) {                               // the segment ends on a byte boundary, filled with 1-bits
            BitWriter bw = bit_writer(bitbuf, tot);
            put_bits(bw, (1u << pad) - 1u, (int)pad);
            finish_bits(bw);
        }
        tot += pad;
        __syncthreads();
        const uint32_t nby = tot >> 3, per = (nby + THREADS - 1) / THREADS;
        const uint32_t j0 = min((uint32_t)t * per, nby), j1 = min(j0 + per, nby);
        uint32_t ff_all;
        const uint32_t ff_before = block_scan(wsum, count_ff(bitbuf, j0, j1), &ff_all);
        copy_stuffed(bitbuf, j0, j1, seg + out_pos + j0 + ff_before);
        out_pos += nby + ff_all;
        carry_bits = tot & 7u;
        carry_byte = carry_bits ? get_byte(bitbuf, nby) & (0xFF00u >> carry_bits) & 255u : 0u;
        __syncthreads();                                   // every lane has read the buffer before the next chunk clears it
    }
    if (t == 0) {
        if (row + 1 < sh.rows) {
            seg[out_pos] = 0xFF;
            seg[out_pos + 1] = (uint8_t)(0xD0 + (row & 7));
            out_pos += 2;
        }
        seg_sizes[seg_index] = out_pos;
    }
}

__global__ __launch_bounds__(THREADS) void jpeg_frame_kernel(const uint32_t* __restrict__ seg_sizes, const uint8_t* __restrict__ segs,
                                                             uint8_t* __restrict__ dst, int32_t* __restrict__ sizes, Shape sh,
                                                             long long slot_bytes) {
    __shared__ uint32_t off[MAX_MCU_ROWS + 1];
    __shared__ uint8_t head[HEADER_MAX];
    __shared__ int head_bytes;
    const int t = threadIdx.x, n = blockIdx.y;
    for (int r = t; r < sh.rows; r += THREADS) off[r + 1] = seg_sizes[(long long)n * sh.rows + r];
    __syncthreads();
    if (t == 0) {
        uint32_t at = 0;
        off[0] = 0;
        for (int r = 0; r < sh.rows; ++r) {
            at += off[r + 1];
            off[r + 1] = at;
        }
        head_bytes = write_header(head, sh.W, sh.H, sh.channels, sh.quality);
    }
    __syncthreads();
    const uint32_t hb = (uint32_t)head_bytes, body = off[sh.rows], size = hb + body + 2;
    const uint8_t* frame_segs = segs + (long long)n * sh.rows * sh.stride;
    uint8_t* slot = dst + (long long)n * slot_bytes;
    auto file_byte = [&](uint32_t k) -> uint32_t {
        if (k < hb) return head[k];
        k -= hb;
        if (k >= body) return k == body ? 0xFFu : 0xD9u;
        const int r = segment_of(off, sh.rows, k);
        return frame_segs[(long long)r * sh.stride + (k - off[r])];
    };
    const uint32_t full = size >> 2;
    for (uint32_t j = blockIdx.x * THREADS + t; j < full; j += gridDim.x * THREADS) {
        const uint32_t k = 4 * j;
        reinterpret_cast<uint32_t*>(slot)[j] = file_byte(k) | (file_byte(k + 1) << 8) | (file_byte(k + 2) << 16) | (file_byte(k + 3) << 24);
    }
    if (blockIdx.x == 0) {
        if (t < (int)(size & 3u)) slot[4 * full + t] = (uint8_t)file_byte(4 * full + t);
        if (t == 0) sizes[n] = (int32_t)size;
    }
}

int check_jpeg(const float* src, const uint8_t* dst, const int32_t* sizes, const void* ws, int N, int C, int H, int W, int channels,
               int quality, long long slot_bytes, long long ws_bytes) {
    if (!src || !dst || !sizes || !ws) return fail(APD_ERR_INVALID, "jpeg_encode: null src / dst / sizes / workspace");
    if (C != 1 && C != 3) return fail(APD_ERR_UNSUPPORTED, "jpeg_encode: C = %ld, served: 1 and 3", C);
    if (channels != 1 && channels != 3) return fail(APD_ERR_UNSUPPORTED, "jpeg_encode: channels = %ld, served: 1 and 3", channels);
    if (channels == 1 && C != 1) return fail(APD_ERR_UNSUPPORTED, "jpeg_encode: channels = 1 (greyscale) needs C = 1, not C = %ld", C);
    if (quality < 1 || quality > 100) return fail(APD_ERR_INVALID, "jpeg_encode: quality = %ld, served: 1 .. 100", quality);
    if (N < 1 || N > 65535) return fail(APD_ERR_INVALID, "jpeg_encode: N = %ld, served: 1 .. 65535", N);
    if (H < 1 || H > APD_MAX_JPEG_SIDE || W < 1 || W > APD_MAX_JPEG_SIDE)
        return fail(APD_ERR_UNSUPPORTED, "jpeg_encode: %ld x %ld, served: sides 1 .. %ld", H, W, APD_MAX_JPEG_SIDE);
    if (slot_bytes < frame_bound(H, W, channels))
        return fail(APD_ERR_INVALID, "jpeg_encode: slot_bytes = %ld is below apd_jpeg_bound = %ld", slot_bytes, frame_bound(H, W, channels));
    if ((slot_bytes & 3) != 0) return fail(APD_ERR_INVALID, "jpeg_encode: slot_bytes = %ld is not a multiple of 4", slot_bytes);
    if ((long long)N * slot_bytes >= (1LL << 31))
        return fail(APD_ERR_UNSUPPORTED, "jpeg_encode: %ld slots of %ld bytes, served: below 2^31 in all", N, slot_bytes);
    if (ws_bytes < workspace_bytes(N, H, W, channels))
        return fail(APD_ERR_INVALID, "jpeg_encode: workspace of %ld bytes, needed: %ld (apd_jpeg_workspace_bytes)", ws_bytes,
                    workspace_bytes(N, H, W, channels));
    if (((uintptr_t)dst & 3) != 0 || ((uintptr_t)sizes & 3) != 0 || ((uintptr_t)ws & 3) != 0)
        return fail(APD_ERR_INVALID, "jpeg_encode: dst / sizes / workspace is not 4-byte aligned");
    return APD_OK;
}

// device memory as it is, pinned host memory through the address the device maps it at, anything else: null
void* device_address(const void* p) {
    hipPointerAttribute_t attr;
    (void)hipGetLastError();
    const hipError_t pe = hipPointerGetAttributes(&attr, p);
    void* target = nullptr;
    if (pe == hipSuccess && attr.type == hipMemoryTypeDevice) target = const_cast<void*>(p);
    else if (pe == hipSuccess && attr.type == hipMemoryTypeHost && attr.devicePointer && attr.hostPointer)
        // p may point into the allocation: whichever of its addresses the runtime reports, keep p's distance from it
        target = static_cast<char*>(attr.devicePointer) + (static_cast<const char*>(p) - static_cast<const char*>(attr.hostPointer));
    if (pe != hipSuccess) (void)hipGetLastError();
    return ((uintptr_t)target & 3) == 0 ? target : nullptr;
}

}  // namespace

extern "C" {

int64_t apd_jpeg_bound(int32_t H, int32_t W, int32_t channels) {
    if (H < 1 || H > APD_MAX_JPEG_SIDE || W < 1 || W > APD_MAX_JPEG_SIDE || (channels != 1 && channels != 3)) {
        fail(APD_ERR_UNSUPPORTED, "jpeg_bound: %ld x %ld x %ld, served: sides 1 .. 2048, channels 1 and 3", H, W, channels);
        return -1;
    }
    return frame_bound(H, W, channels);
}

int64_t apd_jpeg_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t channels) {
    if (N < 1 || N > 65535 || apd_jpeg_bound(H, W, channels) < 0) {
        if (N < 1 || N > 65535) fail(APD_ERR_INVALID, "jpeg_workspace_bytes: N = %ld, served: 1 .. 65535", N);
        return -1;
    }
    return workspace_bytes(N, H, W, channels);
}

int32_t apd_jpeg_encode_ok(const float* src, const uint8_t* dst, const int32_t* sizes, const void* ws, int32_t N, int32_t C, int32_t H,
                           int32_t W, int32_t channels, int32_t quality, int64_t slot_bytes, int64_t ws_bytes) {
    return check_jpeg(src, dst, sizes, ws, N, C, H, W, channels, quality, slot_bytes, ws_bytes) == APD_OK ? 1 : 0;
}

int apd_jpeg_encode(const float* src, int32_t N, int32_t C, int32_t H, int32_t W, int32_t channels, int32_t quality, uint8_t* dst,
                    int64_t slot_bytes, int32_t* sizes, void* ws, int64_t ws_bytes, void* stream) {
    const int rc = check_jpeg(src, dst, sizes, ws, N, C, H, W, channels, quality, slot_bytes, ws_bytes);
    if (rc != APD_OK) return rc;
    uint8_t* target = static_cast<uint8_t*>(device_address(dst));
    int32_t* target_sizes = static_cast<int32_t*>(device_address(sizes));
    if (!target || !target_sizes)
        return fail(APD_ERR_INVALID, "jpeg_encode: dst / sizes is neither device memory nor pinned host memory mapped for the device");
    Shape sh;
    sh.C = C; sh.H = H; sh.W = W; sh.channels = channels; sh.quality = quality;
    sh.rows = mcu_rows(H);
    sh.mcus = mcus_per_row(W);
    sh.bpr = blocks_per_row(W, channels);
    sh.stride = segment_stride(W, channels);
    int16_t* coef = static_cast<int16_t*>(ws);
    uint32_t* seg_sizes = reinterpret_cast<uint32_t*>(static_cast<char*>(ws) + coef_bytes(N, H, W, channels));
    uint8_t* segs = reinterpret_cast<uint8_t*>(seg_sizes + (long long)N * sh.rows);
    const long long total = (long long)N * sh.rows * sh.bpr;
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(jpeg_transform_kernel, dim3((unsigned)((total + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, src, coef, sh, total);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        const size_t lds = sizeof(uint32_t) * (size_t)bitbuf_words(sh.bpr < CHUNK_BLOCKS ? sh.bpr : CHUNK_BLOCKS);
        hipLaunchKernelGGL(jpeg_segment_kernel, dim3((unsigned)sh.rows, (unsigned)N), dim3(THREADS), lds, s, coef, seg_sizes, segs, sh);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        const unsigned blocks = (unsigned)(sh.rows < 32 ? sh.rows : 32);
        hipLaunchKernelGGL(jpeg_frame_kernel, dim3(blocks, (unsigned)N), dim3(THREADS), 0, s, seg_sizes, segs, target, target_sizes, sh,
                           (long long)slot_bytes);
        e = hipGetLastError();
    }
    if (e != hipSuccess) {
        snprintf(apd::g_err, sizeof(apd::g_err), "jpeg_encode: launch failed: %s", hipGetErrorString(e));
        return APD_ERR_LAUNCH;
    }
    return APD_OK;
}

}  // extern "C"
