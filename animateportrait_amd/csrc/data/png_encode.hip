// apd_png_encode: a batch of fp32 NCHW frames -> one complete PNG file per frame, on the device
// (include/animateportrait_data.h; the stream layout and every piece of arithmetic are in png_deflate.h).
//
// Two launches, no atomics, no synchronisation:
//   png_band_kernel    one workgroup per (band, frame).  The band's filtered bytes are staged in LDS as packed dwords (the
//                      bytes are apd_frames_to_u8's); lane s encodes segment s into its own LDS area and sums its Adler part;
//                      a workgroup scan turns bit counts into bit offsets; then every lane gathers a contiguous run of the
//                      chunk's dwords, stores them to the workspace and carries their CRC in a register; the partial CRCs are
//                      combined with x^(8 n) mod P.  One lane closes the chunk (length, type, last bytes, CRC) and its record.
//   png_finish_kernel  a few workgroups per frame.  Each reads the frame's band records, prefix-sums the chunk sizes and
//                      chains the Adler parts (one lane, <= 1024 bands), then assembles the slot's dwords -- head, chunks,
//                      tail -- each in exactly one lane, the last 1..3 bytes singly so that nothing past sizes[n] is written.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../../include/animateportrait_data.h"
#include "apd_common.h"
#include "png_deflate.h"

namespace {

using apd::fail;
using namespace apd_png;

constexpr int THREADS = 256;
constexpr int FINISH_BLOCKS = 4;

struct Shape {
    int C, H, W, channels, rb, rows, bands;
    long long stride;          // bytes of a band's chunk slot in the workspace
};

// byte x of image row y of frame n, as apd_frames_to_u8 writes it (channels 1: the single plane)
struct Pixels {
    const float* src;
    long long plane;
    int W, C, channels;
    __device__ uint32_t operator()(int y, int x) const {
        const int px = channels == 3 ? x / 3 : x, ch = channels == 3 ? x - px * 3 : 0;
        return apd::to_byte(src[(C == 3 ? ch : 0) * plane + (long long)y * W + px]);
    }
};

__device__ __forceinline__ uint32_t block_reduce(uint32_t* red, uint32_t v, bool is_xor) {
    const int t = threadIdx.x;
    __syncthreads();
    red[t] = v;
    __syncthreads();
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if (t < s) red[t] = is_xor ? red[t] ^ red[t + s] : red[t] + red[t + s];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(THREADS) void png_band_kernel(const float* __restrict__ src, uint32_t* __restrict__ meta,
                                                           uint32_t* __restrict__ chunks, Shape sh) {
    __shared__ uint32_t raw_w[BAND_BYTES / 4];
    __shared__ uint32_t areas[(MAX_SEGMENTS + 1) * AREA_WORDS + 1];
    __shared__ uint32_t bit_off[THREADS + 1];
    __shared__ uint32_t crc_tab[256];
    __shared__ uint32_t red[THREADS];
    const int t = threadIdx.x, band = blockIdx.x, n = blockIdx.y;
    const int y0 = band * sh.rows, rows = min(sh.rows, sh.H - y0), nbytes = rows * sh.rb;
    const int nseg = (nbytes + SEGMENT - 1) / SEGMENT;
    const uint8_t* raw = reinterpret_cast<const uint8_t*>(raw_w);
    const long long plane = (long long)sh.H * sh.W;
    const Pixels px{src + (long long)n * sh.C * plane, plane, sh.W, sh.C, sh.channels};

    crc_tab[t] = crc_table_entry((uint32_t)t);
    for (int d = t; d < (nbytes + 3) / 4; d += THREADS) {
        uint32_t w = 0;
        for (int k = 0; k < 4; ++k)
            if (4 * d + k < nbytes) w |= filtered_byte(px, 4 * d + k, sh.rb, sh.channels, y0) << (8 * k);
        raw_w[d] = w;
    }
    __syncthreads();

    uint32_t bits = 0, asum = 0, aweighted = 0;
    if (t < nseg) {
        bits = encode_segment(raw, nbytes, t, band == 0, areas + t * AREA_WORDS);
        const int start = t * SEGMENT, len = min(SEGMENT, nbytes - start);
        adler_part(raw + start, len, &asum, &aweighted);
        aweighted = (uint32_t)((aweighted + (uint64_t)(nbytes - start - len) * asum) % ADLER_MOD);
    }
    // exclusive scan of the bit counts (Hillis-Steele over THREADS entries)
    bit_off[t + 1] = bits;
    if (t == 0) bit_off[0] = 0;
    __syncthreads();
    for (int s = 1; s < THREADS; s <<= 1) {
        const uint32_t add = t + 1 > s ? bit_off[t + 1 - s] : 0u;
        __syncthreads();
        bit_off[t + 1] += add;
        __syncthreads();
    }
    if (t == 0) bit_off[nseg + 1] = bit_off[nseg] + encode_trailer(bit_off[nseg], areas + nseg * AREA_WORDS);
    const uint32_t band_sum = block_reduce(red, asum, false) % ADLER_MOD;
    const uint32_t band_weighted = block_reduce(red, aweighted, false) % ADLER_MOD;       // 256 terms below 65521 each
    const int count = nseg + 1;
    const uint32_t len = bit_off[count] >> 3, full = len >> 2;             // the chunk's data bytes, its whole dwords
    uint32_t* chunk = chunks + ((long long)n * sh.bands + band) * (sh.stride / 4);

    const uint32_t per = (full + THREADS - 1) / THREADS;
    const uint32_t j0 = min((uint32_t)t * per, full), j1 = min(j0 + per, full);
    uint32_t state = 0;
    for (uint32_t j = j0; j < j1; ++j) {
        const uint32_t w = gather_dword(areas, bit_off, count, j);
        chunk[2 + j] = w;
        state = crc_dword(crc_tab, state, w);
    }
    if (j1 > j0) state = crc_mulmod(state, crc_x8n(4 * (full - j1)));
    uint32_t crc = block_reduce(red, state, true);
    if (t == 0) {
        crc ^= crc_mulmod(CRC_STATE_IDAT, crc_x8n(4 * full));
        // the last 0..3 data bytes, then the CRC, big-endian: 4..7 bytes from dword 2 + full on, zero-padded
        const uint32_t last = gather_dword(areas, bit_off, count, full), rest = len & 3u;
        for (uint32_t k = 0; k < rest; ++k) crc = crc_byte(crc_tab, crc, (last >> (8 * k)) & 255u);
        crc = ~crc;
        const uint32_t be = __builtin_bswap32(crc);
        const uint64_t both = (uint64_t)(rest ? last & ((1u << (8 * rest)) - 1) : 0u) | ((uint64_t)be << (8 * rest));
        chunk[2 + full] = (uint32_t)both;
        chunk[3 + full] = (uint32_t)(both >> 32);
        chunk[0] = __builtin_bswap32(len);
        chunk[1] = 0x54414449u;                                            // "IDAT"
        uint32_t* m = meta + ((long long)n * sh.bands + band) * META_WORDS;
        m[0] = 12 + len;
        m[1] = band_sum;
        m[2] = band_weighted;
        m[3] = (uint32_t)nbytes;
    }
}

__global__ __launch_bounds__(THREADS) void png_finish_kernel(const uint32_t* __restrict__ meta, const uint8_t* __restrict__ chunks,
                                                             uint8_t* __restrict__ dst, int32_t* __restrict__ sizes, Shape sh,
                                                             long long slot_bytes) {
    __shared__ uint32_t off[MAX_BANDS + 1];
    __shared__ uint32_t part[MAX_BANDS * 3];
    __shared__ uint8_t head[HEAD_BYTES + 3], tail[TAIL_BYTES + 3];
    const int t = threadIdx.x, n = blockIdx.y;
    const uint32_t* m = meta + (long long)n * sh.bands * META_WORDS;
    for (int b = t; b < sh.bands; b += THREADS) {
        off[b + 1] = m[b * META_WORDS];
        for (int k = 0; k < 3; ++k) part[b * 3 + k] = m[b * META_WORDS + 1 + k];
    }
    __syncthreads();
    if (t == 0) {
        uint32_t A = 1, B = 0, at = 0;
        off[0] = 0;
        for (int b = 0; b < sh.bands; ++b) {
            at += off[b + 1];
            off[b + 1] = at;
            adler_append(&A, &B, part[b * 3], part[b * 3 + 1], part[b * 3 + 2]);
        }
        write_head(head, sh.W, sh.H, sh.channels);
        write_tail(tail, (B << 16) | A);
    }
    __syncthreads();
    const uint32_t body = off[sh.bands], size = HEAD_BYTES + body + TAIL_BYTES;
    const uint8_t* frame_chunks = chunks + (long long)n * sh.bands * sh.stride;
    uint8_t* slot = dst + (long long)n * slot_bytes;
    auto file_byte = [&](uint32_t k) -> uint32_t {
        if (k < HEAD_BYTES) return head[k];
        k -= HEAD_BYTES;
        if (k >= body) return tail[k - body];
        const int b = band_of(off, sh.bands, k);
        return frame_chunks[(long long)b * sh.stride + (k - off[b])];
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

int check_png(const float* src, const uint8_t* dst, const int32_t* sizes, const void* ws, int N, int C, int H, int W, int channels,
              long long slot_bytes, long long ws_bytes) {
    if (!src || !dst || !sizes || !ws) return fail(APD_ERR_INVALID, "png_encode: null src / dst / sizes / workspace");
    if (C != 1 && C != 3) return fail(APD_ERR_UNSUPPORTED, "png_encode: C = %ld, served: 1 and 3", C);
    if (channels != 1 && channels != 3) return fail(APD_ERR_UNSUPPORTED, "png_encode: channels = %ld, served: 1 and 3", channels);
    if (channels == 1 && C != 1) return fail(APD_ERR_UNSUPPORTED, "png_encode: channels = 1 (greyscale) needs C = 1, not C = %ld", C);
    if (N < 1 || N > 65535) return fail(APD_ERR_INVALID, "png_encode: N = %ld, served: 1 .. 65535", N);
    if (H < 1 || H > APD_MAX_PNG_SIDE || W < 1 || W > APD_MAX_PNG_SIDE)
        return fail(APD_ERR_UNSUPPORTED, "png_encode: %ld x %ld, served: sides 1 .. %ld", H, W, APD_MAX_PNG_SIDE);
    if (slot_bytes < frame_bound(H, W, channels))
        return fail(APD_ERR_INVALID, "png_encode: slot_bytes = %ld is below apd_png_bound = %ld", slot_bytes, frame_bound(H, W, channels));
    if ((slot_bytes & 3) != 0) return fail(APD_ERR_INVALID, "png_encode: slot_bytes = %ld is not a multiple of 4", slot_bytes);
    if ((long long)N * slot_bytes >= (1LL << 31))
        return fail(APD_ERR_UNSUPPORTED, "png_encode: %ld slots of %ld bytes, served: below 2^31 in all", N, slot_bytes);
    if (ws_bytes < workspace_bytes(N, H, W, channels))
        return fail(APD_ERR_INVALID, "png_encode: workspace of %ld bytes, needed: %ld (apd_png_workspace_bytes)", ws_bytes,
                    workspace_bytes(N, H, W, channels));
    if (((uintptr_t)dst & 3) != 0 || ((uintptr_t)sizes & 3) != 0 || ((uintptr_t)ws & 3) != 0)
        return fail(APD_ERR_INVALID, "png_encode: dst / sizes / workspace is not 4-byte aligned");
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

int64_t apd_png_bound(int32_t H, int32_t W, int32_t channels) {
    if (H < 1 || H > APD_MAX_PNG_SIDE || W < 1 || W > APD_MAX_PNG_SIDE || (channels != 1 && channels != 3)) {
        fail(APD_ERR_UNSUPPORTED, "png_bound: %ld x %ld x %ld, served: sides 1 .. 2048, channels 1 and 3", H, W, channels);
        return -1;
    }
    return frame_bound(H, W, channels);
}

int64_t apd_png_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t channels) {
    if (N < 1 || N > 65535 || apd_png_bound(H, W, channels) < 0) {
        if (N < 1 || N > 65535) fail(APD_ERR_INVALID, "png_workspace_bytes: N = %ld, served: 1 .. 65535", N);
        return -1;
    }
    return workspace_bytes(N, H, W, channels);
}

int32_t apd_png_encode_ok(const float* src, const uint8_t* dst, const int32_t* sizes, const void* ws, int32_t N, int32_t C, int32_t H,
                          int32_t W, int32_t channels, int64_t slot_bytes, int64_t ws_bytes) {
    return check_png(src, dst, sizes, ws, N, C, H, W, channels, slot_bytes, ws_bytes) == APD_OK ? 1 : 0;
}

int apd_png_encode(const float* src, int32_t N, int32_t C, int32_t H, int32_t W, int32_t channels, uint8_t* dst, int64_t slot_bytes,
                   int32_t* sizes, void* ws, int64_t ws_bytes, void* stream) {
    const int rc = check_png(src, dst, sizes, ws, N, C, H, W, channels, slot_bytes, ws_bytes);
    if (rc != APD_OK) return rc;
    uint8_t* target = static_cast<uint8_t*>(device_address(dst));
    int32_t* target_sizes = static_cast<int32_t*>(device_address(sizes));
    if (!target || !target_sizes)
        return fail(APD_ERR_INVALID, "png_encode: dst / sizes is neither device memory nor pinned host memory mapped for the device");
    Shape sh;
    sh.C = C; sh.H = H; sh.W = W; sh.channels = channels;
    sh.rb = row_bytes(W, channels);
    sh.rows = band_rows(W, channels);
    sh.bands = band_count(H, W, channels);
    sh.stride = chunk_stride(W, channels);
    uint32_t* meta = static_cast<uint32_t*>(ws);
    uint32_t* chunks = meta + (long long)N * sh.bands * META_WORDS;
    hipLaunchKernelGGL(png_band_kernel, dim3((unsigned)sh.bands, (unsigned)N), dim3(THREADS), 0, (hipStream_t)stream, src, meta, chunks, sh);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        hipLaunchKernelGGL(png_finish_kernel, dim3(FINISH_BLOCKS, (unsigned)N), dim3(THREADS), 0, (hipStream_t)stream, meta,
                           reinterpret_cast<const uint8_t*>(chunks), target, target_sizes, sh, (long long)slot_bytes);
        e = hipGetLastError();
    }
    if (e != hipSuccess) {
        snprintf(apd::g_err, sizeof(apd::g_err), "png_encode: launch failed: %s", hipGetErrorString(e));
        return APD_ERR_LAUNCH;
    }
    return APD_OK;
}

}  // extern "C"
