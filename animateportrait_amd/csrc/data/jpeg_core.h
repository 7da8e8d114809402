// The pieces of apd_jpeg_encode as functions over plain pointers (host and device: a stand-alone host program runs the same
// text under sanitizers, tools/jpeg_host_check.cpp): the tables of ITU T.81 Annex K, the IJG quality scaling, the JFIF colour
// conversion, the forward DCT with quantisation, the per-block Huffman symbol generator over a most-significant-bit-first
// bit writer, 0xFF stuffing, and the header writer.  Integer arithmetic only: the host build and the device give equal bytes.
//
// Layout of one frame (include/animateportrait_data.h): SOI, JFIF APP0, DQT, SOF0, DHT (the four Annex K.3 tables), DRI,
// SOS, the scan, EOI.  The restart interval is one MCU row, so a row is a byte-aligned segment with its own DC prediction:
// it is encoded without knowing any other row.  Within a row the blocks are taken CHUNK_BLOCKS at a time: every block's bit
// count is found first (encode_block<false>), an exclusive scan places the strings, every block then writes its bits into
// one shared word buffer (encode_block<true>; two blocks may share a word, hence or_word), and the chunk's whole bytes are
// copied out with every 0xFF followed by 0x00; the bits of the last partial byte are carried into the next chunk.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define APD_HD __host__ __device__ inline
#else
#define APD_HD inline
#endif

namespace apd_jpeg {

constexpr int MAX_SIDE = 2048;
constexpr int CHUNK_BLOCKS = 256;        // blocks placed by one scan: the workgroup size of the segment kernel
constexpr int BLOCK_BITS_MAX = 64 * 26;  // a DC symbol is at most 11 + 11 bits, an AC symbol 16 + 10
constexpr int BLOCK_BYTES_MAX = BLOCK_BITS_MAX / 8;       // 208 before stuffing, twice that after
constexpr int MAX_MCU_ROWS = MAX_SIDE / 8;

// ---- geometry shared by the launcher, the kernels and the host check
APD_HD int mcus_per_row(int W) { return (W + 7) / 8; }
APD_HD int mcu_rows(int H) { return (H + 7) / 8; }
APD_HD int blocks_per_row(int W, int channels) { return mcus_per_row(W) * channels; }
APD_HD int header_bytes(int channels) {
    // SOI 2, APP0 18, DQT 4 + 65 per table, SOF0 10 + 3 per component, DHT 4 + 2 (17 + 12) + 2 (17 + 162), DRI 6,
    // SOS 8 + 2 per component
    return channels == 3 ? 2 + 18 + 134 + 19 + 420 + 6 + 14 : 2 + 18 + 69 + 13 + 420 + 6 + 10;
}
// bytes of a segment at most, its RSTm marker included: bits <= blocks * 1664, so ceil(bits / 8) <= blocks * 208 bytes (the
// 1-bit padding fills the last of them), each of which stuffing may double
APD_HD int64_t segment_bound(int W, int channels) { return (int64_t)blocks_per_row(W, channels) * (2 * BLOCK_BYTES_MAX) + 2; }
APD_HD int64_t segment_stride(int W, int channels) { return (segment_bound(W, channels) + 3) / 4 * 4; }
// header + every segment at its bound + EOI (the last segment carries no RSTm: two bytes to spare), in whole dwords
APD_HD int64_t frame_bound(int H, int W, int channels) {
    return (header_bytes(channels) + (int64_t)mcu_rows(H) * segment_bound(W, channels) + 2 + 3) / 4 * 4;
}
// workspace: zigzag int16 coefficients of every block, then one uint32 size per segment, then the segments at their stride
APD_HD int64_t coef_bytes(int N, int H, int W, int channels) { return (int64_t)N * mcu_rows(H) * blocks_per_row(W, channels) * 128; }
APD_HD int64_t workspace_bytes(int N, int H, int W, int channels) {
    return coef_bytes(N, H, W, channels) + (int64_t)N * mcu_rows(H) * (4 + segment_stride(W, channels));
}
// words of the bit buffer a chunk of `blocks` blocks needs: up to 7 carried bits, the strings, one word of slack for the
// writer's last flush and one the carry read may touch
APD_HD int bitbuf_words(int blocks) { return (7 + blocks * BLOCK_BITS_MAX + 31) / 32 + 2; }

// ---- tables.  Kept inside functions: a local constexpr array is usable from host and device code alike.
// natural index of zigzag position k
APD_HD int zigzag_nat(int k) {
    constexpr uint8_t t[64] = {
        0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5,
        12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
        35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
        58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return t[k];
}
// zigzag position of natural index i
APD_HD int zigzag_pos(int i) {
    constexpr uint8_t t[64] = {
        0, 1, 5, 6, 14, 15, 27, 28, 2, 4, 7, 13, 16, 26, 29, 42,
        3, 8, 12, 17, 25, 30, 41, 43, 9, 11, 18, 24, 31, 40, 44, 53,
        10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60,
        21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};
    return t[i];
}
// Annex K.1 (which = 0, luminance) and K.2 (which = 1, chrominance), natural order
APD_HD int base_quant(int which, int i) {
    constexpr uint8_t lum[64] = {
        16, 11, 10, 16, 24, 40, 51, 61,
        12, 12, 14, 19, 26, 58, 60, 55,
        14, 13, 16, 24, 40, 57, 69, 56,
        14, 17, 22, 29, 51, 87, 80, 62,
        18, 22, 37, 56, 68, 109, 103, 77,
        24, 35, 55, 64, 81, 104, 113, 92,
        49, 64, 78, 87, 103, 121, 120, 101,
        72, 92, 95, 98, 112, 100, 103, 99};
    constexpr uint8_t chr[64] = {
        17, 18, 24, 47, 99, 99, 99, 99,
        18, 21, 26, 66, 99, 99, 99, 99,
        24, 26, 56, 99, 99, 99, 99, 99,
        47, 66, 99, 99, 99, 99, 99, 99,
        99, 99, 99, 99, 99, 99, 99, 99,
        99, 99, 99, 99, 99, 99, 99, 99,
        99, 99, 99, 99, 99, 99, 99, 99,
        99, 99, 99, 99, 99, 99, 99, 99};
    return which ? chr[i] : lum[i];
}
// the IJG rule: s = q < 50 ? 5000 / q : 200 - 2 q, t = clamp((base s + 50) / 100, 1, 255)
APD_HD int scaled_quant(int which, int i, int quality) {
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    const int t = (base_quant(which, i) * s + 50) / 100;
    return t < 1 ? 1 : t > 255 ? 255 : t;
}
// Annex K.3 as the bytes of a DHT table body: 16 counts, then the symbols.  which: 0 DC luminance, 1 DC chrominance,
// 2 AC luminance, 3 AC chrominance
APD_HD int dht_symbols(int which) { return which < 2 ? 12 : 162; }
APD_HD int dht_byte(int which, int i) {
    constexpr uint8_t dc0[28] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
    constexpr uint8_t dc1[28] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
    constexpr uint8_t ac0[178] = {
        0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125,
        0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07,
        0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0,
        0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
        0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49,
        0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
        0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
        0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7,
        0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5,
        0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
        0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
        0xf9, 0xfa};
    constexpr uint8_t ac1[178] = {
        0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119,
        0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71,
        0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0,
        0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
        0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
        0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
        0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
        0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
        0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
        0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
        0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
        0xf9, 0xfa};
    return which == 0 ? dc0[i] : which == 1 ? dc1[i] : which == 2 ? ac0[i] : ac1[i];
}
// The canonical codes of table `which` into tab[symbol] = code | length << 16 (0 for a symbol the table lacks).  tab has
// 16 entries for a DC table, 256 for an AC table.
APD_HD void build_huffman(int which, uint32_t* tab) {
    const int size = which < 2 ? 16 : 256;
    for (int i = 0; i < size; ++i) tab[i] = 0;
    uint32_t code = 0;
    int k = 16;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < dht_byte(which, len - 1); ++i) tab[dht_byte(which, k++)] = code++ | ((uint32_t)len << 16);
        code <<= 1;
    }
}

// ---- colour.  JFIF: Y = 0.299 R + 0.587 G + 0.114 B, Cb = -0.16874 R - 0.33126 G + 0.5 B + 128, Cr = 0.5 R - 0.41869 G
// - 0.08131 B + 128 at 16 fractional bits; Y is rounded half up (+ 2^15), Cb and Cr get + 2^15 - 1, so that grey gives 128
// exactly and 255 is never passed.  Every sum is non-negative, so the shift is a plain division.
APD_HD int component_sample(int r, int g, int b, int comp) {
    if (comp == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    if (comp == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// ---- the forward DCT.  c(u, x) = C(u) / 2 cos((2 x + 1) u pi / 16), C(0) = 1 / sqrt 2, rounded to 20 fractional bits.
APD_HD int dct_c20(int u, int x) {
    constexpr int32_t t[64] = {
        370728, 370728, 370728, 370728, 370728, 370728, 370728, 370728,
        514214, 435930, 291279, 102284, -102284, -291279, -435930, -514214,
        484379, 200636, -200636, -484379, -484379, -200636, 200636, 484379,
        435930, -102284, -514214, -291279, 291279, 514214, 102284, -435930,
        370728, -370728, -370728, 370728, 370728, -370728, -370728, 370728,
        291279, -514214, 102284, 435930, -435930, -102284, 514214, -291279,
        200636, -484379, 484379, -200636, -200636, 484379, -484379, 200636,
        102284, -291279, 435930, -514214, 514214, -435930, 291279, -102284};
    return t[u * 8 + x];
}
constexpr int COEF_FRAC = 20;            // fractional bits of a coefficient before quantisation

// s: the 64 level-shifted samples (-128 .. 127), row major; qt: the 64 scaled quantisers in natural order; zz: the quantised
// coefficients in zigzag order.
// Row pass: int32 sum c20 s, kept whole: 20 fractional bits, |sum| <= 128 * 2965824 < 2^29.
// Column pass: int64 sum c20 tmp (40 fractional bits, |sum| < 2^51), rounded half up to COEF_FRAC bits: an int32 below 2^31.
// The constants' error (2^-21 each) moves a coefficient by less than 0.002; 13-bit constants moved the high-contrast blocks
// of a line drawing by up to 0.1, which cost 1 dB against libjpeg at quality 100.
// The DC term is not taken from the passes: it is the sum of the samples / 8 exactly (sum << 17), so a flat block that lies
// on a rounding tie -- white, 1016 / 16 at quality 50 -- rounds as the exact value does.
// Quantisation: sign(v) * ((|v| + q 2^(COEF_FRAC - 1)) / (q 2^COEF_FRAC)): half goes away from zero; |v| + q 2^19 < 2^31.  AC
// results are clamped to +-1023 (10 magnitude bits, the most a baseline code carries); a DC result is within +-1024.
APD_HD void fdct_quant_block(const int* s, const uint16_t* qt, int16_t* zz) {
    int tmp[64];
    int sum = 0;
#pragma unroll
    for (int y = 0; y < 8; ++y) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            int acc = 0;
#pragma unroll
            for (int x = 0; x < 8; ++x) acc += dct_c20(u, x) * s[y * 8 + x];
            tmp[y * 8 + u] = acc;
        }
#pragma unroll
        for (int x = 0; x < 8; ++x) sum += s[y * 8 + x];
    }
#pragma unroll
    for (int v = 0; v < 8; ++v) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            int64_t wide = 0;
#pragma unroll
            for (int y = 0; y < 8; ++y) wide += (int64_t)dct_c20(v, y) * tmp[y * 8 + u];
            const int acc = v + u == 0 ? sum * (1 << (COEF_FRAC - 3)) : (int)((wide + (1 << 19)) >> 20);
            const int q = qt[v * 8 + u];
            const int mag = ((acc < 0 ? -acc : acc) + (q << (COEF_FRAC - 1))) / (q << COEF_FRAC);
            int r = acc < 0 ? -mag : mag;
            if (v + u != 0) r = r > 1023 ? 1023 : r < -1023 ? -1023 : r;
            zz[zigzag_pos(v * 8 + u)] = (int16_t)r;
        }
    }
}

// ---- bits.  JPEG packs from the most significant bit: bit p of the stream is bit 31 - (p & 31) of word p >> 5, and byte k
// of the stream is get_byte(buf, k).
APD_HD void or_word(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (v) atomicOr(p, v);               // an LDS word may be shared with the neighbouring blocks' writers
#else
    *p |= v;
#endif
}
APD_HD uint32_t get_byte(const uint32_t* buf, uint32_t k) { return (buf[k >> 2] >> (24 - 8 * (k & 3u))) & 255u; }

struct BitWriter {
    uint32_t* buf;
    uint32_t word;
    uint64_t acc;      // pending bits, from bit 63 down
    int n;             // how many (below 32 between calls); the first p & 31 of them are the neighbour's: zeros here
};
APD_HD BitWriter bit_writer(uint32_t* buf, uint32_t p) { return BitWriter{buf, p >> 5, 0, (int)(p & 31u)}; }
APD_HD void put_bits(BitWriter& b, uint32_t v, int nb) {          // 1 <= nb <= 26, v < 2^nb
    b.acc |= (uint64_t)v << (64 - b.n - nb);
    b.n += nb;
    if (b.n >= 32) {
        or_word(b.buf + b.word++, (uint32_t)(b.acc >> 32));
        b.acc <<= 32;
        b.n -= 32;
    }
}
APD_HD void finish_bits(BitWriter& b) {
    if (b.n > 0) or_word(b.buf + b.word, (uint32_t)(b.acc >> 32));
}

APD_HD int magnitude_bits(int v) {
    int a = v < 0 ? -v : v, n = 0;
    while (a) { ++n; a >>= 1; }
    return n;
}
// One block: the DC difference against `pred`, the AC run / size symbols with ZRL and EOB.  Returns the bit count; WRITE puts
// the bits through `b`.  dc: 16 entries, ac: 256 (build_huffman).
template <bool WRITE>
APD_HD uint32_t encode_block(const int16_t* zz, int pred, const uint32_t* dc, const uint32_t* ac, BitWriter* b) {
    uint32_t total = 0;
    auto emit = [&](uint32_t entry, int value, int size) {
        const int len = (int)(entry >> 16);
        total += (uint32_t)(len + size);
        if (WRITE) {
            const uint32_t extra = (uint32_t)(value < 0 ? value - 1 : value) & ((1u << size) - 1u);
            put_bits(*b, ((entry & 0xFFFFu) << size) | extra, len + size);
        }
    };
    const int diff = zz[0] - pred;
    const int dsize = magnitude_bits(diff);
    emit(dc[dsize], diff, dsize);
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int v = zz[k];
        if (v == 0) { ++run; continue; }
        while (run > 15) { emit(ac[0xF0], 0, 0); run -= 16; }
        const int size = magnitude_bits(v);
        emit(ac[(run << 4) | size], v, size);
        run = 0;
    }
    if (run > 0) emit(ac[0x00], 0, 0);
    return total;
}
// the prediction of block b of a row (blocks in MCU order, `channels` per MCU): the DC of the same component one MCU back
APD_HD int dc_prediction(const int16_t* row_coef, int b, int channels) { return b >= channels ? row_coef[(long)(b - channels) * 64] : 0; }

// ---- stuffing: bytes j0 .. j1 of the bit buffer, every 0xFF followed by 0x00
APD_HD uint32_t count_ff(const uint32_t* buf, uint32_t j0, uint32_t j1) {
    uint32_t n = 0;
    for (uint32_t j = j0; j < j1; ++j) n += get_byte(buf, j) == 255u;
    return n;
}
APD_HD void copy_stuffed(const uint32_t* buf, uint32_t j0, uint32_t j1, uint8_t* dst) {
    for (uint32_t j = j0; j < j1; ++j) {
        const uint32_t v = get_byte(buf, j);
        *dst++ = (uint8_t)v;
        if (v == 255u) *dst++ = 0;
    }
}

// ---- the header: everything in front of the scan.  Returns header_bytes(channels).
APD_HD int write_header(uint8_t* h, int W, int H, int channels, int quality) {
    int at = 0;
    auto u8 = [&](int v) { h[at++] = (uint8_t)v; };
    auto u16 = [&](int v) { u8(v >> 8); u8(v & 255); };
    u16(0xFFD8);
    u16(0xFFE0); u16(16);
    u8('J'); u8('F'); u8('I'); u8('F'); u8(0);
    u16(0x0101); u8(0); u16(1); u16(1); u8(0); u8(0);               // 1.01, no units, 1 : 1, no thumbnail
    const int tables = channels == 3 ? 2 : 1;
    u16(0xFFDB); u16(2 + 65 * tables);
    for (int t = 0; t < tables; ++t) {
        u8(t);                                                         // 8-bit entries, table t
        for (int k = 0; k < 64; ++k) u8(scaled_quant(t, zigzag_nat(k), quality));
    }
    u16(0xFFC0); u16(8 + 3 * channels);
    u8(8); u16(H); u16(W); u8(channels);
    for (int c = 0; c < channels; ++c) { u8(c + 1); u8(0x11); u8(c ? 1 : 0); }
    u16(0xFFC4); u16(2 + 2 * (17 + 12) + 2 * (17 + 162));
    for (int t = 0; t < 4; ++t) {
        const int which = (t & 1) * 2 + (t >> 1);                     // DC 0, AC 0, DC 1, AC 1
        u8(((which >> 1) << 4) | (which & 1));
        for (int i = 0; i < 16 + dht_symbols(which); ++i) u8(dht_byte(which, i));
    }
    u16(0xFFDD); u16(4); u16(mcus_per_row(W));
    u16(0xFFDA); u16(6 + 2 * channels);
    u8(channels);
    for (int c = 0; c < channels; ++c) { u8(c + 1); u8(c ? 0x11 : 0x00); }
    u8(0); u8(63); u8(0);
    return at;
}

// The segment whose bytes hold byte k of the scan: off[r] <= k < off[r + 1], off[0] = 0, off[count] = all bytes
APD_HD int segment_of(const uint32_t* off, int count, uint32_t k) {
    int a = 0, z = count - 1;
    while (a < z) {
        const int m = (a + z + 1) >> 1;
        if (off[m] <= k) a = m; else z = m - 1;
    }
    return a;
}

}  // namespace apd_jpeg
