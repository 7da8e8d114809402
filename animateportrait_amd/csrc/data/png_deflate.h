// The pieces of apd_png_encode as functions over plain pointers (host and device: a stand-alone host program runs the same
// text under sanitizers, tools/png_host_check.cpp): the PNG row filter, the fixed-Huffman bit packer with its distance-1
// match finder, the gather that turns per-segment bit strings into output dwords, CRC-32 with the x^(8n) combination, and
// Adler-32 as (sum, weighted sum, length) parts that concatenate.
//
// Layout of one frame (include/animateportrait_data.h): signature, IHDR, one IDAT chunk per band of R rows, a last 9-byte
// IDAT chunk (the final empty stored block and the Adler-32), IEND.  A band is one fixed-Huffman block followed by an empty
// stored block, so every band starts and ends on a byte boundary and is encoded without knowing any other band.  Within a
// band every SEGMENT bytes are one lane's work: the lane writes its bit string into an area of its own, an exclusive scan
// of the bit counts places the strings, and output dword j is then put together by whoever asks for it (gather_dword) --
// no two writers ever share a dword.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define APD_HD __host__ __device__ inline
#else
#define APD_HD inline
#endif

namespace apd_png {

constexpr int MAX_SIDE = 2048;
constexpr int BAND_BYTES = 16384;       // filtered bytes of a band at most (its LDS staging buffer)
constexpr int MAX_ROWS = 16;            // rows per band at most
constexpr int SEGMENT = 132;            // bytes per lane: 33 dwords, an odd stride, so the lanes' byte reads spread over the LDS banks
constexpr int MAX_SEGMENTS = (BAND_BYTES + SEGMENT - 1) / SEGMENT;       // 125
constexpr int PREFIX_BITS = 19;         // zlib header (first band only) + block header, in front of segment 0
constexpr int AREA_WORDS = 39;          // >= ceil((9 SEGMENT + PREFIX_BITS) / 32) + 1 spare word gather_dword may read; odd
constexpr int TRAILER_BITS_MAX = 49;    // end of block (7) + stored header (3) + padding (<= 7) + LEN / NLEN (32)
constexpr int MAX_BANDS = 1024;         // 2048 rows in bands of >= 2 rows (row bytes <= 6145)
constexpr int HEAD_BYTES = 33;          // signature + IHDR chunk
constexpr int TAIL_BYTES = 33;          // the last IDAT chunk (12 + 9) + IEND (12)
static_assert(AREA_WORDS * 32 >= 9 * SEGMENT + PREFIX_BITS + 32 && (AREA_WORDS & 1) == 1, "area too small");
static_assert(MAX_SEGMENTS + 1 <= 128, "segments + trailer must fit the scan");

// ---- geometry shared by the launcher, the kernels and the host check
APD_HD int row_bytes(int W, int channels) { return W * channels + 1; }
APD_HD int band_rows(int W, int channels) {
    const int r = BAND_BYTES / row_bytes(W, channels);           // >= 2: row bytes <= 6145
    return r > MAX_ROWS ? MAX_ROWS : r;
}
APD_HD int band_count(int H, int W, int channels) {
    const int r = band_rows(W, channels);
    return (H + r - 1) / r;
}
// bytes of a band's IDAT chunk at most: every byte a 9-bit literal
APD_HD int64_t chunk_bound(int64_t band_bytes) { return 12 + (9 * band_bytes + PREFIX_BITS + TRAILER_BITS_MAX + 7) / 8; }
// the stride of a band's chunk in the workspace: the bound, in whole dwords, plus one dword the last store may pad into
APD_HD int64_t chunk_stride(int W, int channels) {
    return ((chunk_bound((int64_t)band_rows(W, channels) * row_bytes(W, channels)) + 3) / 4 + 1) * 4;
}
APD_HD int64_t frame_bound(int H, int W, int channels) {
    const int r = band_rows(W, channels), rb = row_bytes(W, channels), full = H / r, rest = H - full * r;
    int64_t b = HEAD_BYTES + TAIL_BYTES + (int64_t)full * chunk_bound((int64_t)r * rb);
    if (rest) b += chunk_bound((int64_t)rest * rb);
    return (b + 3) / 4 * 4;
}
constexpr int META_WORDS = 4;           // per band in the workspace: chunk bytes, Adler sum, Adler weighted sum, filtered bytes
APD_HD int64_t workspace_bytes(int N, int H, int W, int channels) {
    return (int64_t)N * band_count(H, W, channels) * (META_WORDS * 4 + chunk_stride(W, channels));
}

// ---- the row filter.  px(y, x) is byte x of image row y (x over W * channels).  Byte i of the band that starts at row y0:
// a filter-type byte in front of every row; the band's first row is filtered Sub (so it needs no row above), the others Up
// (the row above comes from the image, not from the band before: bands stay independent).
template <class Px>
APD_HD uint32_t filtered_byte(Px px, int i, int rb, int channels, int y0) {
    const int r = i / rb, c = i - r * rb;
    if (c == 0) return r == 0 ? 1u : 2u;
    const int x = c - 1, y = y0 + r;
    const uint32_t v = px(y, x);
    const uint32_t ref = r == 0 ? (x >= channels ? px(y, x - channels) : 0u) : px(y - 1, x);
    return (v - ref) & 255u;
}

// ---- bits.  Deflate packs from the least significant bit; Huffman codes go in most significant bit first.
struct BitWriter {
    uint32_t* w;
    uint64_t acc;
    int n;
    uint32_t total;
};
APD_HD BitWriter bit_writer(uint32_t* area) { return BitWriter{area, 0, 0, 0}; }
APD_HD void put_bits(BitWriter& b, uint32_t v, int nb) {         // nb <= 32
    b.acc |= (uint64_t)v << b.n;
    b.n += nb;
    b.total += (uint32_t)nb;
    if (b.n >= 32) {
        *b.w++ = (uint32_t)b.acc;
        b.acc >>= 32;
        b.n -= 32;
    }
}
APD_HD uint32_t finish_bits(BitWriter& b) {
    if (b.n > 0) *b.w++ = (uint32_t)b.acc;
    return b.total;
}
APD_HD uint32_t reverse_bits(uint32_t v, int nb) {
    uint32_t r = 0;
    for (int i = 0; i < nb; ++i) r |= ((v >> i) & 1u) << (nb - 1 - i);
    return r;
}
// fixed Huffman code of literal / length symbol s (0..287), reversed for put_bits; returns its length
APD_HD int fixed_code(uint32_t s, uint32_t* code) {
    if (s < 144) { *code = reverse_bits(0x30 + s, 8); return 8; }
    if (s < 256) { *code = reverse_bits(0x190 + (s - 144), 9); return 9; }
    if (s < 280) { *code = reverse_bits(s - 256, 7); return 7; }
    *code = reverse_bits(0xC0 + (s - 280), 8);
    return 8;
}
APD_HD void put_literal(BitWriter& b, uint32_t v) {
    uint32_t code;
    const int nb = fixed_code(v, &code);
    put_bits(b, code, nb);
}
// a match of `len` (3..258) bytes at distance 1: length symbol, its extra bits, the 5-bit distance code 0
APD_HD void put_run(BitWriter& b, int len) {
    uint32_t sym, extra = 0;
    int eb = 0;
    const int l = len - 3;
    if (len == 258) sym = 285;
    else if (l < 8) sym = 257 + l;
    else {
        int lg = 3;
        while ((l >> (lg + 1)) != 0) ++lg;
        eb = lg - 2;
        sym = 257 + 4 * eb + 4 + ((l >> eb) & 3);
        extra = l & ((1u << eb) - 1);
    }
    uint32_t code;
    const int nb = fixed_code(sym, &code);
    put_bits(b, code | (extra << nb), nb + eb + 5);               // the distance code's five zero bits ride on top
}

// Segment `seg` of a band of `nbytes` filtered bytes (raw) into `area` (AREA_WORDS): returns its bit count.  Matches are runs
// at distance 1; the byte before the segment may start one, the segment's end ends it.  Segment 0 carries the zlib header
// (first band of a frame only) and the block header BFINAL = 0, BTYPE = 01.
APD_HD uint32_t encode_segment(const uint8_t* raw, int nbytes, int seg, bool first_band, uint32_t* area) {
    BitWriter b = bit_writer(area);
    if (seg == 0) {
        if (first_band) put_bits(b, 0x0178u, 16);                 // 78 01: deflate, 32K window, no preset, fastest
        put_bits(b, 2u, 3);
    }
    const int start = seg * SEGMENT, end = start + SEGMENT < nbytes ? start + SEGMENT : nbytes;
    int i = start;
    while (i < end) {
        const uint32_t v = raw[i];
        if (i > 0 && raw[i - 1] == v) {
            int len = 1;
            while (i + len < end && len < 258 && raw[i + len] == v) ++len;
            if (len >= 3) {
                put_run(b, len);
                i += len;
                continue;
            }
        }
        put_literal(b, v);
        ++i;
    }
    return finish_bits(b);
}

// What follows the last segment, given the bits before it: end of block, an empty stored block padded to a byte boundary
// (BFINAL = 0, BTYPE = 00, LEN = 0, NLEN = FFFF).  The band's bit count becomes a multiple of 8.
APD_HD uint32_t encode_trailer(uint32_t bits_before, uint32_t* area) {
    BitWriter b = bit_writer(area);
    put_bits(b, 0u, 7 + 3);
    const int pad = (int)((8 - ((bits_before + 10) & 7)) & 7);
    put_bits(b, 0u, pad);
    put_bits(b, 0xFFFF0000u, 32);
    return finish_bits(b);
}

// Output dword j of a band: bits 32 j .. 32 j + 31 of the concatenated strings.  areas + s * AREA_WORDS holds string s,
// bit_off[s] its first bit (bit_off[count] = all bits).  Bits past the end are zero.
APD_HD uint32_t gather_dword(const uint32_t* areas, const uint32_t* bit_off, int count, uint32_t j) {
    const uint32_t lo = 32u * j, hi = lo + 32u;
    if (lo >= bit_off[count]) return 0u;
    int a = 0, z = count - 1;                                     // the last string that starts at or before lo
    while (a < z) {
        const int m = (a + z + 1) >> 1;
        if (bit_off[m] <= lo) a = m; else z = m - 1;
    }
    uint32_t out = 0;
    for (int s = a; s < count && bit_off[s] < hi; ++s) {
        const uint32_t from = bit_off[s] > lo ? bit_off[s] : lo, to = bit_off[s + 1] < hi ? bit_off[s + 1] : hi;
        if (to <= from) continue;
        const uint32_t p = from - bit_off[s], n = to - from;      // n in 1..32
        const uint32_t* w = areas + (long)s * AREA_WORDS + (p >> 5);
        const uint64_t two = (uint64_t)w[0] | ((uint64_t)w[1] << 32);
        uint32_t bits = (uint32_t)(two >> (p & 31));
        if (n < 32) bits &= (1u << n) - 1;
        out |= bits << (from - lo);
    }
    return out;
}

// ---- CRC-32 (reflected, polynomial EDB88320).  `state` is the raw register: crc32(M) = ~crc_bytes(~0, M).
constexpr uint32_t CRC_POLY = 0xEDB88320u;
APD_HD uint32_t crc_table_entry(uint32_t i) {
    for (int k = 0; k < 8; ++k) i = (i & 1u) ? (i >> 1) ^ CRC_POLY : i >> 1;
    return i;
}
APD_HD uint32_t crc_byte(const uint32_t* table, uint32_t state, uint32_t byte) { return table[(state ^ byte) & 255u] ^ (state >> 8); }
APD_HD uint32_t crc_dword(const uint32_t* table, uint32_t state, uint32_t w) {       // four bytes, lowest first
    state = crc_byte(table, state, w & 255u);
    state = crc_byte(table, state, (w >> 8) & 255u);
    state = crc_byte(table, state, (w >> 16) & 255u);
    return crc_byte(table, state, w >> 24);
}
APD_HD uint32_t crc_byte_slow(uint32_t state, uint32_t byte) { return crc_table_entry((state ^ byte) & 255u) ^ (state >> 8); }
// a(x) b(x) mod P in the reflected representation (bit 31 is x^0)
APD_HD uint32_t crc_mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t m = 1u << 31; m != 0; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ CRC_POLY : b >> 1;
    }
    return p;
}
// x^(8 n) mod P.  The register after bytes A then B, started at s: crc(s, A B) = crc(s, A) x^(8 |B|) + crc(0, B).
APD_HD uint32_t crc_x8n(uint32_t n) {
    uint32_t r = 1u << 31, base = 1u << 23;                       // x^0, x^8
    while (n) {
        if (n & 1u) r = crc_mulmod(r, base);
        base = crc_mulmod(base, base);
        n >>= 1;
    }
    return r;
}

// ---- Adler-32 in parts.  A run of bytes d_0 .. d_{n-1} is (sum d_i, sum (n - i) d_i, n), both mod 65521; a part appended to
// a running (A, B) gives B += n A + weighted, A += sum.
constexpr uint32_t ADLER_MOD = 65521u;
APD_HD void adler_part(const uint8_t* d, int n, uint32_t* sum, uint32_t* weighted) {      // n <= 4096: no overflow before the mod
    uint32_t a = 0, b = 0;
    for (int i = 0; i < n; ++i) {
        a += d[i];
        b += a;
    }
    *sum = a % ADLER_MOD;
    *weighted = b % ADLER_MOD;
}
APD_HD void adler_append(uint32_t* A, uint32_t* B, uint32_t sum, uint32_t weighted, uint32_t n) {
    *B = (uint32_t)((*B + (uint64_t)(n % ADLER_MOD) * *A + weighted) % ADLER_MOD);
    *A = (*A + sum) % ADLER_MOD;
}

// ---- the fixed ends of a file
APD_HD void put_be32(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v;
}
APD_HD uint32_t crc_slow(const uint8_t* p, int n) {
    uint32_t s = ~0u;
    for (int i = 0; i < n; ++i) s = crc_byte_slow(s, p[i]);
    return ~s;
}
// signature + IHDR: 8-bit samples, colour type 2 (channels 3) or 0 (channels 1), no interlace
APD_HD void write_head(uint8_t* h, int W, int H, int channels) {
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    for (int i = 0; i < 8; ++i) h[i] = sig[i];
    put_be32(h + 8, 13);
    h[12] = 'I'; h[13] = 'H'; h[14] = 'D'; h[15] = 'R';
    put_be32(h + 16, (uint32_t)W);
    put_be32(h + 20, (uint32_t)H);
    h[24] = 8; h[25] = channels == 3 ? 2 : 0; h[26] = 0; h[27] = 0; h[28] = 0;
    put_be32(h + 29, crc_slow(h + 12, 17));
}
// the last IDAT chunk (BFINAL = 1 empty stored block, Adler-32 of all filtered bytes) + IEND
APD_HD void write_tail(uint8_t* t, uint32_t adler) {
    put_be32(t, 9);
    t[4] = 'I'; t[5] = 'D'; t[6] = 'A'; t[7] = 'T';
    t[8] = 1; t[9] = 0; t[10] = 0; t[11] = 0xFF; t[12] = 0xFF;
    put_be32(t + 13, adler);
    put_be32(t + 17, crc_slow(t + 4, 13));
    put_be32(t + 21, 0);
    t[25] = 'I'; t[26] = 'E'; t[27] = 'N'; t[28] = 'D';
    put_be32(t + 29, 0xAE426082u);
}
constexpr uint32_t CRC_STATE_IDAT = 0xCA50F9E1u;   // the register after "IDAT": ~crc32("IDAT") = ~0x35AF061E

// The band whose chunk holds byte k of the chunk area: off[b] <= k < off[b + 1], off[0] = 0, off[count] = all bytes
APD_HD int band_of(const uint32_t* off, int count, uint32_t k) {
    int a = 0, z = count - 1;
    while (a < z) {
        const int m = (a + z + 1) >> 1;
        if (off[m] <= k) a = m; else z = m - 1;
    }
    return a;
}

}  // namespace apd_png
