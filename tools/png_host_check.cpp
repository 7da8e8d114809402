// The PNG encoder of apd_png_encode on the host: the same functions (animateportrait_amd/csrc/data/png_deflate.h) driven in
// the order the two kernels drive them -- per band: filter, one encode_segment per "lane", the scan, the trailer, the gather of
// every dword, per-lane CRC parts combined with x^(8 n), the Adler part; per frame: prefix sum, Adler chain, head, chunks, tail.
// tools/png_host_check.py builds it with -fsanitize=address,undefined, feeds it u8 images and decodes what it writes.
//
//   png_host_check <cases.bin> <out.bin>
//   cases.bin: per case  int32 H, W, channels;  H W channels bytes
//   out.bin:   per case  int32 size, int32 bound;  size bytes
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../animateportrait_amd/csrc/data/png_deflate.h"

using namespace apd_png;

namespace {

constexpr int LANES = 256;

struct Image {
    const uint8_t* p;
    int row;
    uint32_t operator()(int y, int x) const { return p[(long)y * row + x]; }
};

// one band -> its IDAT chunk (appended to `chunks`) and its Adler part
void encode_band(const Image& im, int y0, int rows, int rb, int channels, bool first, const uint32_t* crc_tab, std::vector<uint8_t>& chunks,
                 uint32_t* sum, uint32_t* weighted, size_t stride) {
    const int nbytes = rows * rb, nseg = (nbytes + SEGMENT - 1) / SEGMENT;
    std::vector<uint8_t> raw(nbytes);                              // exactly nbytes: a read past the band is an error here
    for (int i = 0; i < nbytes; ++i) raw[i] = (uint8_t)filtered_byte(im, i, rb, channels, y0);
    std::vector<uint32_t> areas((size_t)(nseg + 1) * AREA_WORDS + 1, 0xDEADBEEFu), bit_off(nseg + 2, 0);
    uint32_t a = 0, b = 0;
    for (int s = 0; s < nseg; ++s) {
        bit_off[s + 1] = bit_off[s] + encode_segment(raw.data(), nbytes, s, first, areas.data() + (size_t)s * AREA_WORDS);
        const int start = s * SEGMENT, len = nbytes - start < SEGMENT ? nbytes - start : SEGMENT;
        uint32_t ps, pw;
        adler_part(raw.data() + start, len, &ps, &pw);
        a += ps;
        b = (uint32_t)((b + pw + (uint64_t)(nbytes - start - len) * ps) % ADLER_MOD);
    }
    *sum = a % ADLER_MOD;
    *weighted = b;
    bit_off[nseg + 1] = bit_off[nseg] + encode_trailer(bit_off[nseg], areas.data() + (size_t)nseg * AREA_WORDS);
    const int count = nseg + 1;
    if (bit_off[count] & 7u) { fprintf(stderr, "band ends off a byte boundary\n"); exit(2); }
    const uint32_t len = bit_off[count] >> 3, full = len >> 2;
    if (12 + (size_t)len > (size_t)chunk_bound(nbytes) || (size_t)chunk_bound(nbytes) + 4 > stride) { fprintf(stderr, "chunk beyond its bound\n"); exit(2); }
    std::vector<uint32_t> chunk(stride / 4, 0);                    // the workspace slot of the kernel, same size
    const uint32_t per = (full + LANES - 1) / LANES;
    uint32_t crc = 0;
    for (int t = 0; t < LANES; ++t) {
        const uint32_t j0 = (uint32_t)t * per < full ? (uint32_t)t * per : full, j1 = j0 + per < full ? j0 + per : full;
        uint32_t state = 0;
        for (uint32_t j = j0; j < j1; ++j) {
            const uint32_t w = gather_dword(areas.data(), bit_off.data(), count, j);
            chunk.at(2 + j) = w;
            state = crc_dword(crc_tab, state, w);
        }
        if (j1 > j0) state = crc_mulmod(state, crc_x8n(4 * (full - j1)));
        crc ^= state;
    }
    crc ^= crc_mulmod(CRC_STATE_IDAT, crc_x8n(4 * full));
    const uint32_t last = gather_dword(areas.data(), bit_off.data(), count, full), rest = len & 3u;
    for (uint32_t k = 0; k < rest; ++k) crc = crc_byte(crc_tab, crc, (last >> (8 * k)) & 255u);
    crc = ~crc;
    const uint32_t be = __builtin_bswap32(crc);
    const uint64_t both = (uint64_t)(rest ? last & ((1u << (8 * rest)) - 1) : 0u) | ((uint64_t)be << (8 * rest));
    chunk.at(2 + full) = (uint32_t)both;
    chunk.at(3 + full) = (uint32_t)(both >> 32);
    chunk.at(0) = __builtin_bswap32(len);
    chunk.at(1) = 0x54414449u;
    const uint8_t* bytes = reinterpret_cast<const uint8_t*>(chunk.data());
    chunks.insert(chunks.end(), bytes, bytes + 12 + len);
}

std::vector<uint8_t> encode(const uint8_t* pixels, int H, int W, int channels, const uint32_t* crc_tab) {
    const int rb = row_bytes(W, channels), rows = band_rows(W, channels), bands = band_count(H, W, channels);
    if (bands > MAX_BANDS || rows * rb > BAND_BYTES) { fprintf(stderr, "geometry beyond the kernel's buffers\n"); exit(2); }
    const Image im{pixels, W * channels};
    std::vector<uint8_t> body;
    std::vector<uint32_t> off(bands + 1, 0);
    uint32_t A = 1, B = 0;
    for (int b = 0; b < bands; ++b) {
        const int y0 = b * rows, r = H - y0 < rows ? H - y0 : rows;
        uint32_t s, w;
        encode_band(im, y0, r, rb, channels, b == 0, crc_tab, body, &s, &w, (size_t)chunk_stride(W, channels));
        off[b + 1] = (uint32_t)body.size();
        adler_append(&A, &B, s, w, (uint32_t)(r * rb));
    }
    uint8_t head[HEAD_BYTES], tail[TAIL_BYTES];
    write_head(head, W, H, channels);
    write_tail(tail, (B << 16) | A);
    std::vector<uint8_t> file(head, head + HEAD_BYTES);
    for (uint32_t k = 0; k < body.size(); ++k) {                   // through band_of, as the finishing kernel looks bytes up
        const int b = band_of(off.data(), bands, k);
        if (k < off[b] || k >= off[b + 1]) { fprintf(stderr, "band_of(%u) = %d is wrong\n", k, b); exit(2); }
        file.push_back(body[k]);
    }
    file.insert(file.end(), tail, tail + TAIL_BYTES);
    return file;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: png_host_check cases.bin out.bin\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    uint32_t crc_tab[256];
    for (uint32_t i = 0; i < 256; ++i) crc_tab[i] = crc_table_entry(i);
    int32_t hdr[3];
    while (fread(hdr, sizeof(int32_t), 3, in) == 3) {
        const int H = hdr[0], W = hdr[1], channels = hdr[2];
        if (H < 1 || H > MAX_SIDE || W < 1 || W > MAX_SIDE || (channels != 1 && channels != 3)) { fprintf(stderr, "bad case\n"); return 2; }
        std::vector<uint8_t> pixels((size_t)H * W * channels);
        if (fread(pixels.data(), 1, pixels.size(), in) != pixels.size()) { fprintf(stderr, "short case\n"); return 2; }
        const std::vector<uint8_t> file = encode(pixels.data(), H, W, channels, crc_tab);
        const int32_t sizes[2] = {(int32_t)file.size(), (int32_t)frame_bound(H, W, channels)};
        fwrite(sizes, sizeof(int32_t), 2, out);
        fwrite(file.data(), 1, file.size(), out);
    }
    fclose(in);
    fclose(out);
    return 0;
}
