// The JPEG encoder of apd_jpeg_encode on the host: the same functions (animateportrait_amd/csrc/data/jpeg_core.h) driven in
// the order the three kernels drive them -- per block: samples with replicated edges, colour, DCT, quantisation; per MCU row:
// chunks of CHUNK_BLOCKS blocks (bit counts, the scan, the bits OR-ed into a word buffer of the kernel's size, per-"lane"
// runs of bytes stuffed into the segment), padding, RSTm; per frame: prefix sum, header, segments, EOI.
// tools/jpeg_host_check.py builds it with -fsanitize=address,undefined, feeds it u8 images and decodes what it writes.
//
//   jpeg_host_check <cases.bin> <out.bin>
//   cases.bin: per case  int32 H, W, channels, quality;  H W channels bytes
//   out.bin:   per case  int32 size, int32 bound;  size bytes
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../animateportrait_amd/csrc/data/jpeg_core.h"

using namespace apd_jpeg;

namespace {

constexpr int LANES = CHUNK_BLOCKS;

struct Tables {
    uint32_t dc[2][16], ac[2][256];
    uint16_t qt[2][64];
};

void die(const char* what) {
    fprintf(stderr, "%s\n", what);
    exit(2);
}

// one MCU row -> its segment (appended to `body`)
void encode_row(const int16_t* row_coef, int bpr, int channels, int row, int rows, const Tables& tb, size_t stride, std::vector<uint8_t>& body) {
    std::vector<uint8_t> seg(stride, 0xEE);                        // the workspace slot of the kernel, same size
    uint32_t out_pos = 0, carry_bits = 0, carry_byte = 0;
    for (int b0 = 0; b0 < bpr; b0 += LANES) {
        const int count = bpr - b0 < LANES ? bpr - b0 : LANES;
        const bool last = b0 + LANES >= bpr;
        std::vector<uint32_t> first(count + 1, carry_bits);
        for (int t = 0; t < count; ++t) {
            const int b = b0 + t, tab = channels == 3 && b % 3 != 0 ? 1 : 0;
            first[t + 1] = first[t] + encode_block<false>(row_coef + (long)b * 64, dc_prediction(row_coef, b, channels), tb.dc[tab], tb.ac[tab], nullptr);
            if (first[t + 1] - first[t] > (uint32_t)BLOCK_BITS_MAX) die("a block beyond 1664 bits");
        }
        uint32_t tot = first[count];
        const uint32_t words = (tot + 31) / 32 + 2;
        if (words > (uint32_t)bitbuf_words(bpr < LANES ? bpr : LANES)) die("chunk beyond the bit buffer");
        std::vector<uint32_t> bitbuf(words, 0);                    // exactly the words the kernel clears: anything past is an error here
        bitbuf[0] = carry_byte << 24;
        for (int t = 0; t < count; ++t) {
            const int b = b0 + t, tab = channels == 3 && b % 3 != 0 ? 1 : 0;
            BitWriter bw = bit_writer(bitbuf.data(), first[t]);
            const uint32_t n = encode_block<true>(row_coef + (long)b * 64, dc_prediction(row_coef, b, channels), tb.dc[tab], tb.ac[tab], &bw);
            finish_bits(bw);
            if (n != first[t + 1] - first[t]) die("the two passes disagree on a block's bits");
        }
        const uint32_t pad = last ? (8u - (tot & 7u)) & 7u : 0u;
        if (pad) {
            BitWriter bw = bit_writer(bitbuf.data(), tot);
            put_bits(bw, (1u << pad) - 1u, (int)pad);
            finish_bits(bw);
        }
        tot += pad;
        const uint32_t nby = tot >> 3, per = (nby + LANES - 1) / LANES;
        uint32_t ff_before = 0;
        for (int t = 0; t < LANES; ++t) {
            const uint32_t j0 = (uint32_t)t * per < nby ? (uint32_t)t * per : nby, j1 = j0 + per < nby ? j0 + per : nby;
            const uint32_t ff = count_ff(bitbuf.data(), j0, j1);
            if ((size_t)out_pos + j1 + ff_before + ff > (size_t)bpr * 2 * BLOCK_BYTES_MAX) die("segment beyond its bound");
            copy_stuffed(bitbuf.data(), j0, j1, seg.data() + out_pos + j0 + ff_before);
            ff_before += ff;
        }
        out_pos += nby + ff_before;
        carry_bits = tot & 7u;
        carry_byte = carry_bits ? get_byte(bitbuf.data(), nby) & (0xFF00u >> carry_bits) & 255u : 0u;
    }
    if (carry_bits) die("segment ends off a byte boundary");
    if (row + 1 < rows) {
        seg.at(out_pos) = 0xFF;
        seg.at(out_pos + 1) = (uint8_t)(0xD0 + (row & 7));
        out_pos += 2;
    }
    body.insert(body.end(), seg.begin(), seg.begin() + out_pos);
}

std::vector<uint8_t> encode(const uint8_t* pixels, int H, int W, int channels, int quality) {
    const int rows = mcu_rows(H), mcus = mcus_per_row(W), bpr = blocks_per_row(W, channels);
    Tables tb;
    for (int t = 0; t < 4; ++t) build_huffman(t, t < 2 ? tb.dc[t] : tb.ac[t - 2]);
    for (int t = 0; t < 128; ++t) tb.qt[t >> 6][t & 63] = (uint16_t)scaled_quant(t >> 6, t & 63, quality);
    std::vector<int16_t> coef((size_t)rows * bpr * 64);
    for (int row = 0; row < rows; ++row)
        for (int b = 0; b < bpr; ++b) {
            const int comp = b % channels, mcu = b / channels;
            int s[64];
            for (int y = 0; y < 8; ++y)
                for (int x = 0; x < 8; ++x) {
                    const int yy = row * 8 + y < H ? row * 8 + y : H - 1, xx = mcu * 8 + x < W ? mcu * 8 + x : W - 1;
                    const uint8_t* p = pixels + ((size_t)yy * W + xx) * channels;
                    s[y * 8 + x] = (channels == 3 ? component_sample(p[0], p[1], p[2], comp) : p[0]) - 128;
                }
            fdct_quant_block(s, tb.qt[comp ? 1 : 0], coef.data() + ((size_t)row * bpr + b) * 64);
        }
    std::vector<uint8_t> body;
    std::vector<uint32_t> off(rows + 1, 0);
    for (int row = 0; row < rows; ++row) {
        encode_row(coef.data() + (size_t)row * bpr * 64, bpr, channels, row, rows, tb, (size_t)segment_stride(W, channels), body);
        off[row + 1] = (uint32_t)body.size();
    }
    std::vector<uint8_t> file(header_bytes(channels));
    if (write_header(file.data(), W, H, channels, quality) != header_bytes(channels)) die("header_bytes is wrong");
    for (uint32_t k = 0; k < body.size(); ++k) {                   // through segment_of, as the frame kernel looks bytes up
        const int r = segment_of(off.data(), rows, k);
        if (k < off[r] || k >= off[r + 1]) die("segment_of is wrong");
        file.push_back(body[k]);
    }
    file.push_back(0xFF);
    file.push_back(0xD9);
    return file;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) die("usage: jpeg_host_check cases.bin out.bin");
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) die("cannot open the files");
    int32_t hdr[4];
    while (fread(hdr, sizeof(int32_t), 4, in) == 4) {
        const int H = hdr[0], W = hdr[1], channels = hdr[2], quality = hdr[3];
        if (H < 1 || H > MAX_SIDE || W < 1 || W > MAX_SIDE || (channels != 1 && channels != 3) || quality < 1 || quality > 100) die("bad case");
        std::vector<uint8_t> pixels((size_t)H * W * channels);
        if (fread(pixels.data(), 1, pixels.size(), in) != pixels.size()) die("short case");
        const std::vector<uint8_t> file = encode(pixels.data(), H, W, channels, quality);
        const int32_t sizes[2] = {(int32_t)file.size(), (int32_t)frame_bound(H, W, channels)};
        fwrite(sizes, sizeof(int32_t), 2, out);
        fwrite(file.data(), 1, file.size(), out);
    }
    fclose(in);
    fclose(out);
    return 0;
}
