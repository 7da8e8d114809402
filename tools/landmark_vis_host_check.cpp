// The per-pixel rule of apd_landmark_vis (animateportrait_amd/csrc/data/landmark_vis.h) compiled for the host: reads frames
// to draw, finds the primitive on top of every pixel through the same functions the kernel uses, row tile by row tile as the
// kernel does, and writes the pictures as the bytes apd_frames_to_u8 makes of the stored values.
// tools/landmark_vis_host_check.py builds it with -fsanitize=address,undefined, feeds it and compares with
// tests/landmark_vis_reference.py.
//
// input  (binary, native endian), repeated until EOF:  int32 H, W, P, S, radius, thickness;  uint32 disc_rgb, bg_rgb;
//        int32 pts[P][2];  int32 seg[S][2];  uint32 seg_rgb[S]
// output: uint8 picture[H][W][3] per frame
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../animateportrait_amd/csrc/data/landmark_vis.h"

using namespace apd_raster;

// apd_frames_to_u8's byte of a stored value, in unfused float32 (built with -ffp-contract=off)
static unsigned char to_byte(float x) {
    const float v = (x + 1.0f) / 2.0f * 255.0f;
    if (!(v > 0.0f)) return 0;
    if (v >= 255.0f) return 255;
    return (unsigned char)(int)v;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s frames.bin pictures.bin\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { perror("open"); return 2; }
    const int TH = 16;
    int32_t hd[8];
    int frames = 0;
    while (fread(hd, sizeof(int32_t), 8, in) == 8) {
        const int H = hd[0], W = hd[1], P = hd[2], S = hd[3], radius = hd[4], thickness = hd[5];
        const uint32_t disc_rgb = (uint32_t)hd[6], bg_rgb = (uint32_t)hd[7];
        std::vector<int32_t> raw(2 * P), seg(2 * S);
        std::vector<uint32_t> rgb(S);
        if (fread(raw.data(), sizeof(int32_t), raw.size(), in) != raw.size()) return 3;
        if (S && fread(seg.data(), sizeof(int32_t), seg.size(), in) != seg.size()) return 3;
        if (S && fread(rgb.data(), sizeof(uint32_t), rgb.size(), in) != rgb.size()) return 3;
        std::vector<int> pts(2 * P);
        for (int i = 0; i < 2 * P; ++i) pts[i] = clamp_coord(raw[i]);
        const int rad = cap_radius(thickness);
        const CircleRows disc = circle_rows(radius < 0 ? 0 : radius), cap = circle_rows(rad);
        std::vector<Segment> segs(S);
        std::vector<unsigned char> img((size_t)H * W * 3);
        for (int row0 = 0; row0 < H; row0 += TH) {
            const int row1 = row0 + TH < H ? row0 + TH : H;
            for (int s = 0; s < S; ++s) {
                const int a = seg[2 * s], b = seg[2 * s + 1];
                build_segment(segs[s], pts[2 * a], pts[2 * a + 1], pts[2 * b], pts[2 * b + 1], thickness, H, W, row0, row1);
            }
            for (int y = row0; y < row1; ++y)
                for (int x = 0; x < W; ++x) {
                    const int top = vis_top(pts.data(), P, segs.data(), S, disc, radius, cap, rad, x, y);
                    const uint32_t c = top == VIS_BACKGROUND ? bg_rgb : top == VIS_DISC ? disc_rgb : rgb[top];
                    for (int k = 0; k < 3; ++k) img[((size_t)y * W + x) * 3 + k] = to_byte(byte_level(c >> (16 - 8 * k)));
                }
        }
        fwrite(img.data(), 1, img.size(), out);
        ++frames;
    }
    fclose(in);
    fclose(out);
    printf("%d frames\n", frames);
    return 0;
}
