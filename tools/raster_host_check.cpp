// The rasteriser of apd_landmark_map and ap_lip_line_mask (animateportrait_amd/csrc/cv_raster.h) compiled for the host: reads
// cases, evaluates every pixel through the same predicates the kernels use, row tile by row tile as the kernels do, and
// writes the maps.  tools/raster_host_check.py builds it with -fsanitize=address,undefined, feeds it and compares with
// oracle/cv_raster.
//
// input  (binary, native endian), repeated until EOF:  int32 H, W, P, S, radius, thickness, op;  float32 lm[P][2];  int32 seg[S][2]
//         op 0 / 1: draw2 (discs / discs and lines, rounded points);  op 2: the lip mask (lines only, truncated points)
// output: uint8 map[H][W] per case (1 on a mark)
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../animateportrait_amd/csrc/cv_raster.h"

using namespace apd_raster;

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s cases.bin maps.bin\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { perror("open"); return 2; }
    const int TH = 16;
    int32_t hd[7];
    int cases = 0;
    while (fread(hd, sizeof(int32_t), 7, in) == 7) {
        const int H = hd[0], W = hd[1], P = hd[2], S = hd[3], radius = hd[4], thickness = hd[5], op = hd[6];
        std::vector<float> lm(2 * P);
        std::vector<int32_t> seg(2 * S);
        if (fread(lm.data(), sizeof(float), lm.size(), in) != lm.size()) return 3;
        if (S && fread(seg.data(), sizeof(int32_t), seg.size(), in) != seg.size()) return 3;
        std::vector<int> pts(2 * P);
        for (int i = 0; i < 2 * P; ++i) pts[i] = op == 2 ? trunc_coord(lm[i]) : round_coord(lm[i]);
        const int rad = cap_radius(thickness);
        const CircleRows disc = circle_rows(radius), cap = circle_rows(rad);
        const int discs = op == 2 ? 0 : P;
        std::vector<Segment> segs(op >= 1 ? S : 0);
        std::vector<unsigned char> map((size_t)H * W);
        for (int row0 = 0; row0 < H; row0 += TH) {
            const int row1 = row0 + TH < H ? row0 + TH : H;
            for (size_t s = 0; s < segs.size(); ++s) {
                const int a = seg[2 * s], b = seg[2 * s + 1];
                build_segment(segs[s], pts[2 * a], pts[2 * a + 1], pts[2 * b], pts[2 * b + 1], thickness, H, W, row0, row1);
            }
            for (int y = row0; y < row1; ++y)
                for (int x = 0; x < W; ++x) {
                    bool hit = false;
                    for (int i = 0; i < discs && !hit; ++i) hit = circle_covers(disc, radius, pts[2 * i], pts[2 * i + 1], x, y);
                    for (size_t s = 0; s < segs.size() && !hit; ++s) hit = segment_covers(segs[s], cap, rad, x, y);
                    map[(size_t)y * W + x] = hit;
                }
        }
        fwrite(map.data(), 1, map.size(), out);
        ++cases;
    }
    fclose(in);
    fclose(out);
    printf("%d cases\n", cases);
    return 0;
}
