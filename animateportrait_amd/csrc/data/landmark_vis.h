// The per-pixel rule of apd_landmark_vis (host and device: tools/landmark_vis_host_check.cpp runs it under sanitizers).
//
// A frame is drawn in painter's order -- the background, then the segments 0 .. S-1 as cv2.line, then the P filled discs --
// and a later primitive overwrites an earlier one.  Read backwards that is a search: the colour of a pixel is the colour of
// the LAST primitive that covers it, so the discs are tried first, then the segments from S-1 down to 0, and the first hit
// ends the scan.  The coverage tests are the predicates of cv_raster.h, unchanged.
#pragma once
#include "../cv_raster.h"

namespace apd_raster {

constexpr int VIS_BACKGROUND = -2, VIS_DISC = -1;       // what vis_top returns besides a segment number

// the clamp of round_coord for coordinates that are integers already
APD_HD int clamp_coord(int v) { return v < -COORD_MAX ? -COORD_MAX : v > COORD_MAX ? COORD_MAX : v; }

// The primitive on top at (x, y): VIS_DISC, a segment number 0 .. S-1, or VIS_BACKGROUND.  pts: [P][2] clamped (x, y);
// segs: [S] built for a row range that holds y; radius < 0: no discs.
APD_HD int vis_top(const int* pts, int P, const Segment* segs, int S, const CircleRows& disc, int radius, const CircleRows& cap,
                   int rad, int x, int y) {
    if (radius >= 0)
        for (int i = 0; i < P; ++i)
            if (circle_covers(disc, radius, pts[2 * i], pts[2 * i + 1], x, y)) return VIS_DISC;
    for (int s = S - 1; s >= 0; --s)
        if (segment_covers(segs[s], cap, rad, x, y)) return s;
    return VIS_BACKGROUND;
}

// A drawn byte v as a frame value: (2 v + 1) / 255 - 1, the middle of v's bucket under the (x + 1) / 2 * 255 truncation of
// apd_frames_to_u8, so every consumer of the frame (PNG, JPEG, tensor2im) reads v back.  Evaluated in double and rounded once.
APD_HD float byte_level(unsigned v) { return (float)((double)(2 * (int)(v & 255u) + 1) / 255.0 - 1.0); }

}  // namespace apd_raster
