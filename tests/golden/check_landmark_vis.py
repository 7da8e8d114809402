#!/usr/bin/env python3
"""One-minute check for a maintainer WITH opencv-python (4.2.0.34) installed -- it is absent from the build image, and pytest
does not run this file: does the composition tests/landmark_vis_reference.py makes of oracle/cv_raster primitives equal what
successive cv2.line / cv2.circle calls really draw on one image?  Draws the FACE_CONTOURS table on the fixture landmarks at
256 and 512 px the way vis_landmark draws it, and the painter's-order cases, and compares every pixel.

    python tests/golden/check_landmark_vis.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def cv2_picture(pts, seg, seg_rgb, height, width, radius, thickness, disc_rgb, bg_rgb):
    """the same frame by direct cv2 calls, colours given as RGB tuples on an RGB image"""
    import cv2
    import landmark_vis_reference as ref
    img = np.empty((height, width, 3), np.uint8)
    img[:] = ref.rgb_bytes(bg_rgb)
    pts = np.clip(np.asarray(pts, dtype=np.int64), -ref.COORD_MAX, ref.COORD_MAX)
    for (a, b), rgb in zip(seg, seg_rgb):
        cv2.line(img, (int(pts[a, 0]), int(pts[a, 1])), (int(pts[b, 0]), int(pts[b, 1])), tuple(int(c) for c in ref.rgb_bytes(rgb)), thickness)
    if radius >= 0:
        for x, y in pts:
            cv2.circle(img, (int(x), int(y)), radius, tuple(int(c) for c in ref.rgb_bytes(disc_rgb)), -1)
    return img


def main():
    import landmark_vis_reference as ref
    bad = 0
    for name, case in sorted(ref.cases().items()):
        h, w, pts, seg, rgb, radius, thickness, disc_rgb, bg_rgb = case
        if thickness == 1:
            print('%-18s skipped: cv2 draws thickness 1 as a Bresenham line, the restatement as the quad (include/animateportrait_data.h)' % name)
            continue
        want = ref.expected(case)
        for n, frame in enumerate(pts):
            if np.abs(frame).max() > 1 << 15:
                print('%-18s frame %d skipped: a coordinate beyond 2^15 is the clamp\'s case, not one cv2 is asked to draw here '
                      '(its 16.16 fixed point holds 15 integer bits in an int32 argument)' % (name, n))
                continue
            diff = int((cv2_picture(frame, seg, rgb, h, w, radius, thickness, disc_rgb, bg_rgb) != want[n]).any(-1).sum())
            bad += diff > 0
            print('%-18s frame %d: %d pixels differ %s' % (name, n, diff, 'OK' if diff == 0 else 'MISMATCH'))
    raise SystemExit(1 if bad else 0)


if __name__ == '__main__':
    main()
