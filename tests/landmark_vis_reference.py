"""The expected picture of apd_landmark_vis, composed from oracle/cv_raster: every primitive is drawn into a fresh mask with
``thick_line`` / ``fill_circle`` in draw order -- the segments 0 .. S-1, then the P discs -- and the mask is painted with
the primitive's colour, ``img[mask] = colour``, so a later primitive overwrites an earlier one as successive cv2 calls on one
image do.  Also the cases the device test and tools/landmark_vis_host_check.py share.

Like the rest of oracle/cv_raster this is **unpinned against cv2 itself**: cv2 cannot be imported in the build image.  A
maintainer with opencv-python runs tests/golden/check_landmark_vis.py (one minute), which draws the same pictures with direct
cv2.line / cv2.circle calls and compares them with this composition."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COORD_MAX = 1 << 20


def rgb_bytes(rgb):
    return np.array([(int(rgb) >> 16) & 255, (int(rgb) >> 8) & 255, int(rgb) & 255], np.uint8)


def draw(pts, seg, seg_rgb, height, width, radius, thickness, disc_rgb, bg_rgb=0xFFFFFF, bg=None):
    """One frame: pts (P, 2) integers, seg (S, 2), seg_rgb (S,) 0xRRGGBB, bg None or (height, width, 3) uint8 -> (height, width,
    3) uint8.  Coordinates are clamped to +-2^20 first, as the kernel clamps them."""
    from oracle import cv_raster
    pts = np.clip(np.asarray(pts, dtype=np.int64), -COORD_MAX, COORD_MAX)
    img = np.empty((height, width, 3), np.uint8)
    img[:] = rgb_bytes(bg_rgb) if bg is None else bg
    for (a, b), rgb in zip(np.asarray(seg, dtype=np.int64).reshape(-1, 2), np.asarray(seg_rgb, dtype=np.int64).reshape(-1)):
        mask = np.zeros((height, width), np.uint8)
        cv_raster.thick_line(mask, (int(pts[a, 0]), int(pts[a, 1])), (int(pts[b, 0]), int(pts[b, 1])), thickness)
        img[mask > 0] = rgb_bytes(rgb)
    if radius >= 0:
        for x, y in pts:
            mask = np.zeros((height, width), np.uint8)
            cv_raster.fill_circle(mask, int(x), int(y), radius)
            img[mask > 0] = rgb_bytes(disc_rgb)
    return img


def bucket_middle(v, dtype=np.float64):
    """the frame value apd_landmark_vis stores for the byte v: (2 v + 1) / 255 - 1 evaluated in `dtype`, as float32"""
    v = np.asarray(v).astype(dtype)
    return ((dtype(2) * v + dtype(1)) / dtype(255) - dtype(1)).astype(np.float32)


def to_u8(x):
    """apd_frames_to_u8's rule on a float32 array: (uint8)((x + 1) / 2 * 255), every step in float32"""
    x = np.asarray(x, dtype=np.float32)
    v = (x + np.float32(1)) / np.float32(2) * np.float32(255)
    return np.clip(np.nan_to_num(v, nan=0.0), 0, 255).astype(np.uint8)


def fixture_landmarks():
    """the 68 points tools/raster_host_check.py draws the 64-segment table on, at 256 x 256 (float64)"""
    rng = np.random.RandomState(1)
    return np.stack([np.linspace(60, 200, 68) + rng.uniform(-20, 20, 68), 128 + 70 * np.sin(np.arange(68)) + rng.uniform(-5, 5, 68)], 1)


PAINTER_RGB = (0x1090F0, 0x00C000, 0x0000FF, 0xFFFF00, 0x7F0180)


def painter_points():
    """37 x 53 (H x W), N = 3, P = 6: points 0-1 and 2-3 are two segments of different colours that cross at (26, 18), where
    point 4 puts a disc; point 5 is far outside -- beyond the clamp in frame 1; the frames differ by a shift"""
    base = np.array([[6, 4], [46, 32], [44, 5], [8, 31], [26, 18], [90, -40]], np.int64)
    pts = np.stack([base, base + [3, -2], base + [-5, 6]])
    pts[1, 5] = (-(1 << 21), 1 << 21)
    return pts.astype(np.int32)


# segments in draw order: the two that cross (the second lies over the first), a zero-length one on the first one's end, one
# wholly outside (both its ends are point 5), one that leaves the frame
PAINTER_SEG = np.array([(0, 1), (2, 3), (0, 0), (5, 5), (1, 5)], np.int32)


def cases():
    """name -> (H, W, pts (N, P, 2) int32, seg (S, 2) int32, seg_rgb (S,) uint32, radius, thickness, disc_rgb, bg_rgb): what
    the device test and the host check both draw with a constant background"""
    from animateportrait_amd.data.visuals import FACE_CONTOURS as table
    out = {}
    pts = painter_points()
    rgb = np.array(PAINTER_RGB, np.uint32)
    for thickness, radius in ((2, 3), (5, 0), (2, -1), (5, 3)):
        out['painter_t%d_r%d' % (thickness, radius)] = (37, 53, pts, PAINTER_SEG, rgb, radius, thickness, 0xFF0000, 0xFFFFFF)
    lm = fixture_landmarks()
    for size in (256, 512):
        two = np.stack([lm * (size / 256.0), (lm + [7.5, -4.25]) * (size / 256.0)]).astype(np.int32)          # truncation
        out['face%d' % size] = (size, size, two, table['segments'], table['colours'], size // 256, 2 * (size // 256),
                                table['disc_rgb'], 0xFFFFFF)
    one = np.array([[[0, 0], [5, 0]]], np.int32)
    out['one1x1'] = (1, 1, one, np.array([(0, 1)], np.int32), np.array([0x123456], np.uint32), -1, 1, 0xFF0000, 0x00FF00)
    tall = np.array([[[8, 3], [2, 1000], [15, 500], [-3, 700]]], np.int32)
    out['tall1024x17'] = (1024, 17, tall, np.array([(0, 1), (1, 2), (2, 3)], np.int32), np.array([0x0000FF, 0x00FF00, 0x102030], np.uint32),
                          2, 3, 0xFF0000, 0x000000)
    return out


def expected(case):
    """(N, H, W, 3) uint8 of one of cases()"""
    h, w, pts, seg, rgb, radius, thickness, disc_rgb, bg_rgb = case
    return np.stack([draw(p, seg, rgb, h, w, radius, thickness, disc_rgb, bg_rgb) for p in pts])
