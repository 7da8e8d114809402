"""OpenCV's 8-bit INTER_CUBIC resize restated in numpy (own code, written from the rule as documented for cv::resize's
fixed-point path): the reference of the device's aligned 512 x 512 picture.

The rule, per axis: for destination index d, f = float((d + 0.5) * scale - 0.5) with scale = 1 / (dst / src) in double;
s = floor(f), t = f - s in float; the four taps s - 1 .. s + 2 are clamped to the image (replicated border); their float
weights are the cubic with a = -0.75, the fourth being 1 minus the other three; each is scaled by 2^11 and rounded half to
even to int16.  The horizontal pass keeps the exact int32 sums; the vertical pass sums them and the result is
(v + 2^21) >> 22, saturated to uint8.

cv2 is absent from the build image: tests/golden/check_cv_resize.py compares this file with cv2.resize on a machine that has
it.  Until that has been run, parity with cv2 itself is unpinned."""
import numpy as np

COEF_BITS = 11
A = np.float32(-0.75)


def cubic_table(src, dst):
    """(taps (dst, 4) int64 clamped source indices, weights (dst, 4) int64 in 2^-11)"""
    scale = 1.0 / (float(dst) / float(src))
    one = np.float32(1.0)
    taps = np.zeros((dst, 4), np.int64)
    weights = np.zeros((dst, 4), np.int64)
    for d in range(dst):
        f = np.float32((d + 0.5) * scale - 0.5)
        s = int(np.floor(f))
        x = np.float32(f - np.float32(s))
        c = np.empty(4, np.float32)
        c[0] = ((A * (x + one) - np.float32(5) * A) * (x + one) + np.float32(8) * A) * (x + one) - np.float32(4) * A
        c[1] = ((A + np.float32(2)) * x - (A + np.float32(3))) * x * x + one
        c[2] = ((A + np.float32(2)) * (one - x) - (A + np.float32(3))) * (one - x) * (one - x) + one
        c[3] = one - c[0] - c[1] - c[2]
        q = np.rint(c * np.float32(1 << COEF_BITS))                # float32 product, round half to even
        weights[d] = np.clip(q, -32768, 32767).astype(np.int64)
        taps[d] = np.clip(s - 1 + np.arange(4), 0, src - 1)
    return taps, weights


def resize_cubic(a, out_h, out_w):
    """(H, W, C) uint8 -> (out_h, out_w, C) uint8"""
    a = np.asarray(a)
    H, W = a.shape[:2]
    xt, xw = cubic_table(W, out_w)
    yt, yw = cubic_table(H, out_h)
    rows = (a.astype(np.int64)[:, xt, :] * xw[None, :, :, None]).sum(2)            # (H, out_w, C)
    acc = (rows[yt] * yw[:, :, None, None]).sum(1)                                 # (out_h, out_w, C)
    return np.clip((acc + (1 << (2 * COEF_BITS - 1))) >> (2 * COEF_BITS), 0, 255).astype(np.uint8)
