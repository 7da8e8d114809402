"""The host arithmetic of the MTCNN detector restated in numpy (own code, written from the arithmetic of the reference's
MTCNN/detector.py, first_stage.py and box_utils.py and of Pillow's Resample.c): pyramid scales, Pillow's 8-bit BILINEAR
resize, candidate boxes, greedy NMS as sort + suppression sweep, calibrate / square / round, the padded cut-out windows and
the crop arithmetic of align_mtcnn.  test_mtcnn_cpu.py holds it against every intermediate tests/golden/mtcnn.npz records and
against PIL itself; the GPU tests then compare the device against it and the golden.

Box arrays are float64 as in the reference; net outputs enter as float32 and are promoted where numpy promotes them."""
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2
MIN_DETECTION_SIZE, FACTOR, STRIDE, CELL = 12, 0.707, 2, 12
THRESHOLDS = (0.6, 0.7, 0.8)
NMS_THRESHOLDS = (0.7, 0.7, 0.7)
LEVEL_NMS = 0.5


def scales(width, height, min_face_size=20.0):
    """the pyramid's scales, in Python float arithmetic (detector.py:31-50)"""
    out = []
    m = MIN_DETECTION_SIZE / min_face_size
    min_length = min(height, width) * m
    k = 0
    while min_length > MIN_DETECTION_SIZE:
        out.append(m * FACTOR ** k)
        min_length *= FACTOR
        k += 1
    return out


def level_size(width, height, s):
    return math.ceil(width * s), math.ceil(height * s)            # (sw, sh)


def pnet_map_size(h, w):
    """P-Net's output size for a level of h x w: conv3, ceil-mode pool 2/2, conv3, conv3"""
    return (h - 2 + 1) // 2 - 4, (w - 2 + 1) // 2 - 4


# ---- Pillow's 8-bit BILINEAR ---------------------------------------------------------------------------------------------
def bilinear_coeffs(in_size, out_size):
    """precompute_coeffs + normalize_coeffs_8bpc for the triangle filter: (xmin (out,), count (out,), weights (out, k))"""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    k = int(math.ceil(support)) * 2 + 1
    xmin = np.zeros(out_size, np.int64)
    cnt = np.zeros(out_size, np.int64)
    weights = np.zeros((out_size, k), np.int64)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - lo
        w = []
        ww = 0.0
        for x in range(n):
            v = abs((x + lo - center + 0.5) * ss)
            v = 1.0 - v if v < 1.0 else 0.0
            w.append(v)
            ww += v
        for x in range(n):
            v = w[x] / ww if ww != 0.0 else w[x]
            weights[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        xmin[xx], cnt[xx] = lo, n
    return xmin, cnt, weights


def _pass(a, out_size):
    """resample the LAST axis of a uint8 array: int accumulation, rounded, clipped to uint8 (Pillow's intermediate)"""
    in_size = a.shape[-1]
    if in_size == out_size:
        return a
    xmin, cnt, weights = bilinear_coeffs(in_size, out_size)
    idx = np.minimum(xmin[:, None] + np.arange(weights.shape[1])[None, :], in_size - 1)
    acc = (a[..., idx].astype(np.int64) * weights).sum(-1) + (1 << (PRECISION_BITS - 1))
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resize_bilinear(a, out_h, out_w):
    """Image.fromarray(a).resize((out_w, out_h), BILINEAR) of an (H, W, 3) uint8 array: horizontal pass, then vertical"""
    planes = np.asarray(a).transpose(2, 0, 1)
    planes = _pass(planes, out_w)
    planes = _pass(planes.transpose(0, 2, 1), out_h).transpose(0, 2, 1)
    return np.ascontiguousarray(planes.transpose(1, 2, 0))


# ---- boxes ---------------------------------------------------------------------------------------------------------------
def generate_bboxes(probs, offsets, scale, threshold):
    """candidates of one level in row-major order: (n, 9) float64 = 4 rounded corners, score, 4 offsets.
    probs (h, w) float32, offsets (4, h, w) float32"""
    iy, ix = np.nonzero(probs > threshold)
    out = np.empty((iy.size, 9), np.float64)
    out[:, 0] = np.round((STRIDE * ix + 1.0) / scale)
    out[:, 1] = np.round((STRIDE * iy + 1.0) / scale)
    out[:, 2] = np.round((STRIDE * ix + 1.0 + CELL) / scale)
    out[:, 3] = np.round((STRIDE * iy + 1.0 + CELL) / scale)
    out[:, 4] = probs[iy, ix]
    out[:, 5:9] = offsets[:, iy, ix].T
    return out


def overlap(a, b, mode):
    """overlap of box a with box b (rows of x1, y1, x2, y2, ...), in the reference's operation order"""
    area_a = (a[2] - a[0] + 1.0) * (a[3] - a[1] + 1.0)
    area_b = (b[2] - b[0] + 1.0) * (b[3] - b[1] + 1.0)
    w = max(0.0, min(a[2], b[2]) - max(a[0], b[0]) + 1.0)
    h = max(0.0, min(a[3], b[3]) - max(a[1], b[1]) + 1.0)
    inter = w * h
    if mode == 'min':
        return inter / min(area_a, area_b)
    return inter / (area_a + area_b - inter)


def nms(boxes, threshold, mode='union'):
    """greedy NMS as a sort by (score, index) and one sweep from the top: a box still alive is picked and kills every
    lower-ranked box it overlaps by more than the threshold.  Picks in the order they are made."""
    n = len(boxes)
    order = sorted(range(n), key=lambda i: (boxes[i, 4], i))
    alive = [True] * n
    pick = []
    for r in range(n - 1, -1, -1):
        if not alive[r]:
            continue
        i = order[r]
        pick.append(i)
        for q in range(r):
            if alive[q] and overlap(boxes[i], boxes[order[q]], mode) > threshold:
                alive[q] = False
    return np.asarray(pick, np.int64)


def calibrate(boxes, offsets):
    """(n, 5) boxes moved by (n, 4) offsets scaled with the box's width and height"""
    out = np.array(boxes[:, :5], np.float64)
    w = out[:, 2] - out[:, 0] + 1.0
    h = out[:, 3] - out[:, 1] + 1.0
    out[:, 0:4] = out[:, 0:4] + np.stack([w, h, w, h], 1) * offsets
    return out


def square(boxes):
    """the square of the longer side about each box's centre; the reference leaves the score column zero"""
    out = np.zeros_like(boxes[:, :5])
    h = boxes[:, 3] - boxes[:, 1] + 1.0
    w = boxes[:, 2] - boxes[:, 0] + 1.0
    side = np.maximum(h, w)
    out[:, 0] = boxes[:, 0] + w * 0.5 - side * 0.5
    out[:, 1] = boxes[:, 1] + h * 0.5 - side * 0.5
    out[:, 2] = out[:, 0] + side - 1.0
    out[:, 3] = out[:, 1] + side - 1.0
    return out


def rounded(boxes):
    out = boxes.copy()
    out[:, 0:4] = np.round(out[:, 0:4])
    return out


def cutout_windows(boxes, width, height):
    """per box: (x1, y1, w, h) of its window as int32 truncations of the float64 corners, taken BEFORE the clip"""
    w = boxes[:, 2] - boxes[:, 0] + 1.0
    h = boxes[:, 3] - boxes[:, 1] + 1.0
    return np.stack([boxes[:, 0], boxes[:, 1], w, h], 1).astype(np.int32)


def clip_to_image(boxes, width, height):
    """what get_image_boxes leaves in the caller's array: correct_bboxes writes through views of its columns"""
    out = boxes.copy()
    out[:, 2] = np.where(out[:, 2] > width - 1.0, width - 1.0, out[:, 2])
    out[:, 3] = np.where(out[:, 3] > height - 1.0, height - 1.0, out[:, 3])
    out[:, 0] = np.where(out[:, 0] < 0.0, 0.0, out[:, 0])
    out[:, 1] = np.where(out[:, 1] < 0.0, 0.0, out[:, 1])
    return out


def cutouts(image, boxes, size):
    """(n, size, size, 3) uint8: each box's window, zero outside the image, resized with Pillow's BILINEAR"""
    H, W = image.shape[:2]
    out = np.zeros((len(boxes), size, size, 3), np.uint8)
    for i, (x1, y1, w, h) in enumerate(cutout_windows(boxes, W, H)):
        win = np.zeros((h, w, 3), np.uint8)
        xa, xb, ya, yb = max(x1, 0), min(x1 + w, W), max(y1, 0), min(y1 + h, H)
        if xb > xa and yb > ya:
            win[ya - y1:yb - y1, xa - x1:xb - x1] = image[ya:yb, xa:xb]
        out[i] = resize_bilinear(win, size, size)
    return out


def landmarks_to_image(boxes, lm):
    """(n, 10) float32: the nets' unit-square landmarks placed in each box (float64 arithmetic, stored as float32)"""
    w = boxes[:, 2] - boxes[:, 0] + 1.0
    h = boxes[:, 3] - boxes[:, 1] + 1.0
    out = np.empty_like(lm)
    out[:, 0:5] = boxes[:, 0:1] + w[:, None] * lm[:, 0:5]
    out[:, 5:10] = boxes[:, 1:2] + h[:, None] * lm[:, 5:10]
    return out


# ---- align_mtcnn ---------------------------------------------------------------------------------------------------------
def align_window(faces):
    """(x11, y11, size1) of the white-padded square about the largest face (by `size`, first wins), or None without faces"""
    best, maxs = None, 0
    for x1, y1, x2, y2 in np.asarray(faces, np.float64)[:, :4]:
        w = x2 - x1 + 1
        h = y2 - y1 + 1
        size = int(min([w, h]) * 1.2)
        cx = x1 + w // 2
        cy = y1 + h // 2
        if size > maxs:
            size1 = int(round(size / 0.7))
            best = (int(cx - size1 // 2), int(cy - (size1 * 11) // 20), size1)
            maxs = size
    return best


def align_cut(image, window, fill=255):
    """the size1 x size1 cut at (x11, y11), white where it leaves the image"""
    x11, y11, size1 = window
    H, W = image.shape[:2]
    out = np.full((size1, size1, 3), fill, np.uint8)
    xa, xb, ya, yb = max(0, x11), min(W, x11 + size1), max(0, y11), min(H, y11 + size1)
    if xb > xa and yb > ya:
        out[ya - y11:yb - y11, xa - x11:xb - x11] = image[ya:yb, xa:xb]
    return out
