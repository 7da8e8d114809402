"""The float64 contract of the photo-landmark detector (animateportrait_amd/fan.py, landmarks.py, csrc/face/face_fan.hip), in
numpy / torch on the CPU.  It states, after face_alignment's FaceAlignment.get_landmarks with flip_input=True:

* the box arithmetic: centre, scale and ``transform(p, centre, scale, S, invert=True)`` (box_frame, transform);
* the crop about a box: a zero-filled window copied from the picture where they overlap -- the package's 1-based index
  arithmetic restated below -- resized by OpenCV's 8-bit INTER_LINEAR rule (crop);
* the network, BatchNorm as written (fan_forward), in the dtype of the state_dict it is given;
* the flip sum and the decode of the heat maps (flip_sum, decode).

Parity with the package, its checkpoint and cv2 itself is unpinned: none of them is part of this repository.
"""
import numpy as np
import torch
import torch.nn.functional as F

POINTS = 68

# the 68-point mirror table: jaw i <-> 16 - i, brows 17 <-> 26 .. 21 <-> 22, nose 31 <-> 35 and 32 <-> 34, eyes, mouth
PAIR = list(range(POINTS))
for _a, _b in ([(i, 16 - i) for i in range(8)] + [(17 + i, 26 - i) for i in range(5)] + [(31, 35), (32, 34)] +
               [(36, 45), (37, 44), (38, 43), (39, 42), (40, 47), (41, 46)] +
               [(48, 54), (49, 53), (50, 52), (55, 59), (56, 58), (60, 64), (61, 63), (65, 67)]):
    PAIR[_a], PAIR[_b] = _b, _a


# ------------------------------------------------------------------------------------------------------------ box arithmetic
def box_frame(box):
    """(centre x, centre y, scale) of a face box (x0, y0, x1, y1), in float64 and this order"""
    x0, y0, x1, y1 = (np.float64(v) for v in box)
    cx = x1 - (x1 - x0) / np.float64(2.0)
    cy = y1 - (y1 - y0) / np.float64(2.0) - (y1 - y0) * np.float64(0.12)
    scale = (x1 - x0 + y1 - y0) / np.float64(195.0)
    return cx, cy, scale


def transform(px, py, box, S):
    """transform((px, py), centre, scale, S, invert=True) before any truncation: the inverse of [[a, 0, bx], [0, a, by], [0, 0, 1]]
    (h = 200 scale, a = S / h, bx = S (0.5 - cx / h), by likewise) is [[1 / a, 0, -bx / a], [0, 1 / a, -by / a], [0, 0, 1]]."""
    cx, cy, scale = box_frame(box)
    h = np.float64(200.0) * scale
    a = np.float64(S) / h
    bx = np.float64(S) * (np.float64(0.5) - cx / h)
    by = np.float64(S) * (np.float64(0.5) - cy / h)
    i00 = np.float64(1.0) / a
    return i00 * np.float64(px) + (-bx / a), i00 * np.float64(py) + (-by / a)


def window(box, R):
    """(ul.x, ul.y, width, height) of the crop window: ul = trunc(transform((1, 1))), br = trunc(transform((R, R)))"""
    ulx, uly = (int(v) for v in transform(1, 1, box, R))
    brx, bry = (int(v) for v in transform(R, R, box, R))
    return ulx, uly, brx - ulx, bry - uly


# ---------------------------------------------------------------------------------------------------------------- the crop
def _linear_axis(src, dst):
    """cv2's INTER_LINEAR taps per destination index: (first source index, weight of it, weight of the next), 11-bit"""
    scale = np.float64(src) / np.float64(dst)
    f = ((np.arange(dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(np.float32)
    f[s < 0] = 0
    s[s < 0] = 0
    f[s >= src - 1] = 0
    s[s >= src - 1] = src - 1
    w0 = np.rint((np.float32(1.0) - f) * np.float32(2048.0)).astype(np.int64)
    w1 = np.rint(f * np.float32(2048.0)).astype(np.int64)
    return s, w0, w1


def resize_linear_u8(img, R):
    """cv2.resize(img, (R, R), interpolation=INTER_LINEAR) of an (h, w, C) uint8 image, as its 8-bit path computes it"""
    h, w = img.shape[:2]
    sx, a0, a1 = _linear_axis(w, R)
    sy, b0, b1 = _linear_axis(h, R)
    v = img.astype(np.int64)
    rows = v[:, sx] * a0[None, :, None] + v[:, np.minimum(sx + 1, w - 1)] * a1[None, :, None]          # (h, R, C), scaled by 2^11
    S0, S1 = rows[sy], rows[np.minimum(sy + 1, h - 1)]
    out = (((b0[:, None, None] * (S0 >> 4)) >> 16) + ((b1[:, None, None] * (S1 >> 4)) >> 16) + 2) >> 2
    return np.clip(out, 0, 255).astype(np.uint8)


def crop_u8(img, box, R):
    """face_alignment's crop(image, centre, scale, R) as uint8 (R, R, 3).  The package's 1-based arithmetic,
        newX = [max(1, -ul.x + 1), min(br.x, wd) - ul.x]     oldX = [max(1, ul.x + 1), min(br.x, wd)]      (Y likewise)
        new[newY[0] - 1:newY[1], newX[0] - 1:newX[1]] = image[oldY[0] - 1:oldY[1], oldX[0] - 1:oldX[1]]
    puts image pixel (wy + ul.y, wx + ul.x) at window pixel (wy, wx) wherever that pixel exists; the rest stays zero.  (Where
    window and picture do not overlap at all the package's slices no longer agree in shape and it raises; here: all zeros.)"""
    H, W = img.shape[:2]
    ulx, uly, ww, wh = window(box, R)
    win = np.zeros((wh, ww, 3), np.uint8)
    y0, y1, x0, x1 = max(0, -uly), min(wh, H - uly), max(0, -ulx), min(ww, W - ulx)
    if y1 > y0 and x1 > x0:
        win[y0:y1, x0:x1] = img[y0 + uly:y1 + uly, x0 + ulx:x1 + ulx]
    return resize_linear_u8(win, R)


def crop(img, box, R, order='bgr', flip=True):
    """(1 + flip, 3, R, R) float32 in [0, 1]: the network's input for an RGB picture.  'bgr': plane c is channel 2 - c, which is
    what the reference's cv2.imread array looks like to a network that takes RGB; row 1: row 0 mirrored in x."""
    u8 = crop_u8(img, box, R)
    if order == 'bgr':
        u8 = u8[:, :, ::-1]
    x = (np.transpose(u8, (2, 0, 1)).astype(np.float32) / np.float32(255.0))[None]
    return np.concatenate([x, x[:, :, :, ::-1]], 0) if flip else x


# ------------------------------------------------------------------------------------------------------------- the network
def _bn_relu(sd, p, x, eps=1e-5):
    return F.relu(F.batch_norm(x, sd[p + '.running_mean'], sd[p + '.running_var'], sd[p + '.weight'], sd[p + '.bias'], False, 0.0, eps))


def _conv_block(sd, p, x):
    o1 = F.conv2d(_bn_relu(sd, p + '.bn1', x), sd[p + '.conv1.weight'], None, 1, 1)
    o2 = F.conv2d(_bn_relu(sd, p + '.bn2', o1), sd[p + '.conv2.weight'], None, 1, 1)
    o3 = F.conv2d(_bn_relu(sd, p + '.bn3', o2), sd[p + '.conv3.weight'], None, 1, 1)
    r = x
    if p + '.downsample.2.weight' in sd:
        r = F.conv2d(_bn_relu(sd, p + '.downsample.0', x), sd[p + '.downsample.2.weight'])
    return torch.cat([o1, o2, o3], 1) + r


def _hourglass(sd, p, level, x):
    up1 = _conv_block(sd, '%s.b1_%d' % (p, level), x)
    low1 = _conv_block(sd, '%s.b2_%d' % (p, level), F.avg_pool2d(x, 2, stride=2))
    low2 = _hourglass(sd, p, level - 1, low1) if level > 1 else _conv_block(sd, p + '.b2_plus_1', low1)
    low3 = _conv_block(sd, '%s.b3_%d' % (p, level), low2)
    return up1 + F.interpolate(low3, scale_factor=2, mode='nearest')


def fan_forward(sd, x, num_modules, depth=4):
    """the LAST stack's heat maps of face_alignment's FAN.forward for state_dict ``sd``, in sd's dtype"""
    x = F.relu(F.batch_norm(F.conv2d(x, sd['conv1.weight'], sd['conv1.bias'], 2, 3), sd['bn1.running_mean'], sd['bn1.running_var'],
                            sd['bn1.weight'], sd['bn1.bias'], False, 0.0, 1e-5))
    x = F.avg_pool2d(_conv_block(sd, 'conv2', x), 2, stride=2)
    previous = _conv_block(sd, 'conv4', _conv_block(sd, 'conv3', x))
    maps = None
    for i in range(num_modules):
        ll = _conv_block(sd, 'top_m_%d' % i, _hourglass(sd, 'm%d' % i, depth, previous))
        ll = F.conv2d(ll, sd['conv_last%d.weight' % i], sd['conv_last%d.bias' % i])
        ll = _bn_relu(sd, 'bn_end%d' % i, ll)
        maps = F.conv2d(ll, sd['l%d.weight' % i], sd['l%d.bias' % i])
        if i < num_modules - 1:
            previous = previous + F.conv2d(ll, sd['bl%d.weight' % i], sd['bl%d.bias' % i]) + \
                F.conv2d(maps, sd['al%d.weight' % i], sd['al%d.bias' % i])
    return maps


def cast(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


# --------------------------------------------------------------------------------------------------------------- the decode
def flip_sum(hm, hm_flipped):
    """hm[b, j] + mirror_x(hm_flipped[b, pair[j]]), in the arrays' dtype and this order"""
    hm, hm_flipped = np.asarray(hm), np.asarray(hm_flipped)
    return hm + hm_flipped[:, PAIR][:, :, :, ::-1]


def decode(hm, boxes, hm_flipped=None, truncate=True):
    """(B, 68, Hm, Hm) maps -> (B, 68, 2) float32 landmarks in picture pixels.  The maps are summed in THEIR dtype (the kernel:
    float32); positions are exact in float32; the transform is float64."""
    m = np.asarray(hm) if hm_flipped is None else flip_sum(hm, hm_flipped)
    B, P, Hm, _ = m.shape
    out = np.zeros((B, P, 2), np.float32)
    for b in range(B):
        for j in range(P):
            idx = int(np.argmax(m[b, j]))                    # the lowest flat index among equal maxima
            px, py = idx % Hm, idx // Hm
            x, y = np.float32(px + 1), np.float32(py + 1)
            if 0 < px < Hm - 1 and 0 < py < Hm - 1:
                x += np.float32(0.25) * np.sign(m[b, j, py, px + 1] - m[b, j, py, px - 1]).astype(np.float32)
                y += np.float32(0.25) * np.sign(m[b, j, py + 1, px] - m[b, j, py - 1, px]).astype(np.float32)
            X, Y = transform(np.float64(x - np.float32(0.5)), np.float64(y - np.float32(0.5)), boxes[b], Hm)
            if truncate:
                X, Y = np.trunc(X), np.trunc(Y)
            out[b, j] = (np.float32(X), np.float32(Y))
    return out


def detect(sd, img, box, num_modules, depth=4, R=256, order='bgr', flip=True, truncate=True):
    """the whole statement in float64 for one picture: (68, 2) float32"""
    x = torch.from_numpy(crop(img, box, R, order, flip).astype(np.float64))
    maps = fan_forward(cast(sd, torch.float64), x, num_modules, depth).numpy()
    return decode(maps[:1], [box], maps[1:2] if flip else None, truncate)[0], maps
