"""Pillow's 8-bit BICUBIC resize and its RGB -> L rule, restated in numpy (own code, written from the arithmetic of
Pillow's Resample.c / Convert.c): the reference of the device image transform.  test_dataset_cpu.py holds it against
PIL itself, difference 0; the GPU tests then need no PIL.

Plain loops on purpose: the product builds its tables with array operations (animateportrait_amd/data/image_prep.py), and the
two are compared."""
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2


def bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def coeffs(in_size, out_size):
    """precompute_coeffs + normalize_coeffs_8bpc: (bounds (out, 2), weights (out, k), k) as int32"""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    k = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    weights = np.zeros((out_size, k), np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = []
        ww = 0.0
        for x in range(xmax):
            v = bicubic((x + xmin - center + 0.5) * ss)
            w.append(v)
            ww += v
        for x in range(xmax):
            v = w[x] / ww if ww != 0.0 else w[x]
            weights[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return bounds, weights, k


_CACHE = {}


def _coeffs(in_size, out_size):
    if (in_size, out_size) not in _CACHE:
        _CACHE[(in_size, out_size)] = coeffs(in_size, out_size)
    return _CACHE[(in_size, out_size)]


def _pass(a, out_size):
    """resample the LAST axis of the uint8 array ``a`` to out_size: int32 accumulation, rounded, clipped to uint8"""
    in_size = a.shape[-1]
    if in_size == out_size:
        return a
    bounds, weights, k = _coeffs(in_size, out_size)
    idx = np.minimum(bounds[:, :1] + np.arange(k)[None, :], in_size - 1)      # (out, k); taps past the count weigh 0
    taps = a[..., idx].astype(np.int64)                                        # (..., out, k)
    acc = (taps * weights.astype(np.int64)).sum(-1) + (1 << (PRECISION_BITS - 1))
    assert np.abs(acc).max() < 2 ** 31                                         # Pillow (and the kernel) accumulate in int32
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resize(a, out_h, out_w):
    """Image.fromarray(a).resize((out_w, out_h), BICUBIC) for a (H, W) or (H, W, C) uint8 array: horizontal, then vertical"""
    a = np.asarray(a)
    planes = a[None] if a.ndim == 2 else a.transpose(2, 0, 1)                  # (C, H, W)
    planes = _pass(planes, out_w)
    planes = _pass(planes.transpose(0, 2, 1), out_h).transpose(0, 2, 1)
    return planes[0] if a.ndim == 2 else np.ascontiguousarray(planes.transpose(1, 2, 0))


def to_gray(a):
    """Image.fromarray(a).convert('L') for a (H, W, 3) uint8 array"""
    a = a.astype(np.int64)
    return ((19595 * a[..., 0] + 38470 * a[..., 1] + 7471 * a[..., 2] + 0x8000) >> 16).astype(np.uint8)


def transform_u8(a, x, y, flip, load_h, load_w, crop, gray):
    """[Grayscale ->] Resize -> crop (x, y, crop) -> flip: the (OC, crop, crop) uint8 image before ToTensor"""
    if gray and a.ndim == 3 and a.shape[2] == 3:
        a = to_gray(a)
    if a.ndim == 3 and a.shape[2] == 1:
        a = a[..., 0]
    r = resize(a, load_h, load_w)
    r = r[y:y + crop, x:x + crop]
    if flip:
        r = r[:, ::-1]
    return np.ascontiguousarray(r[None] if r.ndim == 2 else r.transpose(2, 0, 1))
