"""The image transform of the reference's data layer (Module2/data/base_dataset.py:153-213 get_transform /
get_transform_mask): [Grayscale ->] Resize(load, BICUBIC) -> crop -> flip -> ToTensor [-> Normalize], for a batch of
decoded 8-bit images.

``prep_device`` runs it as one ``apd_image_prep_u8`` launch (libapdata.so), ``prep_host`` through PIL on the CPU.  Both
give the same bits: Pillow's 8-bit resampler is integer arithmetic on coefficient tables, which ``resample_table`` builds
in double exactly as Pillow's precompute_coeffs / normalize_coeffs_8bpc do, and ToTensor / Normalize are a 256-entry table
computed with the float32 ops torchvision uses."""
import ctypes
import functools
import math

import numpy as np
import torch

from .. import _dataapi as D

PRECISION_BITS = 32 - 8 - 2


def _bicubic(x):
    """Pillow's bicubic_filter (a = -0.5), elementwise on a float64 array, same operation order"""
    a = -0.5
    x = np.abs(x)
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    far = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


@functools.lru_cache(maxsize=64)
def resample_table(in_size, out_size):
    """Pillow's coefficients for resizing one axis from in_size to out_size with BICUBIC: (bounds (out, 2) int32 -- first
    source index, tap count; weights (out, k) int32 with 22 fractional bits, zero past the count; k).  None when the size
    does not change (Pillow skips the pass)."""
    if in_size == out_size:
        return None
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    k = int(math.ceil(support)) * 2 + 1
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale          # in0 = 0
    ss = 1.0 / filterscale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)           # (int) truncates; below zero is clamped anyway
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    t = np.arange(k, dtype=np.int64)[None, :]
    w = _bicubic((t + xmin[:, None] - center[:, None] + 0.5) * ss)
    w = np.where(t < xmax[:, None], w, 0.0)
    ww = np.cumsum(w, axis=1)[:, -1:]                                         # summed tap by tap, as the C loop does
    w = np.where(ww != 0.0, w / np.where(ww != 0.0, ww, 1.0), w)
    fixed = np.where(w < 0, -0.5 + w * (1 << PRECISION_BITS), 0.5 + w * (1 << PRECISION_BITS)).astype(np.int64)   # (int): toward 0
    fixed = np.where(t < xmax[:, None], fixed, 0).astype(np.int32)
    bounds = np.stack([xmin, xmax], 1).astype(np.int32)
    return np.ascontiguousarray(bounds), np.ascontiguousarray(fixed), k


def lut(kind):
    """The 256 values ToTensor [+ Normalize(0.5, 0.5)] give an 8-bit pixel, in torchvision's own float32 operations."""
    v = torch.arange(256, dtype=torch.float32).div(255)
    if kind == 'image':
        return v.sub(0.5).div(0.5)
    if kind == 'mask':
        return v
    raise ValueError("lut: kind must be 'image' or 'mask', not %r" % (kind,))


_DEV = {}        # (device, what...) -> device tensors uploaded once: tables and LUTs


def _table_on(device, in_size, out_size):
    key = (str(device), 'table', in_size, out_size)
    if key not in _DEV:
        tab = resample_table(in_size, out_size)
        _DEV[key] = None if tab is None else (torch.from_numpy(tab[0]).to(device), torch.from_numpy(tab[1]).to(device), tab[2])
    return _DEV[key]


def _lut_on(device, kind):
    key = (str(device), 'lut', kind)
    if key not in _DEV:
        _DEV[key] = lut(kind).to(device)
    return _DEV[key]


def describe(n, hs, ws, c, load_w, load_h, crop, to_gray, max_x=0, max_y=0):
    kh = 0 if ws == load_w else int(math.ceil(2.0 * max(ws / load_w, 1.0))) * 2 + 1
    kv = 0 if hs == load_h else int(math.ceil(2.0 * max(hs / load_h, 1.0))) * 2 + 1
    return D.ApdImagePrep(n, hs, ws, c, load_w, load_h, crop, int(bool(to_gray)), kh, kv, max_x, max_y)


def prep_device(src, params, load_size, crop, to_gray, kind, out=None):
    """src: (N, Hs, Ws, C) uint8 on the device; params: (N, 3) int32 rows (crop x, crop y, flip), on the host or the device.
    Returns the (N, OC, crop, crop) float32 device tensor (written into ``out`` when given).  One launch on the current
    stream, no synchronisation apart from the read of ``params`` when it lives on the device."""
    if not (torch.is_tensor(src) and src.is_cuda and src.dtype == torch.uint8 and src.dim() == 4 and src.is_contiguous()):
        raise ValueError('prep_device: expected a contiguous (N, Hs, Ws, C) uint8 device tensor')
    n, hs, ws, c = src.shape
    load_w, load_h = (load_size, load_size) if isinstance(load_size, int) else load_size
    params = torch.as_tensor(params, dtype=torch.int32).reshape(n, 3)
    host = params.cpu()
    pdev = params.to(src.device).contiguous()
    d = describe(n, hs, ws, c, load_w, load_h, crop, to_gray, int(host[:, 0].max()), int(host[:, 1].max()))
    if int(host[:, :2].min()) < 0:
        raise ValueError('prep_device: negative crop offset')
    oc = 3 if (c == 3 and not to_gray) else 1
    if out is None:
        out = torch.empty((n, oc, crop, crop), dtype=torch.float32, device=src.device)
    elif tuple(out.shape) != (n, oc, crop, crop) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != src.device:
        raise ValueError('prep_device: out must be a contiguous (%d, %d, %d, %d) float32 tensor on %s' % (n, oc, crop, crop, src.device))
    th = _table_on(src.device, ws, load_w)
    tv = _table_on(src.device, hs, load_h)
    table = _lut_on(src.device, kind)

    def p(t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None else None
    with torch.cuda.device(src.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream(src.device).cuda_stream)
        D.check(D.lib().apd_image_prep_u8(ctypes.byref(d), p(src), p(pdev), p(th[0] if th else None), p(th[1] if th else None),
                                          p(tv[0] if tv else None), p(tv[1] if tv else None), p(table), p(out), stream),
                'image_prep_u8')
    return out


def prep_host_u8(arr, x, y, flip, load_size, crop, to_gray):
    """One decoded image (Hs, Ws) / (Hs, Ws, 3) uint8 -> the (OC, crop, crop) uint8 image the reference's transform holds before
    ToTensor, through PIL itself."""
    from PIL import Image
    img = Image.fromarray(arr)
    if to_gray:
        img = img.convert('L')
    load_w, load_h = (load_size, load_size) if isinstance(load_size, int) else load_size
    img = img.resize((load_w, load_h), Image.BICUBIC)
    if load_w > crop or load_h > crop:
        img = img.crop((x, y, x + crop, y + crop))
    if flip:
        img = img.transpose(Image.FLIP_LEFT_RIGHT)
    a = np.asarray(img)
    return np.ascontiguousarray(a[None] if a.ndim == 2 else a.transpose(2, 0, 1))


def prep_host(arrs, params, load_size, crop, to_gray, kind, pool=None):
    """The batch ``prep_device`` returns, computed by PIL on the CPU: (N, OC, crop, crop) float32 host tensor.  ``pool``: a
    concurrent.futures executor to spread the images over (Pillow releases the GIL while it resamples); None = this thread."""
    def one(ap):
        a, p = ap
        return prep_host_u8(a, int(p[0]), int(p[1]), int(p[2]), load_size, crop, to_gray)
    u8 = np.stack(list((pool.map if pool is not None else map)(one, zip(arrs, params))))
    return lut(kind)[torch.from_numpy(u8).long()]
