"""Plain restatements of the forward streaming passes of csrc/conv_prepass.h and csrc/instnorm.hip (torch / numpy only), shared by
tests/test_prepass_reference_cpu.py (which checks the restatements themselves) and tests/test_prepass_gpu.py (which holds the
kernels to them).

Written from the text of include/animateportrait_amd.h:
    XS[n][head|tail][C/8][H*W + 1][8 x bf16]     the split tensor; the last 16-byte slot of every plane is all-zero
    v = act((x - mean) * rstd) [+ (res - res_mean) * res_rstd]
    R[ky*C + c][y][x] = src[c][y + ky - pad][x]                               the 7x7 stems' row form, 32 channels
    X'[(ry*2 + rx)*C + c][qy][qx] = pad1(src)[c][2 qy + ry][2 qx + rx]        the stride-2 layers' space-to-depth form
"""
import numpy as np
import torch

SLOPE32 = float(np.float32(0.2))        # the kernels' LeakyReLU slope is the fp32 constant 0.2f
ROW_CHANNELS = 32
REFINE_RATIO = 32.0                     # kInstNormRefineRatio of csrc/common.h: mean^2 > 32 var -> statistics recomputed from the data


# ------------------------------------------------------------------------------------------------------------ the split tensor

def split_encode(v):
    """fp32 -> (head, tail) bf16: head = rne(v), tail = rne(v - head), both differences in fp32 (split_bf16 of csrc/lds_dma.h)."""
    assert v.dtype == torch.float32
    head = v.to(torch.bfloat16)
    tail = (v - head.float()).to(torch.bfloat16)
    return head, tail


def pack_xs(v):
    """[N, C, H, W] fp32 -> the bytes (uint8, 1-D) of XS[n][head|tail][C/8][H*W + 1][8], closing slots zero."""
    n, c, h, w = v.shape
    assert c % 8 == 0
    hw = h * w
    out = torch.zeros(n, 2, c // 8, hw + 1, 8, dtype=torch.bfloat16)
    for part, plane in enumerate(split_encode(v.contiguous())):
        out[:, part, :, :hw, :] = plane.reshape(n, c // 8, 8, hw).permute(0, 1, 3, 2)
    return out.reshape(-1).view(torch.uint8)


def unpack_xs(raw, n, c, h, w):
    """The bytes of a split tensor -> (head, tail) as fp32 [N, C, H, W] and the closing slots as int16 [N, 2, C/8, 8]."""
    hw = h * w
    assert raw.dtype == torch.uint8 and raw.numel() == n * 2 * (c // 8) * (hw + 1) * 16
    words = raw.contiguous().view(torch.int16).reshape(n, 2, c // 8, hw + 1, 8)
    planes = words[:, :, :, :hw, :].contiguous().view(torch.bfloat16).float()
    planes = planes.permute(0, 1, 2, 4, 3).reshape(n, 2, c, h, w)
    return planes[:, 0].contiguous(), planes[:, 1].contiguous(), words[:, :, :, hw, :].contiguous()


def to_octet(x):
    """NCHW -> the channel-octet layout [N][C/8][H*W][8]."""
    n, c, h, w = x.shape
    return x.reshape(n, c // 8, 8, h * w).permute(0, 1, 3, 2).contiguous()


# ------------------------------------------------------------------------------------------------------------ norm + activation

def _per_plane(s, x):
    return s.reshape(x.shape[0], x.shape[1], 1, 1).to(x.dtype)


def norm_act(x, mean, rstd, act, dtype=torch.float32, slope=None):
    """act((x - mean) * rstd) of an [N, C, H, W] tensor; mean / rstd are [N*C] or None (a plain feature).

    dtype = float32: the kernels' own IEEE operations -- a subtraction, a multiplication, and max(t, 0) (ReLU) or
    max(t, slope * t) with slope = float32(0.2) (LeakyReLU).  No FMA can form in that chain, so this is bit-exact.
    dtype = float64: the same formula in double (slope 0.2 unless given)."""
    t = x.to(dtype)
    if mean is not None:
        t = (t - _per_plane(mean, t)) * _per_plane(rstd, t)
    if act == 1:
        t = torch.maximum(t, torch.zeros((), dtype=dtype))
    elif act == 2:
        s = torch.tensor(SLOPE32 if dtype == torch.float32 else (0.2 if slope is None else slope), dtype=dtype)
        t = torch.maximum(t, s * t)
    else:
        assert act == 0
    return t


def stats64(x, eps):
    """fp64 two-pass mean, biased variance and rstd = 1 / sqrt(var + eps) of every plane: three [N*C] float64 tensors."""
    n, c = x.shape[:2]
    v = x.double().reshape(n * c, -1)
    mean = v.mean(1)
    var = ((v - mean[:, None]) ** 2).mean(1)
    return mean, var, 1.0 / torch.sqrt(var + eps)


def tile_edges(hw, tiles):
    """tiles + 1 edges of contiguous pixel runs over [0, hw): uneven on purpose, the last run a single pixel; where a plane has fewer
    pixels than tiles, the surplus runs are empty (their sums are zero)."""
    if tiles == 1:
        return [0, hw]
    if hw < tiles:
        return list(range(hw + 1)) + [hw] * (tiles - hw)
    body = hw - 1
    e = [int(body * (k / (tiles - 1.0)) ** 1.5) for k in range(tiles)]
    for k in range(1, tiles):
        e[k] = max(e[k], e[k - 1] + 1)
    e[tiles - 1] = body
    for k in range(tiles - 2, -1, -1):
        e[k] = min(e[k], e[k + 1] - 1)
    assert e[0] == 0
    return e + [hw]


def make_partials(x, tiles):
    """The producing convolution's statistics tiles [N*C][tiles][2] (fp32): the sum of x and of x^2 over each run of tile_edges, each
    summed in fp64 and rounded to fp32 once."""
    n, c = x.shape[:2]
    v = x.double().reshape(n * c, -1)
    e = tile_edges(v.shape[1], tiles)
    out = torch.zeros(n * c, tiles, 2, dtype=torch.float64)
    for t in range(tiles):
        run = v[:, e[t]:e[t + 1]]
        out[:, t, 0] = run.sum(1)
        out[:, t, 1] = (run * run).sum(1)
    return out.float()


def unrefined_stats(partials, count, eps):
    """What the finalizers compute when they do not go back to the data: the fp32 tiles summed in fp64 (exact), then
    mean = s / count, rstd = 1 / sqrt(q / count - mean^2 + eps) with the variance clamped at zero.  Float64 [N*C] each."""
    p = partials.double()
    s, q = p[:, :, 0].sum(1), p[:, :, 1].sum(1)
    mean = s / count
    var = torch.clamp(q / count - mean * mean, min=0.0)
    return mean, 1.0 / torch.sqrt(var + eps)


# ------------------------------------------------------------------------------------------------------------ the two expansions

def rows_expand(x, pad_mode):
    """[N, C, H, W], C <= 4 -> [N, 32, H, W]: R[ky*C + c][y][x] = x[c][y + ky - 3][x], rows outside the image zero (pad_mode 0) or
    reflected without repeating the edge (pad_mode 1, needs H >= 4); channels 7*C ... 31 are zero."""
    n, c, h, w = x.shape
    assert 7 * c <= ROW_CHANNELS
    out = torch.zeros(n, ROW_CHANNELS, h, w, dtype=x.dtype)
    for ky in range(7):
        for y in range(h):
            sy = y + ky - 3
            if pad_mode == 1:
                assert h > 3
                sy = -sy if sy < 0 else sy
                sy = 2 * (h - 1) - sy if sy >= h else sy
            elif sy < 0 or sy >= h:
                continue
            out[:, ky * c:(ky + 1) * c, y, :] = x[:, :, sy, :]
    return out


def s2d_expand(x):
    """[N, C, H, W], H and W even -> [N, 4C, H/2 + 1, W/2 + 1]: X'[(ry*2 + rx)*C + c][qy][qx] = pad1(x)[c][2 qy + ry][2 qx + rx]."""
    n, c, h, w = x.shape
    assert h % 2 == 0 and w % 2 == 0
    p = torch.zeros(n, c, h + 2, w + 2, dtype=x.dtype)
    p[:, :, 1:h + 1, 1:w + 1] = x
    return torch.cat([p[:, :, ry::2, rx::2] for ry in (0, 1) for rx in (0, 1)], 1).contiguous()
