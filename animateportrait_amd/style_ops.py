"""Operator layer of libapstyle.so: thin wrappers that hand raw device pointers to the kernels of the static cartoon
generator (include/animateportrait_style.h).  Tensors are contiguous fp32 NCHW on the MI355X; outputs are allocated here."""
import torch

from . import _styleapi as S
from .ops import _ptr, _require_device, _stream, EPS
from ._styleapi import ACT_NONE, ACT_RELU  # noqa: F401


def _vec(n, dev):
    return torch.empty(n, dtype=torch.float32, device=dev)


def lin_coeffs(x, rho, gamma, beta, eps=EPS):
    """LIN (gamma / beta of C values) or adaLIN (of N*C values: one pair per sample) of ``x`` folded to the affine pair
    (a, b) of N*C values each: LIN(x) = a x + b  (photo2cartoon.py:488-525)."""
    _require_device(x, 'lin_coeffs input')
    n, c, h, w = x.shape
    if rho.numel() != c or gamma.numel() != beta.numel() or gamma.numel() not in (c, n * c):
        raise ValueError('lin_coeffs: rho of %d, gamma of %d, beta of %d values for %d x %d planes'
                         % (rho.numel(), gamma.numel(), beta.numel(), n, c))
    per_sample = 1 if (gamma.numel() == n * c and n > 1) else 0
    rho, gamma, beta = (t.detach().reshape(-1).contiguous() for t in (rho, gamma, beta))
    for t, name in ((rho, 'rho'), (gamma, 'gamma'), (beta, 'beta')):
        _require_device(t, name)
    planes, a, b = _vec(2 * n * c, x.device), _vec(n * c, x.device), _vec(n * c, x.device)
    S.check(S.lib().aps_lin_coeffs(_ptr(x), n, c, h, w, _ptr(rho), _ptr(gamma), _ptr(beta), per_sample, eps, _ptr(planes), _ptr(a),
                                   _ptr(b), _stream()), 'lin_coeffs')
    return a, b


def affine_apply(x, a, b, act=ACT_NONE, residual=None, want_stats=False):
    """act(a[n,c] x + b[n,c]) (+ residual); want_stats: also the biased InstanceNorm (mean, rstd) of the result."""
    _require_device(x, 'affine_apply input')
    n, c, h, w = x.shape
    for t, name in ((a, 'a'), (b, 'b')):
        _require_device(t, name)
        if t.numel() != n * c:
            raise ValueError('affine_apply: %s of %d values for %d planes' % (name, t.numel(), n * c))
    if residual is not None:
        _require_device(residual, 'affine_apply residual')
        if residual.shape != x.shape:
            raise ValueError('affine_apply: residual shape mismatch')
    y = torch.empty_like(x)
    mean = _vec(n * c, x.device) if want_stats else None
    rstd = _vec(n * c, x.device) if want_stats else None
    S.check(S.lib().aps_affine_apply(_ptr(x), _ptr(a), _ptr(b), act, _ptr(residual), n, c, h, w, _ptr(y), _ptr(mean), _ptr(rstd),
                                     _stream()), 'affine_apply')
    return (y, mean, rstd) if want_stats else y


def _combine(mode, srcs, n, c, h, w, out_shape, want_stats, hs=0, ws=0):
    dev = srcs[0].device
    for t in srcs:
        if t is not None:
            _require_device(t, 'plane_combine source')
    s = list(srcs) + [None] * (4 - len(srcs))
    y = torch.empty(out_shape, dtype=torch.float32, device=dev)
    mean = _vec(n * c, dev) if want_stats else None
    rstd = _vec(n * c, dev) if want_stats else None
    S.check(S.lib().aps_plane_combine(mode, _ptr(s[0]), _ptr(s[1]), _ptr(s[2]), _ptr(s[3]), n, c, h, w, hs, ws, 0, _ptr(y), _ptr(mean),
                                      _ptr(rstd), _stream()), 'plane_combine')
    return (y, mean, rstd) if want_stats else y


def join(r, p0, p1, p2, want_stats=False):
    """r + cat(p0, p1, p2) over channels, widths C/2, C/4, C/4 (ConvBlock.forward, photo2cartoon.py:317-328)."""
    n, c, h, w = r.shape
    if c % 4 or p0.shape != (n, c // 2, h, w) or p1.shape != (n, c // 4, h, w) or p2.shape != (n, c // 4, h, w):
        raise ValueError('join: parts %s %s %s for a residual of %s' % (tuple(p0.shape), tuple(p1.shape), tuple(p2.shape), tuple(r.shape)))
    return _combine(S.JOIN, [r, p0, p1, p2], n, c, h, w, r.shape, want_stats)


def pool2(x, want_stats=False):
    """F.avg_pool2d(x, 2)."""
    n, c, h, w = x.shape
    return _combine(S.POOL2, [x], n, c, h, w, (n, c, h // 2, w // 2), want_stats)


def up2_add(x, skip=None, want_stats=False):
    """skip + nearest_up2(x); skip None: nn.Upsample(scale_factor=2)."""
    n, c, h, w = x.shape
    hs = ws = 0
    if skip is not None:
        if skip.dim() != 4 or skip.shape[:2] != (n, c):
            raise ValueError('up2_add: skip of %s for an input of %s' % (tuple(skip.shape), tuple(x.shape)))
        hs, ws = skip.shape[2:]
    return _combine(S.UP2ADD, [x, skip], n, c, h, w, (n, c, 2 * h, 2 * w), want_stats, hs, ws)


def sum3(x, a, b, want_stats=False):
    """x + a + b (HourGlass.forward with use_res)."""
    if a.shape != x.shape or b.shape != x.shape:
        raise ValueError('sum3: shapes %s %s %s' % (tuple(x.shape), tuple(a.shape), tuple(b.shape)))
    n, c, h, w = x.shape
    return _combine(S.SUM3, [x, a, b], n, c, h, w, x.shape, want_stats)


def plane_mean(x, relu=False):
    """F.adaptive_avg_pool2d(x, 1) as (N, C), optionally of relu(x)."""
    _require_device(x, 'plane_mean input')
    n, c, h, w = x.shape
    mean = _vec(n * c, x.device)
    S.check(S.lib().aps_plane_combine(S.STAT, _ptr(x), None, None, None, n, c, h, w, 0, 0, S.STAT_RELU if relu else 0, None, _ptr(mean),
                                      None, _stream()), 'plane_combine')
    return mean.view(n, c)


def quantize_u8(x):
    """The uint8 round trip the reference sends the photo through before the cartoon generator
    (geomcgt_ifw_test_model.py:287-289, photo2cartoon.py:584): floor((x + 1) 127.5) / 127.5 - 1 in float32.  The input
    contract is [-1, 1]; values outside are clamped to the byte range (numpy's cast would wrap them)."""
    return torch.floor((x + 1) * 127.5).clamp_(0, 255) / 127.5 - 1
