"""GPU (-m gpu): the forward streaming passes of csrc/conv_prepass.h and csrc/instnorm.hip through the C ABI, against the plain
restatements of tests/prepass_reference.py:

    ap_norm_apply_split_ex       norm_split_kernel<VEC, XB16, RES> (12 instantiations) and norm_split_oct_kernel<RES> (2)
    ap_instnorm_finalize[_octet] instnorm_finalize_kernel, plane and channel-octet addressing
    ap_instnorm_apply            instnorm_apply_kernel, up to the first plane size at which its capped grid strides
    ap_split_prepass_rows        split_rows_kernel<7, 1..4>
    ap_split_prepass_s2d         split_s2d_kernel

No kernel here has a dependence across pixels, so the shapes are the smallest that cross a block edge (256 pixels for VEC = 1,
1024 for VEC = 4, 512 for the octet form with a 128-pixel stride between a lane's four pixels), a tile-loop edge (8 lanes per channel
in the norm/split pass, 64 in the finalizer) or the plane stride H*W + 1 of the split tensor (n > 0, channel group > 0).

Every output lies in a window of a larger allocation, 16-byte aligned and no more, between guard bytes that have to survive; the
window starts as 0xFF bytes (NaN as fp32 and as bf16), so a store that was skipped shows as well as one that went astray.

Bars.  None is measured:
  * without a residual, y = act((x - mean) * rstd) is a subtraction, a multiplication and a max in fp32: no FMA can form, and the
    result equals the fp32 restatement bit for bit; the split copy is an exact function of it (byte for byte);
  * with a residual, a = the activated term and b = the residual term in fp64 from the same fp32 inputs: |y - (a + b)| <=
    2^-21 (|a| + |b|) -- at most four fp32 roundings per term (4 * 2^-24), times 2 for the final add (an FMA there only helps);
  * statistics from partial tiles against the fp64 two-pass ones: the mean within one fp32 ulp of float32(mean64) plus
    2^-24 |mean| (the tiles' roundings), rstd within 2^-17 relative -- tests/test_prepass_reference_cpu.py shows that the
    unrefined formula holds this where mean^2 <= 32 var and misses it by orders of magnitude on ill-conditioned planes;
  * y of such a plane against fp64 InstanceNorm with the fp64 statistics: those two bars carried through (x - mean) * rstd,
    |y - y64| <= |y64| (2^-17 + 2^-22) + rstd64 (ulp(mean) + 2^-24 |mean|) (1 + 2^-17)."""
import ctypes
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import prepass_reference as pr

pytestmark = pytest.mark.gpu

EPS = 1e-5
GUARD = 80                  # bytes in front of a window: more than 64, and 16-byte aligned without being 32-byte aligned
GUARD_BYTE, FILL, PATTERN = 0xA5, 0xFF, 0x5C
RES_BOUND = 2.0 ** -21
STAT_BOUND = 2.0 ** -17
INVALID, UNSUPPORTED = -1, -2


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


# ------------------------------------------------------------------------------------------------------------ guarded windows

class Guarded:
    """`nbytes` at a 16-byte-aligned offset of a larger allocation, guard bytes on both sides, the window prefilled with `fill`."""

    def __init__(self, nbytes, dev, fill=FILL):
        self.nbytes, self.fill = nbytes, fill
        self.buf = torch.full((GUARD + nbytes + GUARD + 32,), GUARD_BYTE, dtype=torch.uint8, device=dev)
        self.off = GUARD + (-(self.buf.data_ptr() + GUARD)) % 16
        self.win = self.buf[self.off:self.off + nbytes]
        self.win.fill_(fill)
        assert self.win.data_ptr() % 16 == 0 and self.off >= 64 and self.buf.numel() - self.off - nbytes >= 64

    def ptr(self):
        return ctypes.c_void_p(self.win.data_ptr())

    def check(self, what, untouched=False):
        assert bool((self.buf[:self.off] == GUARD_BYTE).all()), what + ': wrote in front of a window'
        assert bool((self.buf[self.off + self.nbytes:] == GUARD_BYTE).all()), what + ': wrote behind a window'
        if untouched:
            assert bool((self.win == self.fill).all()), what + ': a refused call wrote to an output'

    def f32(self):
        return self.win.view(torch.float32).cpu()

    def raw(self):
        return self.win.cpu()


def _gptr(g):
    return g.ptr() if g is not None else ctypes.c_void_p(0)


def _dptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _apsrc(data, C, act=0, mean=None, rstd=None):
    from animateportrait_amd import _capi
    s = _capi.ApSrc()
    s.data = data.data_ptr()
    s.mean = mean.data_ptr() if mean is not None else None
    s.rstd = rstd.data_ptr() if rstd is not None else None
    s.C, s.act = C, act
    return s


def _xs_bytes(N, C, H, W):
    from animateportrait_amd import _capi
    return int(_capi.check(_capi.lib().ap_split_prepass_bytes(N, C, H, W), 'split_prepass_bytes'))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _ulp32(v64):
    return torch.from_numpy(np.spacing(np.abs(v64.numpy()).astype(np.float32)).astype(np.float64))


def _norm_split(dev, N, C, H, W, xd, act, flags, mean=None, rstd=None, partials=None, tiles=0, stats_out=True, res=None,
                want_y=True, want_xs=True, xs_fill=FILL, expect=0, src_c=None, xs_c=None):
    """One ap_norm_apply_split_ex call into guarded windows; the outputs on the CPU.  expect != 0: the call has to be refused with
    that code and to leave every window as it was."""
    from animateportrait_amd import ops, _capi
    what = 'norm_apply_split N=%d C=%d %dx%d act=%d flags=%d tiles=%d' % (N, C, H, W, act, flags, tiles)
    s = _apsrc(xd, src_c or C, act, mean, rstd)
    yb = Guarded(N * C * H * W * 4, dev) if want_y else None
    xb = Guarded(_xs_bytes(N, xs_c or C, H, W), dev, xs_fill) if want_xs else None
    mo = Guarded(N * C * 4, dev) if partials is not None and stats_out else None
    ro = Guarded(N * C * 4, dev) if partials is not None and stats_out else None
    rc = _capi.lib().ap_norm_apply_split_ex(ctypes.byref(s), _dptr(partials), tiles, EPS, _gptr(mo), _gptr(ro),
                                            ctypes.byref(res) if res is not None else None, N, H, W, _gptr(yb), _gptr(xb), flags,
                                            ops._stream())
    torch.cuda.synchronize()
    assert rc == expect, '%s: returned %d, expected %d' % (what, rc, expect)
    for b in (yb, xb, mo, ro):
        if b is not None:
            b.check(what, untouched=expect != 0)
    return SimpleNamespace(y=yb.f32().view(N, C, H, W) if yb else None, xs=xb.raw() if xb else None,
                           mean=mo.f32() if mo else None, rstd=ro.f32() if ro else None)


def _finalize(dev, partials, y, N, C, tiles, count, octet, expect=0):
    from animateportrait_amd import ops, _capi
    lib = _capi.lib()
    what = 'instnorm_finalize%s NC=%d tiles=%d count=%d' % ('_octet' if octet else '', N * C, tiles, count)
    mo, ro = Guarded(N * C * 4, dev), Guarded(N * C * 4, dev)
    if octet:
        rc = lib.ap_instnorm_finalize_octet(_dptr(partials), _dptr(y), N, C, tiles, count, EPS, mo.ptr(), ro.ptr(), ops._stream())
    else:
        rc = lib.ap_instnorm_finalize(_dptr(partials), _dptr(y), N * C, tiles, count, EPS, mo.ptr(), ro.ptr(), ops._stream())
    torch.cuda.synchronize()
    assert rc == expect, '%s: returned %d' % (what, rc)
    mo.check(what, untouched=expect != 0)
    ro.check(what, untouched=expect != 0)
    return mo.f32(), ro.f32()


# ------------------------------------------------------------------------------------------------------------ inputs

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _assert_stats(what, mean, rstd, x, planes=None):
    """mean / rstd as a kernel wrote them against the fp64 two-pass statistics of x (see the module's docstring)."""
    mean64, _, rstd64 = pr.stats64(x, EPS)
    assert not bool(torch.isnan(mean).any()) and not bool(torch.isnan(rstd).any()), what + ': a statistic was never written'
    dm = (mean.double() - mean64.float().double()).abs() - (_ulp32(mean64) + 2.0 ** -24 * mean64.abs())
    dr = (rstd.double() - rstd64).abs() / rstd64
    print('%s: mean excess %.3g, rstd rel %.3g (bound %.3g)' % (what, float(dm.max()), float(dr.max()), STAT_BOUND))
    assert float(dm.max()) <= 0.0, what + ': mean'
    assert float(dr.max()) <= STAT_BOUND, what + ': rstd'


def _assert_residual_bound(what, y, a64, b64):
    err = (y.double() - (a64 + b64)).abs()
    lim = RES_BOUND * (a64.abs() + b64.abs())
    print('%s: worst |y - ref| / (|a| + |b|) = %.3g (bound %.3g)' % (what, float((err / (a64.abs() + b64.abs() + 1e-300)).max()), RES_BOUND))
    assert bool((err <= lim).all()), what


# ------------------------------------------------------------------------------------------------------------ ap_norm_apply_split_ex

Case = namedtuple('Case', 'src res stats tiles act flags N C H W')

#        source  residual  statistics tiles act flags  N   C   H    W
PLANE_CASES = [
    # VEC = 1 (H*W % 4 != 0): 256 pixels per block
    Case('f32', 'none',  'part', 7,  1, 0, 1, 8,  1,  1),
    Case('f32', 'none',  'fin',  0,  2, 2, 3, 24, 27, 19),
    Case('f32', 'plain', 'none', 0,  0, 1, 3, 8,  1,  3),
    Case('f32', 'norm',  'part', 23, 0, 0, 1, 24, 1,  257),
    Case('f32', 'xs',    'fin',  0,  1, 3, 1, 8,  3,  85),
    Case('f32', 'xs',    'part', 9,  2, 0, 3, 8,  27, 19),
    Case('b16', 'none',  'part', 8,  2, 1, 1, 24, 3,  85),
    Case('b16', 'none',  'none', 0,  1, 0, 3, 8,  1,  257),
    Case('b16', 'plain', 'fin',  0,  1, 2, 1, 8,  1,  3),
    Case('b16', 'norm',  'part', 1,  0, 0, 3, 8,  27, 19),
    Case('b16', 'xs',    'none', 0,  0, 0, 3, 24, 1,  1),
    Case('b16', 'xs',    'part', 7,  1, 1, 1, 8,  1,  257),
    # VEC = 4: 1024 pixels per block
    Case('f32', 'none',  'part', 9,  1, 0, 3, 8,  2,  2),
    Case('f32', 'none',  'none', 0,  2, 1, 1, 24, 4,  257),
    Case('f32', 'plain', 'fin',  0,  2, 0, 1, 8,  4,  255),
    Case('f32', 'norm',  'part', 8,  1, 2, 3, 8,  4,  257),
    Case('f32', 'xs',    'none', 0,  0, 0, 1, 24, 32, 32),
    Case('f32', 'xs',    'part', 23, 1, 1, 1, 8,  4,  257),
    Case('b16', 'none',  'fin',  0,  1, 3, 3, 24, 32, 32),
    Case('b16', 'none',  'part', 1,  0, 0, 1, 8,  4,  257),
    Case('b16', 'plain', 'part', 7,  0, 0, 1, 8,  2,  2),
    Case('b16', 'norm',  'fin',  0,  2, 0, 3, 8,  4,  257),
    Case('b16', 'xs',    'part', 23, 2, 2, 1, 8,  4,  255),
    Case('b16', 'xs',    'fin',  0,  0, 1, 3, 8,  4,  257),
]
# the channel-octet form: 512 pixels per block
OCTET_CASES = [
    Case('oct', 'none',  'part', 7,  1, 0, 3, 8,  1,  1),
    Case('oct', 'xs',    'fin',  0,  2, 1, 1, 24, 1,  127),
    Case('oct', 'none',  'none', 0,  0, 2, 1, 8,  3,  43),
    Case('oct', 'xs',    'part', 9,  1, 0, 3, 8,  7,  73),
    Case('oct', 'none',  'part', 23, 2, 1, 1, 24, 27, 19),
    Case('oct', 'xs',    'none', 0,  0, 2, 3, 8,  32, 32),
    Case('oct', 'none',  'fin',  0,  1, 0, 1, 8,  32, 32),
    Case('oct', 'xs',    'part', 8,  2, 3, 1, 8,  27, 19),
]
RES_KIND = {'none': 0, 'plain': 1, 'norm': 1, 'xs': 2}


def _case_id(c):
    form = 'oct' if c.src == 'oct' else 'vec%d-%s' % (4 if (c.H * c.W) % 4 == 0 else 1, c.src)
    stats = c.stats + (str(c.tiles) if c.stats == 'part' else '')
    return '%s-res%d%s-%s-act%d-flags%d-n%dc%d-%dx%d' % (form, RES_KIND[c.res], c.res if c.res in ('plain', 'norm') else '', stats,
                                                         c.act, c.flags, c.N, c.C, c.H, c.W)


def test_case_table_covers_every_instantiation_and_axis():
    """The table, not the kernels: each of the 14 instantiations at a shape under and one over its block span, each flag and each
    statistics source with each form, every tile count and every shape of the plan."""
    seen = {}
    for c in PLANE_CASES + OCTET_CASES:
        hw = c.H * c.W
        form = 'oct' if c.src == 'oct' else ('v4' if hw % 4 == 0 else 'v1')
        span = {'oct': 512, 'v4': 1024, 'v1': 256}[form]
        seen.setdefault((form, c.src, RES_KIND[c.res]), set()).add(hw > span)
        seen.setdefault(('stats', form), set()).add(c.stats)
        seen.setdefault(('flags', form), set()).update(b for b in (1, 2) if c.flags & b)
        seen.setdefault(('shapes', form), set()).add((c.H, c.W))
        seen.setdefault('tiles', set()).update([c.tiles] if c.stats == 'part' else [])
        seen.setdefault('acts', set()).add(c.act)
        seen.setdefault('res', set()).add(c.res)
        assert c.N in (1, 3) and c.C in (8, 24)
    inst = [k for k in seen if isinstance(k, tuple) and len(k) == 3]
    assert len(inst) == 14 and all(seen[k] == {False, True} for k in inst)
    for form in ('v1', 'v4', 'oct'):
        assert seen[('stats', form)] == {'none', 'fin', 'part'} and seen[('flags', form)] == {1, 2}
    assert seen[('shapes', 'v1')] == {(1, 1), (1, 3), (3, 85), (1, 257), (27, 19)}
    assert seen[('shapes', 'v4')] == {(2, 2), (4, 255), (32, 32), (4, 257)}
    assert seen[('shapes', 'oct')] == {(1, 1), (1, 127), (3, 43), (7, 73), (27, 19), (32, 32)}
    assert seen['tiles'] == {1, 7, 8, 9, 23} and seen['acts'] == {0, 1, 2} and seen['res'] == {'none', 'plain', 'norm', 'xs'}
    assert len({_case_id(c) for c in PLANE_CASES + OCTET_CASES}) == len(PLANE_CASES + OCTET_CASES)


def _case_inputs(c):
    """The values of a case, made once and never modified: x (fp32; bf16-representable for a bf16 source), its statistics in the
    form the case hands over, and the residual."""
    def make():
        g = torch.Generator().manual_seed(1000 + (PLANE_CASES + OCTET_CASES).index(c))
        shape = (c.N, c.C, c.H, c.W)
        # with statistics: mean 2.5, deviation 1 (mean^2 / var about 6: the tile sums are well conditioned and of one sign);
        # a plain feature carries both signs by itself
        x = torch.randn(shape, generator=g) * 3 if c.stats == 'none' else torch.randn(shape, generator=g) + 2.5
        if c.src == 'b16':
            x = x.to(torch.bfloat16).float()
        d = SimpleNamespace(x=x, mean=None, rstd=None, partials=None, r=None)
        if c.stats == 'fin':
            m64, _, r64 = pr.stats64(x, EPS)
            d.mean, d.rstd = m64.float(), r64.float()
        elif c.stats == 'part':
            d.partials = pr.make_partials(x, c.tiles)
        if c.res != 'none':
            d.r = torch.randn(shape, generator=g) * 2 + 0.5
            if c.res == 'norm':
                m64, _, r64 = pr.stats64(d.r, EPS)
                d.rmean, d.rrstd = m64.float(), r64.float()
                d.b64 = (d.r.double() - d.rmean.double().view(c.N, c.C, 1, 1)) * d.rrstd.double().view(c.N, c.C, 1, 1)
            elif c.res == 'xs':
                head, tail = pr.split_encode(d.r)
                d.b64 = (head.float() + tail.float()).double()        # what the kernel reads: head + tail, added in fp32 (exact or not)
                d.r_xs = pr.pack_xs(d.r)
            else:
                d.b64 = d.r.double()
        return d
    return _cached(('ns', c), make)


def _launch_case(dev, c, d, src, flags, want_y, want_xs, xs_fill=FILL, stats_out=True):
    """The case's call with the source in layout `src` ('f32', 'b16', 'oct')."""
    xd = {'f32': lambda: d.x, 'b16': lambda: d.x.to(torch.bfloat16), 'oct': lambda: pr.to_octet(d.x)}[src]().contiguous().to(dev)
    flags = flags | {'f32': 0, 'b16': 8, 'oct': 16}[src]
    keep, res = [], None
    if c.res in ('plain', 'norm'):
        keep = [d.r.to(dev)] + ([d.rmean.to(dev), d.rrstd.to(dev)] if c.res == 'norm' else [])
        res = _apsrc(keep[0], c.C, 0, *keep[1:])
    elif c.res == 'xs':
        keep = [d.r_xs.to(dev)]
        res = _apsrc(keep[0], c.C)
        flags |= 4
    mean, rstd = (d.mean.to(dev), d.rstd.to(dev)) if d.mean is not None else (None, None)
    partials = d.partials.to(dev) if d.partials is not None else None
    return _norm_split(dev, c.N, c.C, c.H, c.W, xd, c.act, flags, mean, rstd, partials, c.tiles, stats_out, res, want_y, want_xs, xs_fill)


def _check_split_of(what, xs, v, relu, c):
    """xs is the split copy of v (of relu(v) under flags bit 1), byte for byte, every closing slot zero."""
    want = pr.pack_xs(torch.maximum(v, torch.zeros(())) if relu else v)
    _, _, closing = pr.unpack_xs(xs, c.N, c.C, c.H, c.W)
    assert int(closing.abs().max()) == 0, what + ': a closing slot is not zero'
    assert torch.equal(xs, want), what + ': xs is not the split copy of the result'


def _check_heads_only(what, dev, c, d, src, full_xs):
    """flags bit 0 over an xs prefilled with a pattern: the head planes are those of the full call, no pixel slot of a tail plane
    changes (the tail planes' closing slot is not asserted)."""
    got = _launch_case(dev, c, d, src, (c.flags & 2) | 1, False, True, xs_fill=PATTERN).xs
    hw = c.H * c.W
    got = got.view(c.N, 2, c.C // 8, hw + 1, 16)
    full = full_xs.view(c.N, 2, c.C // 8, hw + 1, 16)
    assert torch.equal(got[:, 0], full[:, 0]), what + ': heads-only changed a head plane'
    assert bool((got[:, 1, :, :hw] == PATTERN).all()), what + ': heads-only wrote a tail slot'


def _check_stats_written(what, dev, c, d, src, full):
    """Statistics from partial tiles: every entry written, bit-equal to the finalizer on the same tiles and data, within the
    bars of the fp64 statistics; a call without y and xs writes the same and nothing else."""
    _assert_stats(what, full.mean, full.rstd, d.x)
    pd = d.partials.to(dev)
    yd = (pr.to_octet(d.x) if src == 'oct' else d.x).contiguous().to(dev)
    fm, fr = _finalize(dev, pd, yd, c.N, c.C, c.tiles, c.H * c.W, src == 'oct')
    assert torch.equal(_bits(fm), _bits(full.mean)) and torch.equal(_bits(fr), _bits(full.rstd)), what + ': not the finalizer\'s statistics'
    if src != 'oct':          # (an octet source has no call without xs)
        bare = _launch_case(dev, c, d, src, 0, False, False)
        assert torch.equal(_bits(bare.mean), _bits(full.mean)) and torch.equal(_bits(bare.rstd), _bits(full.rstd)), what + ': plain finalize'


def _check_plane_call(what, dev, c, d, src):
    """The plane-layout call of a case, checked in full; returns the y + xs call's outputs."""
    relu = bool(c.flags & 2)
    full = _launch_case(dev, c, d, src, c.flags & 2, True, True)
    if c.stats == 'part':
        _check_stats_written(what, dev, c, d, src, full)
    mean, rstd = (full.mean, full.rstd) if c.stats == 'part' else (d.mean, d.rstd)
    assert not bool(torch.isnan(full.y).any()), what + ': an element of y was never written'
    if c.res == 'none':
        want = pr.norm_act(d.x, mean, rstd, c.act)
        assert torch.equal(_bits(full.y), _bits(want)), what + ': y is not the fp32 restatement, worst %g' % float((full.y - want).abs().max())
    else:
        a64 = pr.norm_act(d.x, mean, rstd, c.act, dtype=torch.float64, slope=pr.SLOPE32)
        _assert_residual_bound(what, full.y, a64, d.b64)
    _check_split_of(what, full.xs, full.y, relu, c)
    xs_only = _launch_case(dev, c, d, src, c.flags & 2, False, True)
    assert torch.equal(xs_only.xs, full.xs), what + ': xs alone differs from xs with y'
    y_only = _launch_case(dev, c, d, src, c.flags & 2, True, False)
    assert torch.equal(_bits(y_only.y), _bits(full.y)), what + ': y alone differs from y with xs'
    if c.stats == 'part':
        assert torch.equal(_bits(xs_only.mean), _bits(full.mean)) and torch.equal(_bits(y_only.rstd), _bits(full.rstd))
    return full


@pytest.mark.parametrize('c', PLANE_CASES, ids=_case_id)
def test_norm_apply_split_plane(dev, c):
    d = _case_inputs(c)
    what = _case_id(c)
    full = _check_plane_call(what, dev, c, d, c.src)
    if c.flags & 1:
        _check_heads_only(what, dev, c, d, c.src, full.xs)


@pytest.mark.parametrize('c', OCTET_CASES, ids=_case_id)
def test_norm_apply_split_octet(dev, c):
    """The channel-octet form gives the split copy only: it is the plane-layout call's on the same values byte for byte (that
    call is checked in full here, y included), and without a residual the split copy of the fp32 restatement itself."""
    d = _case_inputs(c)
    what = _case_id(c)
    relu = bool(c.flags & 2)
    got = _launch_case(dev, c, d, 'oct', c.flags & 2, False, True)
    if c.stats == 'part':
        _check_stats_written(what, dev, c, d, 'oct', got)
    mean, rstd = (got.mean, got.rstd) if c.stats == 'part' else (d.mean, d.rstd)
    if c.res == 'none':
        _check_split_of(what, got.xs, pr.norm_act(d.x, mean, rstd, c.act), relu, c)
    plane = _check_plane_call(what + ' (plane layout)', dev, c, d, 'f32')
    if c.stats == 'part':
        assert torch.equal(_bits(plane.mean), _bits(got.mean)) and torch.equal(_bits(plane.rstd), _bits(got.rstd))
    _, _, closing = pr.unpack_xs(got.xs, c.N, c.C, c.H, c.W)
    assert int(closing.abs().max()) == 0, what + ': a closing slot is not zero'
    assert torch.equal(got.xs, plane.xs), what + ': the octet form differs from the plane form'
    if c.flags & 1:
        _check_heads_only(what, dev, c, d, 'oct', got.xs)


# ---- ill-conditioned planes

RATIOS = [1.0, 20.0, 50.0, 1.0e6, 1.0e6, 1.0, 50.0, 20.0]       # mean^2 / var of the 8 channels of every group


def _ill_inputs(H, W, b16):
    def make():
        N, C, hw = 2, 16, H * W
        rng = np.random.default_rng(77 + hw)
        z = rng.standard_normal((N, C, hw))
        z = (z - z.mean(2, keepdims=True)) / z.std(2, keepdims=True)
        sign = np.where(np.arange(C) < 8, 1.0, -1.0)[None, :, None]
        x = torch.from_numpy((sign * 1.00037 * np.sqrt(np.array(RATIOS * 2))[None, :, None] + z).astype(np.float32)).reshape(N, C, H, W)
        if b16:
            x = x.to(torch.bfloat16).float()
        return x, pr.make_partials(x, 9)
    return _cached(('ill', H, W, b16), make)


@pytest.mark.parametrize('H,W', [(7, 73), (32, 32)], ids=['7x73-vec1-oct_under', '32x32-vec4-oct_over'])
def test_ill_conditioned_planes_are_recomputed_from_the_data(dev, H, W):
    N, C, hw = 2, 16, H * W
    bad = torch.tensor([r > 1e5 for r in RATIOS * 2 * N])
    for src in ('f32', 'b16', 'oct'):
        x, partials = _ill_inputs(H, W, src == 'b16')
        what = 'ill-conditioned %dx%d %s' % (H, W, src)
        mean64, var64, rstd64 = pr.stats64(x, EPS)
        # what skipping the recompute would give on these very planes: far outside the bar.  (Not so from bf16 data: values of 8
        # significant bits have tile sums that fp32 holds exactly, so there the recompute runs -- the decision is the same -- and
        # a wrong one, a wrong stride say, fails the bar, but a skipped one would not.)
        _, rstd_u = pr.unrefined_stats(partials, hw, EPS)
        if src != 'b16':
            assert float(((rstd_u - rstd64).abs() / rstd64)[bad].max()) > 100 * STAT_BOUND
        c = Case(src, 'none', 'part', 9, 0, 0, N, C, H, W)
        d = SimpleNamespace(x=x, mean=None, rstd=None, partials=partials, r=None)
        got = _launch_case(dev, c, d, src, 0, src != 'oct', True)
        _assert_stats(what, got.mean, got.rstd, x)
        if src == 'oct':
            plane = _launch_case(dev, c, d, 'f32', 0, True, True)
            assert torch.equal(got.xs, plane.xs), what + ': the octet form differs from the plane form'
            assert torch.equal(_bits(got.mean), _bits(plane.mean)) and torch.equal(_bits(got.rstd), _bits(plane.rstd))
        else:
            y64 = pr.norm_act(x, mean64, rstd64, 0, dtype=torch.float64)
            lim = y64.abs() * (2.0 ** -17 + 2.0 ** -22) + (rstd64 * (_ulp32(mean64) + 2.0 ** -24 * mean64.abs()) * (1 + 2.0 ** -17)).view(N, C, 1, 1)
            err = (got.y.double() - y64).abs()
            print('%s: worst err / bound = %.3g' % (what, float((err / lim).max())))
            assert bool((err <= lim).all()), what + ': y of an ill-conditioned plane'
            _check_split_of(what, got.xs, got.y, False, c)
        if src != 'b16':
            pd = partials.to(dev)
            yd = (pr.to_octet(x) if src == 'oct' else x).contiguous().to(dev)
            fm, fr = _finalize(dev, pd, yd, N, C, 9, hw, src == 'oct')
            _assert_stats(what + ' finalizer', fm, fr, x)
            assert torch.equal(_bits(fm), _bits(got.mean)) and torch.equal(_bits(fr), _bits(got.rstd)), what + ': finalizer differs'


# ------------------------------------------------------------------------------------------------------------ the finalizers

@pytest.mark.parametrize('count', [1, 3, 513])
@pytest.mark.parametrize('tiles', [1, 63, 64, 65, 130])
def test_instnorm_finalize(dev, tiles, count):
    """Plane and channel-octet form (C = 24: c >> 3 and c & 7 both vary) over the 64-lane tile loop's edges.  Without y: the
    unrefined formula, to one fp32 rounding (2^-24) plus the association of the fp64 expression (another 2^-24 allowed).  With y:
    the bars of the fp64 statistics, planes of |mean| = 100 deviations among the others."""
    N, C = 2, 24

    def make():
        g = torch.Generator().manual_seed(500 + count)
        x = torch.randn(N, C, 1, count, generator=g) + 2.5
        x[:, 5::7] += 97.5
        return x, pr.make_partials(x, tiles)
    x, partials = _cached(('fin', tiles, count), make)
    what = 'finalize tiles=%d count=%d' % (tiles, count)
    pd = partials.to(dev)
    mean_u, rstd_u = pr.unrefined_stats(partials, count, EPS)
    m0, r0 = _finalize(dev, pd, None, N, C, tiles, count, False)
    assert float(((m0.double() - mean_u).abs() / mean_u.abs()).max()) <= 2.0 ** -23, what + ': unrefined mean'
    assert float(((r0.double() - rstd_u).abs() / rstd_u).max()) <= 2.0 ** -23, what + ': unrefined rstd'
    m0o, r0o = _finalize(dev, pd, None, N, C, tiles, count, True)
    assert torch.equal(_bits(m0o), _bits(m0)) and torch.equal(_bits(r0o), _bits(r0)), what + ': octet form without y'
    m1, r1 = _finalize(dev, pd, x.contiguous().to(dev), N, C, tiles, count, False)
    _assert_stats(what, m1, r1, x)
    m2, r2 = _finalize(dev, pd, pr.to_octet(x).to(dev), N, C, tiles, count, True)
    assert torch.equal(_bits(m2), _bits(m1)) and torch.equal(_bits(r2), _bits(r1)), what + ': octet form differs from the plane form'


# ------------------------------------------------------------------------------------------------------------ ap_instnorm_apply

def _apply(dev, x, mean, rstd, act, res, rmean, rrstd, NC, HW, expect=0):
    from animateportrait_amd import ops, _capi
    what = 'instnorm_apply NC=%d HW=%d act=%d' % (NC, HW, act)
    t = [v.to(dev) if v is not None else None for v in (x, mean, rstd, res, rmean, rrstd)]
    out = Guarded(x.numel() * 4, dev)
    rc = _capi.lib().ap_instnorm_apply(_dptr(t[0]), _dptr(t[1]), _dptr(t[2]), act, _dptr(t[3]), _dptr(t[4]), _dptr(t[5]), out.ptr(),
                                       NC, HW, ops._stream())
    torch.cuda.synchronize()
    assert rc == expect, '%s: returned %d, expected %d' % (what, rc, expect)
    out.check(what, untouched=expect != 0)
    return out.f32()


@pytest.mark.parametrize('act', [0, 1, 2])
@pytest.mark.parametrize('res', ['none', 'plain', 'norm'])
@pytest.mark.parametrize('NC,HW', [(5, 4), (5, 1028), (1, 65540)], ids=['nc5-hw4', 'nc5-hw1028', 'nc1-hw65540'])
def test_instnorm_apply(dev, NC, HW, res, act):
    """HW = 4 * (64 * 256 + 1) is the first plane at which the grid cap of 64 blocks makes a thread take a second float4."""
    def make():
        g = torch.Generator().manual_seed(600 + HW)
        x = torch.randn(1, NC, 1, HW, generator=g) + 2.5
        r = torch.randn(1, NC, 1, HW, generator=g) * 2 + 0.5
        return x, r, [s.float() for s in pr.stats64(x, EPS)], [s.float() for s in pr.stats64(r, EPS)]
    x, r, (mean, _, rstd), (rmean, _, rrstd) = _cached(('apply', NC, HW), make)
    what = 'instnorm_apply NC=%d HW=%d res=%s act=%d' % (NC, HW, res, act)
    y = _apply(dev, x, mean, rstd, act, r if res != 'none' else None, rmean if res == 'norm' else None,
               rrstd if res == 'norm' else None, NC, HW).view(1, NC, 1, HW)
    assert not bool(torch.isnan(y).any()), what + ': an element was never written'
    if res == 'none':
        want = pr.norm_act(x, mean, rstd, act)
        assert torch.equal(_bits(y), _bits(want)), what + ': worst %g' % float((y - want).abs().max())
    else:
        a64 = pr.norm_act(x, mean, rstd, act, dtype=torch.float64, slope=pr.SLOPE32)
        b64 = r.double() if res == 'plain' else (r.double() - rmean.double().view(1, NC, 1, 1)) * rrstd.double().view(1, NC, 1, 1)
        _assert_residual_bound(what, y, a64, b64)


# ------------------------------------------------------------------------------------------------------------ the split copies

def _rows(dev, x, mean, rstd, act, N, C, H, W, K=7, pad=3, pad_mode=0, expect=0):
    from animateportrait_amd import ops, _capi
    what = 'split_prepass_rows N=%d C=%d %dx%d K=%d pad_mode=%d act=%d' % (N, C, H, W, K, pad_mode, act)
    t = [v.to(dev) if v is not None else None for v in (x, mean, rstd)]
    out = Guarded(_xs_bytes(N, pr.ROW_CHANNELS, H, W), dev)
    s = _apsrc(t[0], C, act, t[1], t[2])
    rc = _capi.lib().ap_split_prepass_rows(ctypes.byref(s), N, H, W, K, pad, pad_mode, out.ptr(), ops._stream())
    torch.cuda.synchronize()
    assert rc == expect, '%s: returned %d, expected %d' % (what, rc, expect)
    out.check(what, untouched=expect != 0)
    return out.raw()


def _virtual(x, act):
    """(mean, rstd, act) of a virtual source (act 1 / 2: finished statistics) or (None, None, 0) of a plain one (act None)."""
    if act is None:
        return None, None, 0
    m64, _, r64 = pr.stats64(x, EPS)
    return m64.float(), r64.float(), act


#  C  H  W    pad_mode  act of a virtual source (None: a plain one)
ROWS_CASES = [
    (1, 1, 255, 0, None), (2, 1, 257, 0, 1), (3, 2, 128, 0, 2), (4, 3, 85, 0, None), (1, 3, 86, 0, 1), (3, 7, 37, 0, 1),
    (1, 7, 5, 0, 2), (2, 4, 64, 1, None), (4, 4, 65, 1, 2), (3, 7, 37, 1, 1), (2, 7, 36, 1, None),
]


@pytest.mark.parametrize('C,H,W,pad_mode,act', ROWS_CASES,
                         ids=['c%d-%dx%d-%s-%s' % (c, h, w, 'reflect' if p else 'zero', 'plain' if a is None else 'virtual_act%d' % a)
                              for c, h, w, p, a in ROWS_CASES])
def test_split_prepass_rows(dev, C, H, W, pad_mode, act):
    N = 3
    x = _cached(('rows', C, H, W), lambda: torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(700 + C * H * W)) + 0.75)
    mean, rstd, a = _virtual(x, act)
    raw = _rows(dev, x, mean, rstd, a, N, C, H, W, pad_mode=pad_mode)
    want = pr.pack_xs(pr.rows_expand(pr.norm_act(x, mean, rstd, a), pad_mode))
    head, tail, closing = pr.unpack_xs(raw, N, pr.ROW_CHANNELS, H, W)
    assert not bool(torch.isnan(head).any()) and not bool(torch.isnan(tail).any()), 'a slot was never written'
    assert closing.shape == (N, 2, 4, 8) and int(closing.abs().max()) == 0, 'a closing slot is not zero'
    past = raw.view(N, 2, 4, H * W + 1, 8, 2).permute(0, 1, 3, 2, 4, 5).reshape(N, 2, H * W + 1, 32, 2)[:, :, :, 7 * C:]
    assert int(past.max()) == 0, 'a channel past 7 * C is not zero'
    assert torch.equal(raw, want)


S2D_CASES = [(8, 2, 2, None), (24, 2, 30, 1), (8, 30, 2, 2), (24, 14, 36, None), (8, 14, 36, 2), (8, 30, 32, 1), (24, 30, 32, None)]


@pytest.mark.parametrize('C,H,W,act', S2D_CASES,
                         ids=['c%d-%dx%d-%s' % (c, h, w, 'plain' if a is None else 'virtual_act%d' % a) for c, h, w, a in S2D_CASES])
def test_split_prepass_s2d(dev, C, H, W, act):
    from animateportrait_amd import ops, _capi
    N, H2, W2 = 3, H // 2 + 1, W // 2 + 1
    x = _cached(('s2d', C, H, W), lambda: torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(800 + C * H * W)) + 0.75)
    mean, rstd, a = _virtual(x, act)
    t = [v.to(dev) if v is not None else None for v in (x, mean, rstd)]
    out = Guarded(_xs_bytes(N, 4 * C, H2, W2), dev)
    s = _apsrc(t[0], C, a, t[1], t[2])
    _capi.check(_capi.lib().ap_split_prepass_s2d(ctypes.byref(s), N, H, W, out.ptr(), ops._stream()), 'split_prepass_s2d')
    torch.cuda.synchronize()
    out.check('split_prepass_s2d')
    raw = out.raw()
    head, tail, closing = pr.unpack_xs(raw, N, 4 * C, H2, W2)
    assert int(closing.abs().max()) == 0, 'a closing slot is not zero'
    ring = pr.s2d_expand(torch.ones(N, C, H, W)) == 0
    assert int(ring.sum()) == N * 4 * C * (H2 * W2 - (H // 2) * (W // 2))
    hb, tb = head.to(torch.bfloat16).view(torch.int16), tail.to(torch.bfloat16).view(torch.int16)
    assert int(hb[ring].abs().max()) == 0 and int(tb[ring].abs().max()) == 0, 'the padding ring is not zero'
    assert torch.equal(raw, pr.pack_xs(pr.s2d_expand(pr.norm_act(x, mean, rstd, a))))


# ------------------------------------------------------------------------------------------------------------ refusals

def _refusal_norm_split(dev, name):
    N, C, H, W = 1, 8, 4, 4
    z = lambda *s: torch.ones(*s, device=dev)           # noqa: E731
    x, st, part = z(N, 16, H, W), z(16), z(16, 2, 2)
    kw = dict(act=0, flags=0, mean=None, rstd=None, partials=None, tiles=0, stats_out=True, res=None, want_y=True, want_xs=True,
              src_c=None, xs_c=None)
    code = INVALID
    if name == 'C=12':
        kw.update(src_c=12, xs_c=16)
    elif name == 'act=3':
        kw.update(act=3)
    elif name == 'finished and partial statistics':
        kw.update(mean=st, rstd=st, partials=part, tiles=2)
    elif name == 'partial tiles without mean_out':
        kw.update(partials=part, tiles=2, stats_out=False)
    elif name == 'tiles=0':
        kw.update(partials=part, tiles=0)
    elif name == 'activated residual':
        kw.update(res=_apsrc(x, C, 1))
    elif name == 'residual of another C':
        kw.update(res=_apsrc(x, 16, 0))
    elif name == 'split-copy residual with statistics':
        kw.update(res=_apsrc(x, C, 0, st, st), flags=4)
    elif name == 'octet source with y':
        kw.update(flags=16)
        code = UNSUPPORTED
    elif name == 'octet source with a plain fp32 residual':
        kw.update(flags=16, want_y=False, res=_apsrc(x, C, 0))
        code = UNSUPPORTED
    elif name == 'octet source of bf16 values':
        kw.update(flags=16 | 8, want_y=False)
        code = UNSUPPORTED
    else:
        raise AssertionError(name)
    _norm_split(dev, N, C, H, W, x, expect=code, **kw)


NORM_SPLIT_REFUSALS = ['C=12', 'act=3', 'finished and partial statistics', 'partial tiles without mean_out', 'tiles=0',
                       'activated residual', 'residual of another C', 'split-copy residual with statistics', 'octet source with y',
                       'octet source with a plain fp32 residual', 'octet source of bf16 values']


@pytest.mark.parametrize('name', NORM_SPLIT_REFUSALS, ids=[n.replace(' ', '_') for n in NORM_SPLIT_REFUSALS])
def test_norm_apply_split_refuses(dev, name):
    _refusal_norm_split(dev, name)


@pytest.mark.parametrize('name,C,H,K,pad_mode,act,lone_mean,code', [
    ('K=5', 3, 8, 5, 0, 0, False, UNSUPPORTED), ('C=5', 5, 8, 7, 0, 0, False, UNSUPPORTED), ('reflection with H=3', 3, 3, 7, 1, 0, False, INVALID),
    ('a lone mean', 3, 8, 7, 0, 0, True, INVALID), ('act=3', 3, 8, 7, 0, 3, False, INVALID), ('act=-1', 3, 8, 7, 0, -1, False, INVALID)],
    ids=['K5', 'C5', 'reflect_H3', 'lone_mean', 'act3', 'act_minus1'])
def test_split_prepass_rows_refuses(dev, name, C, H, K, pad_mode, act, lone_mean, code):
    x = torch.ones(1, 8, H, 8)
    _rows(dev, x, torch.ones(8) if lone_mean else None, None, act, 1, C, H, 8, K=K, pad=3 if K == 7 else 2, pad_mode=pad_mode, expect=code)


@pytest.mark.parametrize('name,C,H,act,code', [('odd H', 8, 5, 0, UNSUPPORTED), ('C=12', 12, 4, 0, UNSUPPORTED), ('act=3', 8, 4, 3, INVALID)],
                         ids=['odd_H', 'C12', 'act3'])
def test_split_prepass_s2d_refuses(dev, name, C, H, act, code):
    from animateportrait_amd import ops, _capi
    x = torch.ones(1, 16, 6, 4, device=dev)
    out = Guarded(_xs_bytes(1, 64, 4, 3), dev)
    s = _apsrc(x, C, act)
    rc = _capi.lib().ap_split_prepass_s2d(ctypes.byref(s), 1, H, 4, out.ptr(), ops._stream())
    torch.cuda.synchronize()
    assert rc == code, '%s: returned %d' % (name, rc)
    out.check(name, untouched=True)


@pytest.mark.parametrize('name,NC,HW,act,res_stats,code', [
    ('HW=6', 2, 6, 0, False, UNSUPPORTED), ('HW=2', 2, 2, 0, False, UNSUPPORTED), ('act=3', 2, 8, 3, False, INVALID),
    ('residual statistics without a residual', 2, 8, 0, True, INVALID), ('NC=65536', 65536, 8, 0, False, UNSUPPORTED)],
    ids=['HW6', 'HW2', 'act3', 'res_stats_without_res', 'NC65536'])
def test_instnorm_apply_refuses(dev, name, NC, HW, act, res_stats, code):
    x, st = torch.ones(64), torch.ones(8)
    _apply(dev, x, st, st, act, None, st if res_stats else None, st if res_stats else None, NC, HW, expect=code)


def test_instnorm_finalize_refuses_zero_tiles(dev):
    pd = torch.ones(16, 2, 2, device=dev)
    _finalize(dev, pd, None, 2, 8, 0, 4, False, expect=INVALID)
    _finalize(dev, pd, None, 2, 8, 0, 4, True, expect=INVALID)
