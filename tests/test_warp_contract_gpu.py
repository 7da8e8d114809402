"""GPU (-m gpu): the feature-warp kernels of csrc/warp_fwd.hip and csrc/warp_bwd.hip -- warp_concat_kernel (forward gather: four layouts, three activations, two
pixel-to-thread mappings), warp_concat_bwd_tiled_kernel (LDS-window scatter) and warp_concat_bwd_kernel (APAMD_WARP_BWD_PLAIN=1) --
held to the C contract "any N, C, H, W, S >= 1" at ragged, degenerate and non-square shapes and on hostile sampling maps, each
against the float64 reference of tests/warp_reference.py.

Every output (out, xs, dx) is a window inside a larger buffer filled with a sentinel, and the window itself is filled with NaN
before the launch: the sentinel has to survive, and no NaN may (a block that never ran, a store that was skipped; dx "zeroed inside").

Bars.  They are calibrated per case from the reference alone, on the same inputs.  With e_ref = max |ref_fp32 - ref_fp64| (torch in
fp32 against torch in fp64) over the compared pixels:
    forward    |kernel - ref64| <= 4 * e_ref + 1e-6
    backward   |dx - ref64|     <= 4 * e_ref + 2^-20 * A   elementwise, A = the sum of the absolute contributions of the element
The 4 covers a different association of the same fp32 formulas (bilerp, unfused pair arithmetic); 2^-20 * A is 16 ulp of the
absolute sum, which bounds any summation order of the scatter.  The mask threshold is the operator's only discontinuity: the flow half
is not compared (forward) / carries no gradient (backward) at the pixels warp_reference.ambiguous names, at most 0.5 % per case."""
import ctypes

import pytest
import torch

import warp_reference as wr

pytestmark = pytest.mark.gpu

SENT = 1e30
PAD = 64            # floats of sentinel around an fp32 window (256 bytes: the window keeps any alignment the kernels rely on)
XS_PAD = 256        # bytes of sentinel around a split-bf16 window
XS_SENT, XS_NAN = 0xA5, 0xFF        # (a bf16 of two 0xFF bytes is a NaN)


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


# ------------------------------------------------------------------------------------------------------------ launches

def _window(numel, dev):
    buf = torch.full((numel + 2 * PAD,), SENT, dtype=torch.float32, device=dev)
    win = buf[PAD:PAD + numel]
    win.fill_(float('nan'))
    return buf, win


def _assert_band(buf, numel, what):
    assert bool((buf[:PAD] == SENT).all()) and bool((buf[PAD + numel:] == SENT).all()), '%s: wrote outside its window' % what


def _xs_window(nbytes, dev):
    buf = torch.full((nbytes + 2 * XS_PAD,), XS_SENT, dtype=torch.uint8, device=dev)
    win = buf[XS_PAD:XS_PAD + nbytes]
    win.fill_(XS_NAN)
    return buf, win


def _assert_xs_band(buf, nbytes, what):
    assert bool((buf[:XS_PAD] == XS_SENT).all()) and bool((buf[XS_PAD + nbytes:] == XS_SENT).all()), '%s: wrote outside xs' % what


def _octet(x):
    """NCHW -> the channel-octet layout [N][C/8][H*W][8]."""
    n, c, h, w = x.shape
    return x.view(n, c // 8, 8, h * w).permute(0, 1, 3, 2).contiguous()


def _fwd(dev, x, stats, act, maps, shape, want_out=True, want_xs=False, flags=0):
    """ap_warp_concat_fwd_ex through ctypes.  (out [N,2C,H,W] on the CPU or None, the xs bytes on the device or None)."""
    from animateportrait_amd import ops, _capi
    lib = _capi.lib()
    N, C, H, W, S, fs = shape
    what = 'warp fwd %s act=%d flags=%d' % (shape, act, flags)
    xd = x.to(dev)
    if flags & 2:
        xd = _octet(xd)
    mean, rstd = (t.to(dev) for t in stats) if stats is not None else (None, None)
    mo, fl, mk = (t.to(dev) for t in maps)
    obuf = o = xbuf = xs = None
    if want_out:
        obuf, o = _window(N * 2 * C * H * W, dev)
    if want_xs:
        xshape = (N, 8 * C, H // 2 + 1, W // 2 + 1) if flags & 1 else (N, 2 * C, H, W)
        nbytes = int(_capi.check(lib.ap_split_prepass_bytes(*xshape), 'split_prepass_bytes'))
        xbuf, xs = _xs_window(nbytes, dev)
    _capi.check(lib.ap_warp_concat_fwd_ex(ops._ptr(xd), ops._ptr(mean), ops._ptr(rstd), act, ops._ptr(mo), ops._ptr(fl), ops._ptr(mk),
                                          ops._ptr(o), ops._ptr(xs), N, C, H, W, S, fs, flags, ops._stream()), what)
    torch.cuda.synchronize()
    out = None
    if want_out:
        _assert_band(obuf, o.numel(), what)
        out = o.view(N, 2 * C, H, W).cpu()
        assert not bool(torch.isnan(out).any()), what + ': an element of out was never written'
    if want_xs:
        _assert_xs_band(xbuf, xs.numel(), what)
        xs = xs.clone()
    return out, xs


def _bwd(dev, gout, maps, shape):
    """ap_warp_concat_bwd through ctypes into a NaN-filled window: dx [N,C,H,W] on the CPU."""
    from animateportrait_amd import ops, _capi
    N, C, H, W, S, fs = shape
    what = 'warp bwd %s' % (shape,)
    mo, fl, mk = (t.to(dev) for t in maps)
    gd = gout.to(dev)
    dbuf, d = _window(N * C * H * W, dev)
    _capi.check(_capi.lib().ap_warp_concat_bwd(ops._ptr(gd), ops._ptr(mo), ops._ptr(fl), ops._ptr(mk), ops._ptr(d), N, C, H, W, S, fs,
                                               ops._stream()), what)
    torch.cuda.synchronize()
    _assert_band(dbuf, d.numel(), what)
    dx = d.view(N, C, H, W).cpu()
    assert not bool(torch.isnan(dx).any()), what + ': dx is not written everywhere'
    return dx


# ------------------------------------------------------------------------------------------------------------ inputs and references

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _inputs(name, kind, shape):
    """x, statistics, maps, the float64 resized mask and the ambiguous pixels of a case (made once, never modified)."""
    def make():
        N, C, H, W, S, fs = shape
        seed = wr.case_seed(name, kind)
        maps = wr.case_maps(kind, shape, seed)
        g = torch.Generator().manual_seed(seed + 1)
        x = torch.randn(N, C, H, W, generator=g) * 3 + 1
        mean = x.mean((2, 3)).reshape(-1)
        rstd = 1.0 / torch.sqrt(x.var((2, 3), unbiased=False).reshape(-1) + 1e-5) if H * W > 1 else torch.ones(N * C)
        gout = torch.randn(N, 2 * C, H, W, generator=g)
        _, _, m64 = wr.resized_maps(*maps, H, W, fs, torch.float64)
        amb = wr.ambiguous(m64)
        share = float(amb.double().mean())
        assert share <= wr.MAX_EXCLUDED, (name, kind, share)
        return dict(x=x, stats=(mean, rstd), maps=maps, m64=m64, amb=amb, share=share, gout=gout)
    return _cached(('in', name, kind, shape), make)


def _fwd_refs(name, kind, shape, act, with_stats):
    """(ref64, ref32, compared [N,2C,H,W] bool) of the forward on act(IN(x)) (or on x itself)."""
    def make():
        N, C, H, W, S, fs = shape
        d = _inputs(name, kind, shape)
        refs = []
        for dtype in (torch.float64, torch.float32):
            xin = wr.instance_norm_act(d['x'], *d['stats'], act, dtype) if with_stats else d['x'].to(dtype)
            refs.append(wr.warp_concat_ref(xin, *d['maps'], H, W, fs, dtype)[0])
        cmp = torch.ones(N, 2 * C, H, W, dtype=torch.bool)
        cmp[:, C:] &= ~d['amb']
        return refs[0], refs[1], cmp
    return _cached(('fwd', name, kind, shape, act, with_stats), make)


def _check_fwd(label, out, ref64, ref32, cmp):
    e_ref = float((ref32.double() - ref64).abs()[cmp].max())
    err = float((out.double() - ref64).abs()[cmp].max())
    print('fwd %-28s e_ref = %.3e  |kernel - ref64| = %.3e  excluded = %.2e' % (label, e_ref, err, 1.0 - float(cmp.double().mean())))
    assert err <= 4 * e_ref + 1e-6, (label, err, e_ref)


def _bwd_refs(name, kind, shape, gout_fix=None):
    """(gout as launched, ref64, e_ref, A): the gradient with its flow half zeroed at ambiguous pixels, and the bar's ingredients."""
    def make():
        N, C, H, W, S, fs = shape
        d = _inputs(name, kind, shape)
        gout = d['gout'].clone()
        if gout_fix is not None:
            gout_fix(gout, C)
        gout[:, C:] *= (~d['amb']).float()
        ref64 = wr.warp_concat_bwd_ref(gout, *d['maps'], fs, torch.float64)
        ref32 = wr.warp_concat_bwd_ref(gout, *d['maps'], fs, torch.float32)
        return gout, ref64, float((ref32.double() - ref64).abs().max()), wr.abs_mass(gout, *d['maps'], fs)
    return _cached(('bwd', name, kind, shape), make)


def _check_bwd(label, dx, ref64, e_ref, A):
    diff = (dx.double() - ref64).abs()
    bar = 4 * e_ref + 2.0 ** -20 * A
    worst = float((diff - bar).max())
    print('bwd %-28s e_ref = %.3e  max|dx - ref64| = %.3e  max A = %.3e  max(diff - bar) = %.3e'
          % (label, e_ref, float(diff.max()), float(A.max()), worst))
    assert worst <= 0.0, (label, float(diff.max()), e_ref, worst)


SHAPE_KIND = [(n, k) for n in wr.SHAPES for k in wr.FWD_KINDS]
MODES = ['tiled', 'plain']


def _set_mode(monkeypatch, mode):
    if mode == 'plain':
        monkeypatch.setenv('APAMD_WARP_BWD_PLAIN', '1')        # read by the library on every call
    else:
        monkeypatch.delenv('APAMD_WARP_BWD_PLAIN', raising=False)


# ------------------------------------------------------------------------------------------------------------ forward

@pytest.mark.parametrize('name,kind', SHAPE_KIND, ids=['%s-%s' % nk for nk in SHAPE_KIND])
def test_forward_at_ragged_shapes(dev, name, kind):
    """The plain fp32 forward at every shape of warp_reference.SHAPES on smooth, noisy and out-of-frame maps; the two pyramid
    levels of an S = 40 model go through ops.warp_concat, everything else through the C entry point."""
    from animateportrait_amd import ops
    shape = wr.SHAPES[name]
    N, C, H, W, S, fs = shape
    d = _inputs(name, kind, shape)
    ref64, ref32, cmp = _fwd_refs(name, kind, shape, 0, False)
    if name in wr.LEVEL_OF:
        out = ops.warp_concat(ops.Feat(d['x'].to(dev)), *(t.to(dev) for t in d['maps']), wr.LEVEL_OF[name]).data.cpu()
        assert fs == 1.0 / (1 << wr.LEVEL_OF[name]) and tuple(out.shape) == (N, 2 * C, H, W)
    else:
        out, _ = _fwd(dev, d['x'], None, 0, d['maps'], shape)
    _check_fwd('%s-%s' % (name, kind), out, ref64, ref32, cmp)
    # the masked-out pixels carry exactly -1 in every channel of the flow half
    off = (d['m64'] <= 0.5) & ~d['amb']
    assert bool((out[:, C:][off.expand(N, C, H, W)] == -1.0).all())


@pytest.mark.parametrize('act', [0, 1, 2])
@pytest.mark.parametrize('name', list(wr.SHAPES))
def test_forward_of_virtual_feature(dev, name, act):
    """x_mean / x_rstd with every activation, against the reference applied to act(instance_norm(x)) materialised in float64: the
    full-octet vector path (C = 8) and the scalar tail-channel path (C = 9, 5, 7, 4, 3), LeakyReLU included."""
    from animateportrait_amd import ops
    shape = wr.SHAPES[name]
    d = _inputs(name, 'noise', shape)
    ref64, ref32, cmp = _fwd_refs(name, 'noise', shape, act, True)
    if name in wr.LEVEL_OF:
        f = ops.Feat(d['x'].to(dev), d['stats'][0].to(dev), d['stats'][1].to(dev), act)
        out = ops.warp_concat(f, *(t.to(dev) for t in d['maps']), wr.LEVEL_OF[name]).data.cpu()
    else:
        out, _ = _fwd(dev, d['x'], d['stats'], act, d['maps'], shape)
    _check_fwd('%s-noise act=%d' % (name, act), out, ref64, ref32, cmp)


def _decode_split(xs, n, c, h, w):
    """XS[n][head|tail][c/8][h*w + 1][8 x bf16] -> (head + tail as fp32 NCHW, the closing slots), as test_gpu_parity decodes it."""
    t = xs.view(torch.bfloat16).view(n, 2, c // 8, h * w + 1, 8).float()
    val = (t[:, 0] + t[:, 1])[:, :, :h * w]
    return val.permute(0, 1, 3, 2).reshape(n, c, h, w), t[:, :, :, h * w]


@pytest.mark.parametrize('name', list(wr.SPLIT_SHAPES))
def test_split_output_alone_and_with_fp32(dev, name):
    """xs alone and xs together with out: head + tail is the fp32 output to 2^-16 relative, every closing slot is zero, out does
    not depend on whether xs is written, and nothing is written behind xs."""
    shape = wr.SPLIT_SHAPES[name]
    N, C, H, W, S, fs = shape
    d = _inputs('split' + name, 'noise', shape)
    ref64, ref32, cmp = _fwd_refs('split' + name, 'noise', shape, 1, True)
    plain, _ = _fwd(dev, d['x'], d['stats'], 1, d['maps'], shape)
    both, xs_both = _fwd(dev, d['x'], d['stats'], 1, d['maps'], shape, want_xs=True)
    none, xs_only = _fwd(dev, d['x'], d['stats'], 1, d['maps'], shape, want_out=False, want_xs=True)
    _check_fwd('split-%s' % name, plain, ref64, ref32, cmp)
    assert none is None and torch.equal(both, plain), 'out depends on xs'
    assert torch.equal(xs_only, xs_both)
    val, closing = _decode_split(xs_both, N, 2 * C, H, W)
    val, closing = val.cpu(), closing.cpu()
    assert not bool(torch.isnan(val).any()) and not bool(torch.isnan(closing).any()), 'a slot of xs was never written'
    assert float(closing.abs().max()) == 0.0
    assert float(((val - plain).abs() - plain.abs() * 2.0 ** -16).max()) <= 1e-30


@pytest.mark.parametrize('name', list(wr.S2D_SHAPES))
def test_space_to_depth_split_on_non_square_maps(dev, name):
    """flags = 1 on even non-square maps: byte for byte ap_split_prepass_s2d of the fp32 result, padding ring and closing slots
    included (the window starts as NaN bytes), nothing behind it."""
    from animateportrait_amd import ops
    shape = wr.S2D_SHAPES[name]
    N, C, H, W, S, fs = shape
    d = _inputs('s2d' + name, 'noise', shape)
    plain, _ = _fwd(dev, d['x'], None, 0, d['maps'], shape)
    both, xs = _fwd(dev, d['x'], None, 0, d['maps'], shape, want_xs=True, flags=1)
    none, xs_only = _fwd(dev, d['x'], None, 0, d['maps'], shape, want_out=False, want_xs=True, flags=1)
    assert torch.equal(both, plain) and torch.equal(xs_only, xs)
    want = ops.presplit_s2d(ops.Feat(plain.to(dev)))
    assert tuple(want.shape) == (N, 8 * C, H // 2 + 1, W // 2 + 1) and want.xs.numel() == xs.numel()
    assert torch.equal(xs.cpu(), want.xs.view(torch.uint8).reshape(-1).cpu())


@pytest.mark.parametrize('act', [0, 2])
@pytest.mark.parametrize('name', list(wr.OCTET_SHAPES))
def test_octet_input_is_bitwise_the_nchw_launch(dev, name, act):
    """flags = 2: the same values in the channel-octet layout give the NCHW launch's output bit for bit -- untiled ragged blocks
    (40 x 40) and the tiled mapping with the lerp path (24 x 64)."""
    shape = wr.OCTET_SHAPES[name]
    d = _inputs('octet' + name, 'noise', shape)
    nchw, xs0 = _fwd(dev, d['x'], d['stats'], act, d['maps'], shape, want_xs=True)
    octet, xs1 = _fwd(dev, d['x'], d['stats'], act, d['maps'], shape, want_xs=True, flags=2)
    assert torch.equal(octet, nchw) and torch.equal(xs0, xs1)
    ref64, ref32, cmp = _fwd_refs('octet' + name, 'noise', shape, act, True)
    _check_fwd('octet-%s act=%d' % (name, act), octet, ref64, ref32, cmp)


@pytest.mark.parametrize('kind', ['noise', 'out'])
@pytest.mark.parametrize('name', list(wr.QUAD_SHAPES))
def test_quad_gather_at_narrow_maps(dev, monkeypatch, name, kind):
    """APAMD_WARP_GATHER=quad on a 4-pixel-wide map (the xb = clamp(x0, 0, W - 2) edge: every sample touches it) and on one tiled
    block, with noisy and with mostly out-of-frame maps: bit for bit the lane gather."""
    shape = wr.QUAD_SHAPES[name]
    d = _inputs('quad' + name, kind, shape)
    monkeypatch.delenv('APAMD_WARP_GATHER', raising=False)
    lane, _ = _fwd(dev, d['x'], d['stats'], 1, d['maps'], shape, flags=2)
    monkeypatch.setenv('APAMD_WARP_GATHER', 'quad')
    quad, _ = _fwd(dev, d['x'], d['stats'], 1, d['maps'], shape, flags=2)
    monkeypatch.delenv('APAMD_WARP_GATHER', raising=False)
    assert torch.equal(quad, lane), float((quad - lane).abs().max())
    ref64, ref32, cmp = _fwd_refs('quad' + name, kind, shape, 1, True)
    _check_fwd('quad-%s-%s' % (name, kind), quad, ref64, ref32, cmp)


# ------------------------------------------------------------------------------------------------------------ backward

@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name,kind', SHAPE_KIND, ids=['%s-%s' % nk for nk in SHAPE_KIND])
def test_backward_at_ragged_shapes(dev, monkeypatch, name, kind, mode):
    """The scatter at every shape of warp_reference.SHAPES (partial tiles, dead pixels of a tile, one-pixel axes, S = 1, S < H),
    by the tiled kernel and by the tap-by-tap comparison kernel: both meet the same bar against float64."""
    from animateportrait_amd import ops
    shape = wr.SHAPES[name]
    d = _inputs(name, kind, shape)
    gout, ref64, e_ref, A = _bwd_refs(name, kind, shape)
    _set_mode(monkeypatch, mode)
    if name in wr.LEVEL_OF:
        dx = ops.warp_concat_bwd(gout.to(dev), *(t.to(dev) for t in d['maps']), wr.LEVEL_OF[name]).cpu()
    else:
        dx = _bwd(dev, gout, d['maps'], shape)
    _check_bwd('%s-%s %s' % (name, kind, mode), dx, ref64, e_ref, A)


def _poison_flow_half(gout, C):
    gout[:, C:] = 1e30


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', list(wr.BWD_CASES))
def test_backward_on_hostile_maps(dev, monkeypatch, name, mode):
    """The named cases of warp_reference.BWD_CASES (tests/test_warp_reference_cpu.py proves that each reaches its branch): boxes
    that fit, windows clipped in both directions with an odd channel count, white noise, a centre window that catches nothing,
    tiles that scatter nothing, same-lane and full-wave collisions, exact border coordinates, a dead flow branch."""
    kind, shape = wr.BWD_CASES[name]
    N, C, H, W, S, fs = shape
    d = _inputs(name, kind, shape)
    gout, ref64, e_ref, A = _bwd_refs(name, kind, shape, _poison_flow_half if name == 'maskoff' else None)
    _set_mode(monkeypatch, mode)
    dx = _bwd(dev, gout, d['maps'], shape)
    _check_bwd('%s %s' % (name, mode), dx, ref64, e_ref, A)
    if name == 'nothing':
        assert float(A.max()) == 0.0 and bool((dx == 0.0).all()), 'nothing: dx must be exactly 0.0 everywhere'
    if name == 'maskoff':
        assert float(dx.abs().max()) < 1e3, 'maskoff: the gradient of the dead flow half leaked into dx'


@pytest.mark.parametrize('name', ['direct40', 'overhang', 'upsample'])
def test_forward_and_backward_are_adjoint(dev, name):
    """sum(fwd(x) * g) == sum(x * bwd(g)), both sides from the kernels (they evaluate the same fp32 weights), accumulated in float64
    on the host; g is zero where the flow half is the constant -1 or ambiguous.  Tolerance: 2^-20 of the sum of the absolute terms
    |x * weight * g|, as for the backward bar."""
    shape = wr.SHAPES[name]
    N, C, H, W, S, fs = shape
    d = _inputs(name, 'noise', shape)
    g = d['gout'].clone()
    g[:, C:] *= ((d['m64'] > 0.5) & ~d['amb']).float()
    y, _ = _fwd(dev, d['x'], None, 0, d['maps'], shape)
    dx = _bwd(dev, g, d['maps'], shape)
    lhs, rhs = float((y.double() * g.double()).sum()), float((d['x'].double() * dx.double()).sum())
    terms = float((d['x'].double().abs() * wr.abs_mass(g, *d['maps'], fs)).sum())
    print('adjoint %-10s <fwd x, g> = %.9e  <x, bwd g> = %.9e  |diff| = %.3e  bar = %.3e' % (name, lhs, rhs, abs(lhs - rhs), 2.0 ** -20 * terms))
    assert abs(lhs - rhs) <= 2.0 ** -20 * terms, (name, lhs, rhs, terms)


# ------------------------------------------------------------------------------------------------------------ refusals

def _refused(rc):
    from animateportrait_amd import _capi
    msg = _capi.lib().ap_last_error()
    return rc < 0 and bool(msg) and len(msg) > 0


def test_forward_refusals(dev):
    """Arguments outside the contract return a negative status with a message; nothing is launched (the dummy buffers are far
    smaller than the shapes named)."""
    from animateportrait_amd import ops, _capi
    lib = _capi.lib()
    buf = torch.full((4096,), SENT, dtype=torch.float32, device=dev)
    p, null = ops._ptr(buf), ops._ptr(None)

    def call(mean=null, rstd=null, act=0, out=p, xs=null, N=1, C=8, H=4, W=4, S=4, flags=0):
        return lib.ap_warp_concat_fwd_ex(p, mean, rstd, act, p, p, p, out, xs, N, C, H, W, S, 1.0, flags, ops._stream())
    assert _refused(call(xs=p, C=12)), 'xs with C % 8 != 0'
    assert _refused(call(xs=p, C=9, out=null))
    assert _refused(call(xs=p, H=5, flags=1)), 's2d with odd H'
    assert _refused(call(xs=p, W=3, flags=1)), 's2d with odd W'
    assert _refused(call(flags=2, C=12)), 'octet input with C = 12'
    assert _refused(call(mean=p)), 'mean without rstd'
    assert _refused(call(rstd=p)), 'rstd without mean'
    assert _refused(call(act=3)) and _refused(call(act=-1))
    assert _refused(call(N=0)) and _refused(call(N=65536))
    assert _refused(call(C=0)) and _refused(call(H=0)) and _refused(call(W=0)) and _refused(call(S=0))
    assert _refused(call(out=null)), 'neither out nor xs'
    assert _refused(call(H=46341, W=46341)) and _refused(call(H=32768, W=32768)), 'H * W > INT_MAX / 2'
    torch.cuda.synchronize()
    assert bool((buf == SENT).all()), 'a refused call wrote'


def test_backward_refusals(dev):
    """Sizes the tiled kernel's packed tap word (15 + 16 bits under a flag) or an int plane offset cannot hold are refused BEFORE dx
    is cleared, as are N = 0 / 65536 and null pointers."""
    from animateportrait_amd import ops, _capi
    lib = _capi.lib()
    buf = torch.full((4096,), SENT, dtype=torch.float32, device=dev)
    p, null = ops._ptr(buf), ops._ptr(None)

    def call(dx=p, N=1, C=1, H=4, W=4, S=4):
        return lib.ap_warp_concat_bwd(p, p, p, p, dx, N, C, H, W, S, 1.0, ops._stream())
    assert _refused(call(H=32758, W=1)), 'H > 32757'
    assert _refused(call(H=1, W=65526)), 'W > 65525'
    assert _refused(call(H=32757, W=32800)), 'H * W > INT_MAX / 2'
    assert _refused(call(N=0)) and _refused(call(N=65536)) and _refused(call(C=0)) and _refused(call(S=0))
    assert _refused(call(dx=null))
    torch.cuda.synchronize()
    assert bool((buf == SENT).all()), 'a refused call cleared or wrote dx'


def test_ops_backward_validates_like_the_forward(dev):
    from animateportrait_amd import ops
    n, c, s = 1, 3, 8
    mo, fl, mk = (torch.zeros(sh, device=dev) for sh in ((n, s, s, 2), (n, 2, s, s), (n, 1, s, s)))
    g = torch.zeros(n, 2 * c, s, s, device=dev)
    assert tuple(ops.warp_concat_bwd(g, mo, fl, mk, 0).shape) == (n, c, s, s)
    with pytest.raises(ValueError):
        ops.warp_concat_bwd(g[:, :5].contiguous(), mo, fl, mk, 0)              # an odd channel count is no concat
    with pytest.raises(ValueError):
        ops.warp_concat_bwd(g, mo, fl, mk, 1)                                  # level 1 of an 8 px model is 4 px
    with pytest.raises(ValueError):
        ops.warp_concat_bwd(g[:, :, :, :4].contiguous(), mo, fl, mk, 0)        # not square
    with pytest.raises(ValueError):
        ops.warp_concat_bwd(g, mo, fl[:, :1].contiguous(), mk, 0)
    with pytest.raises(ValueError):
        ops.warp_concat_bwd(g, mo[:, :4].contiguous(), fl, mk, 0)
    with pytest.raises(ValueError):
        ops.warp_concat_bwd(g, mo, fl, torch.zeros(2, 1, s, s, device=dev), 0)
    with pytest.raises(RuntimeError):
        ops.warp_concat_bwd(g.cpu(), mo, fl, mk, 0)
