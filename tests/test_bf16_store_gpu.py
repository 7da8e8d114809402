"""GPU (-m gpu): the stores of the plain-bf16 train step's ResNet trunk and the output windows they go through.

* A: the bf16 epilogue of the dense 3x3 stride-1 tiles (Bf3Cfg::OB16, tall and short) in each of its three store forms -- 16-byte
  words of 8 pixels, 8-byte words of 4, single elements -- against the fp64 sum of the bf16 operands, rounded to bf16: bit for
  bit on all but a few elements, and the InstanceNorm partial sums from the fp32 values before rounding.
* B: ap_conv2d_fwd_view / _view_bf16out into windows of a larger destination filled with a sentinel: the window holds the
  reference's sub-grid, every element outside it keeps the sentinel bit for bit.
* C: ops.conv2d_dgrad_strip (the padded-coordinate data gradient of a reflection-padded 3x3 layer in two launches) against the
  gradient with respect to the padded input, whole map, last two columns and corners, and against the single launch it replaces.
Every reference is fp64 on the CPU; r16(t) is the bf16 value of an operand or of a stored result."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from conftest import linf

pytestmark = pytest.mark.gpu

TALL, SHORT = 'Bf3Cfg<1, 3, 1, 2, 4, 4> bf16', 'Bf3Cfg<1, 3, 1, 2, 4, 1> bf16'
SENT32, SENT16 = 0x7FC0A5A5, 0x7FA5          # NaN bit patterns no kernel writes


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


def r16(t):
    """round to bf16 (nearest even), back in fp64"""
    return t.float().bfloat16().double()


def bf16_ulp(v):
    """spacing of the bf16 numbers at |v| (fp64 in, fp64 out)"""
    return torch.pow(2.0, torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126))) - 7)


def check_bf16_store(out, ref, what, min_equal=0.999):
    """out: a stored bf16 result, ref: the fp64 value it stands for.  At least `min_equal` of the elements equal bf16(ref) bit for
    bit, and none is more than one bf16 ulp away.  An element flips only where the fp32 accumulation and the fp64 one lie on
    either side of a rounding midpoint; where ref is within fp32 summation noise of zero (an activation's kink, a cancelling sum)
    the bound is that noise instead."""
    assert out.dtype == torch.bfloat16, what
    o, e = out.detach().cpu().double(), r16(ref)
    assert o.shape == e.shape, what
    floor = 1e-6 * float(ref.abs().max())
    d = (o - e).abs()
    eq = float((o == e).double().mean())
    worst = float((d / torch.maximum(bf16_ulp(e), torch.full_like(e, floor))).max())
    assert eq >= min_equal, (what, 'bit-equal fraction', eq)
    assert worst <= 1.0, (what, 'worst error in bf16 ulps', worst)
    return eq


def kernel_name(spec, n, h, w):
    from animateportrait_amd import _capi
    buf = ctypes.create_string_buffer(96)
    d = spec.desc(n, h, w)
    _capi.check(_capi.lib().ap_conv2d_kernel_name(ctypes.byref(d), buf, 96), 'kernel_name')
    return buf.value.decode(), d


def act_ref(v, act):
    from animateportrait_amd import ops
    if act == ops.ACT_RELU:
        return v.clamp_min(0)
    if act == ops.ACT_LRELU:
        return torch.where(v > 0, v, 0.2 * v)
    return v


# ---------------------------------------------------------------- A: bf16-output forward, the three store forms of both tile heights

FWD = [
    # name, N, segments, cout, H, W, reflect, virtual segment 0, bias, act, statistics, tall tiles
    # 16-byte form: W % 32 == 0, Cout % 64 == 0, H % TH == 0
    ('16B tall, ConvLayer.run', 1, (64,), 64, 16, 64, True, False, False, 'none', True, True),
    ('16B short', 3, (32, 32), 128, 8, 32, False, False, True, 'relu', False, False),
    ('16B tall, virtual source', 1, (64, 32), 64, 16, 32, True, True, True, 'none', True, True),
    # 8-byte form: even ragged W, H not a multiple of TH, a partial cout tile
    ('8B tall', 1, (64,), 80, 19, 66, True, False, True, 'lrelu', True, True),
    ('8B short', 3, (128,), 40, 6, 66, False, False, False, 'none', True, False),
    # element form: odd W
    ('scalar tall', 1, (48, 16, 32), 64, 17, 37, True, False, True, 'relu', True, True),
    ('scalar short', 1, (64,), 80, 5, 45, False, False, True, 'lrelu', False, False),
]


@pytest.mark.parametrize('case', FWD, ids=[c[0] for c in FWD])
def test_bf16_output_forward(dev, monkeypatch, case):
    """ops.conv2d(out_bf16=True) of a dense 3x3 stride-1 layer in plain-bf16 arithmetic: act(sum r16(x) r16(w) + b) stored as bf16
    (ConvLayer.run reaches the store only with norm_act, i.e. without bias and activation: the other cases call ops.conv2d)."""
    from animateportrait_amd import ops
    from animateportrait_amd.networks import ConvLayer
    name, n, segs, cout, H, W, reflect, virt, has_bias, act, stats, tall = case
    act = {'none': ops.ACT_NONE, 'relu': ops.ACT_RELU, 'lrelu': ops.ACT_LRELU}[act]
    monkeypatch.setattr(ops, 'DEFAULT_PRECISION', ops.PRECISION_BF16)
    if tall:
        monkeypatch.setenv('APAMD_NO_SMALL_TILES', '1')
    else:
        monkeypatch.delenv('APAMD_NO_SMALL_TILES', raising=False)
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    cin = sum(segs)
    w = torch.randn(cout, cin, 3, 3, generator=gen) / (3.0 * cin ** 0.5)
    b = torch.randn(cout, generator=gen) * 0.3 if has_bias else torch.zeros(cout)
    xs = [torch.randn(n, c, H, W, generator=gen) * 1.3 + 0.2 for c in segs]
    layer = ConvLayer(list(segs), cout, 3, 1, 1, ops.PAD_REFLECT if reflect else ops.PAD_ZERO).to(dev)
    layer.spec.precision = ops.PRECISION_BF16
    with torch.no_grad():
        layer.weight.copy_(w); layer.bias.copy_(b)
    kname, d = kernel_name(layer.spec, n, H, W)
    assert kname == (TALL if tall else SHORT), kname
    assert ops.C.lib().ap_conv2d_bf16out_ok(ctypes.byref(d)) == 1
    srcs, ops_in = [], []
    for i, x in enumerate(xs):
        if virt and i == 0:
            # a virtual source: relu(IN(x)) applied by the split pass on the device, from these fp32 statistics
            xd = x.to(dev)
            mean = xd.mean((2, 3)).reshape(-1).contiguous()
            rstd = (xd.var((2, 3), unbiased=False) + 1e-5).rsqrt().reshape(-1).contiguous()
            srcs.append(ops.Feat(xd, mean, rstd, ops.ACT_RELU))
            m64, r64 = mean.cpu().double().view(n, -1, 1, 1), rstd.cpu().double().view(n, -1, 1, 1)
            ops_in.append(((x.double() - m64) * r64).clamp_min(0))
        else:
            srcs.append(ops.Feat(x.to(dev)))
            ops_in.append(x.double())
    if name.endswith('ConvLayer.run'):
        assert not has_bias and act == ops.ACT_NONE and stats
        out = layer.run(srcs, norm_act=ops.ACT_RELU, out_bf16=True)
    else:
        out = ops.conv2d(layer.spec, srcs, layer.packed(), layer.bias.detach() if has_bias else None, act=act,
                         want_stats=stats, out_bf16=True)
    assert out.data.dtype == torch.bfloat16 and tuple(out.data.shape) == (n, cout, H, W)
    xp = torch.cat([F.pad(r16(v), (1,) * 4, mode='reflect' if reflect else 'constant') for v in ops_in], 1)
    pre = F.conv2d(xp, r16(w)) + b.double().view(1, -1, 1, 1)           # the fp32 accumulators' exact value
    ref = act_ref(pre, act)
    if virt:
        # the split pass evaluates relu(IN(.)) in fp32: an operand that lies within fp32 noise of a bf16 midpoint rounds to the
        # neighbouring bf16 and moves the 9 x cout outputs it feeds by |w| ulp -- the quantile bar of
        # test_resnet_block_with_bf16_stored_activations instead of the bit-for-bit one
        err = (out.data.cpu().double() - r16(ref)).abs()
        scale = float(ref.abs().max())
        assert float((err == 0).double().mean()) >= 0.99, name
        assert float(err.quantile(0.999)) < 1e-3 * scale, (name, float(err.quantile(0.999)) / scale)
        assert float(err.max()) < 3e-2 * scale, (name, float(err.max()) / scale)
    else:
        check_bf16_store(out.data, ref, name)
    if stats:
        partial, tiles = out.pending
        p = partial.cpu().double().view(n, cout, tiles, 2).sum(2)
        cnt = H * W
        mean_k = p[..., 0] / cnt
        var_k = p[..., 1] / cnt - mean_k ** 2
        mean_r, var_r = pre.mean((2, 3)), pre.var((2, 3), unbiased=False)
        sd = var_r.sqrt()
        e_mean = float(((mean_k - mean_r).abs() / sd).max())
        e_rstd = float(((var_r / var_k).sqrt() - 1).abs().max())
        # fp32 sums of <= 512 values per tile: ~1e-7 of the plane's spread.  Statistics of the ROUNDED stored values differ from
        # these by the mean of the rounding errors, ~ 2^-9 sd / sqrt(H W): 2e-5 sd and more at these plane sizes (<= 4096 pixels),
        # ten times the bar -- sums taken after the rounding fail it (checked below on this very output)
        assert e_mean < 2e-6 and e_rstd < 2e-6, (name, e_mean, e_rstd)
        o = out.data.cpu().double()
        if act == ops.ACT_NONE:
            gap_mean = float(((o.mean((2, 3)) - mean_r).abs() / sd).max())
            gap_rstd = float(((var_r / o.var((2, 3), unbiased=False)).sqrt() - 1).abs().max())
            assert gap_mean > 1e-5 or gap_rstd > 1e-5, (name, gap_mean, gap_rstd)


# ---------------------------------------------------------------- B: output windows

ARITH = [('bf16x3', torch.float32), ('bf16', torch.float32), ('bf16', torch.bfloat16)]


def _windows():
    # name, N, C, cout, input H, W, pad, window(Hout, Wout, cout) -> (base, nstride, cstride, rstride, xstride, y_off, x_off, OH, OW)
    return [
        # the strip's main window: columns 0 .. Wout - 3 of a padded data gradient
        ('strip main', 2, 32, 64, 6, 32, 2,
         lambda ho, wo, co: (0, co * ho * wo, ho * wo, wo, 1, 0, 0, ho, wo - 2)),
        # the strip's transposed window: output rows become destination columns 30..33 of 34-element rows
        ('strip transposed', 3, 64, 80, 2, 20, 2,
         lambda ho, wo, co: (0, co * wo * 34, wo * 34, 1, 34, 30, 0, ho, wo)),
        # a general window: offsets, every other column, odd row stride, fewer rows, padded channel and image strides, y not aligned
        ('general', 2, 48, 80, 12, 40, 1,
         lambda ho, wo, co: (1, 918 * co + 7, 918, 83, 2, 2, 3, ho - 3, wo - 3)),
        # row stride a multiple of 4 (and of 8), odd channel stride: no 16- or 8-byte store may be used
        ('rstride % 8 == 0, odd cstride', 1, 64, 64, 8, 64, 1,
         lambda ho, wo, co: (0, 545 * co + 4, 545, 68, 1, 0, 0, ho, wo)),
        # every stride a multiple of 8, y one / two elements past a 16-byte boundary
        ('y + 1 element', 2, 32, 64, 8, 64, 1,
         lambda ho, wo, co: (1, 576 * co, 576, 72, 1, 0, 0, ho, wo)),
        ('y + 2 elements', 2, 32, 64, 8, 64, 1,
         lambda ho, wo, co: (2, 576 * co, 576, 72, 1, 0, 0, ho, wo)),
    ]


WINDOWS = _windows()


@pytest.mark.parametrize('arith', ARITH, ids=['%s into %s' % (a, str(t)[6:]) for a, t in ARITH])
@pytest.mark.parametrize('win', WINDOWS, ids=[w[0] for w in WINDOWS])
def test_output_window(dev, monkeypatch, arith, win):
    """ops._conv2d_view of a 3x3 layer into a window of a sentinel-filled buffer: the reference's sub-grid inside, the sentinel
    everywhere else (the 256 elements behind the window's last one included).  The last three windows have strides or a y
    that rule out the 16- and 8-byte store forms: ap_out_view takes any strides."""
    from animateportrait_amd import ops
    prec_name, dtype = arith
    name, n, c, cout, H, W, pad, mk = win
    prec = ops.PRECISION_BY_NAME[prec_name]
    monkeypatch.setattr(ops, 'DEFAULT_PRECISION', prec)
    gen = torch.Generator().manual_seed(sum(map(ord, name)) + prec)
    x = torch.randn(n, c, H, W, generator=gen)
    w = torch.randn(cout, c, 3, 3, generator=gen) / (3.0 * c ** 0.5)
    spec = ops.ConvSpec([c], cout, 3, 1, pad, ops.PAD_ZERO)
    spec.precision = prec
    ho, wo = spec.out_size(H, W)
    base, ns, cs, rs, xs, y_off, x_off, oh, ow = mk(ho, wo, cout)
    assert 1 <= oh <= ho and 1 <= ow <= wo
    v = ops.C.ApOutView()
    v.nstride, v.cstride, v.rstride, v.xstride, v.y_off, v.x_off, v.OH, v.OW = ns, cs, rs, xs, y_off, x_off, oh, ow
    idx = (base + torch.arange(n).view(-1, 1, 1, 1) * ns + torch.arange(cout).view(1, -1, 1, 1) * cs +
           (torch.arange(oh).view(1, 1, -1, 1) + y_off) * rs + (torch.arange(ow).view(1, 1, 1, -1) + x_off) * xs)
    assert int(idx.min()) >= 0 and idx.flatten().unique().numel() == idx.numel()
    total = int(idx.max()) + 1 + 256                               # a sentinel tail behind the last element of the window
    ibits = torch.int32 if dtype == torch.float32 else torch.int16
    sent = SENT32 if dtype == torch.float32 else SENT16
    buf = torch.full((total,), sent, dtype=ibits, device=dev).view(dtype)
    packed = ops.pack_weights(spec, w.to(dev))
    ops._conv2d_view(spec, [ops.Feat(x.to(dev))], packed, buf[base:], v)
    torch.cuda.synchronize()
    got = buf.cpu()
    bits = got.view(ibits)
    inside = torch.zeros(total, dtype=torch.bool)
    inside[idx.flatten()] = True
    assert bool((bits[~inside] == sent).all()), (name, 'written outside the window', int((bits[~inside] != sent).sum()))
    vals = got[idx]
    bf16 = prec == ops.PRECISION_BF16
    ref = F.conv2d(F.pad(r16(x) if bf16 else x.double(), (pad,) * 4), r16(w) if bf16 else w.double())[:, :, :oh, :ow]
    if dtype == torch.bfloat16:
        check_bf16_store(vals, ref, name)
    else:
        sc = float(ref.abs().max())
        # plain bf16: fp32 sums of exact products; split bf16: ~2^-16 per operand
        assert linf(vals, ref) <= (3e-5 if bf16 else 1e-4) * sc, (name, linf(vals, ref) / sc)


def test_output_window_dense_equals_plain_forward(dev, monkeypatch):
    """the whole output as a window with the dense strides is ap_conv2d_fwd bit for bit (same tiles, same stores)"""
    from animateportrait_amd import ops
    monkeypatch.setattr(ops, 'DEFAULT_PRECISION', ops.PRECISION_BF16X3)
    gen = torch.Generator().manual_seed(5)
    n, c, cout, H, W = 2, 64, 80, 9, 40
    x = torch.randn(n, c, H, W, generator=gen).to(dev)
    spec = ops.ConvSpec([c], cout, 3, 1, 1, ops.PAD_ZERO)
    spec.precision = ops.PRECISION_BF16X3
    packed = ops.pack_weights(spec, (torch.randn(cout, c, 3, 3, generator=gen) * 0.05).to(dev))
    f = ops.Feat(x)
    plain = ops.conv2d(spec, [f], packed).data
    out = torch.full_like(plain, float('nan'))
    v = ops.C.ApOutView()
    v.nstride, v.cstride, v.rstride, v.xstride, v.y_off, v.x_off, v.OH, v.OW = cout * H * W, H * W, W, 1, 0, 0, H, W
    ops._conv2d_view(spec, [f], packed, out, v)
    assert torch.equal(out, plain)


# ---------------------------------------------------------------- C: the strip data gradient

STRIP = [
    # N, layer input segments, layer outputs (= gradient channels), H, W
    (1, (64,), 32, 4, 32),          # the smallest gradient width the split path takes, the smallest H
    (3, (72,), 64, 5, 64),          # odd H, a partial cout tile in the gradient operator (72 outputs)
    (1, (64,), 256, 4, 96),
    (1, (48, 16), 128, 7, 128),     # two segments: the weight operand is a strided channel slice; 16 outputs from 128 inputs
    (2, (64,), 64, 4, 256),
    (1, (64,), 64, 64, 64),         # the trunk's map
]
STRIP_ARITH = [('bf16x3', False), ('bf16', False), ('bf16', True)]


def padded_grad_ref(dy, w):
    """gradient of sum(conv2d(xp, w) * dy) with respect to the padded input xp (N, Cin, H+2, W+2), fp64"""
    n, _, h, wd = dy.shape
    xp = torch.zeros(n, w.shape[1], h + 2, wd + 2, dtype=torch.float64, requires_grad=True)
    return torch.autograd.grad((F.conv2d(xp, w) * dy).sum(), xp)[0]


def check_padded_grad(out, ref, bf16_arith, what):
    """whole padded map, then its last two columns and its four corners on their own (where a strip bug would hide)"""
    W = ref.shape[3] - 2
    regions = [('map', lambda t: t), ('last two columns', lambda t: t[..., W:]),
               ('corners', lambda t: t[..., [0, 0, -1, -1], [0, -1, 0, -1]])]
    if out.dtype == torch.bfloat16:
        for rname, sel in regions:
            check_bf16_store(sel(out.cpu()), sel(ref), (what, rname), 0.999 if rname == 'map' else 0.0)
        return
    sc = float(ref.abs().max())
    errs = {rname: linf(sel(out), sel(ref)) / sc for rname, sel in regions}
    assert max(errs.values()) <= (3e-5 if bf16_arith else 1e-4), (what, errs)


@pytest.mark.parametrize('from_inbwd', [False, True], ids=['host strip', 'instnorm_bwd_split strip'])
@pytest.mark.parametrize('arith', STRIP_ARITH, ids=['%s%s' % (a, ' bf16 out' if o else '') for a, o in STRIP_ARITH])
@pytest.mark.parametrize('case', STRIP, ids=['N%d %s->%d %dx%d' % (c[0], '+'.join(map(str, c[1])), c[2], c[3], c[4]) for c in STRIP])
def test_dgrad_strip(dev, monkeypatch, case, arith, from_inbwd):
    from animateportrait_amd import ops, autograd
    from animateportrait_amd.networks import ConvLayer
    n, segs, cout, H, W = case
    prec_name, out_bf16 = arith
    prec = ops.PRECISION_BY_NAME[prec_name]
    bf16 = prec == ops.PRECISION_BF16
    monkeypatch.setattr(ops, 'DEFAULT_PRECISION', prec)
    gen = torch.Generator().manual_seed(n * 7 + cout + H + W + prec)
    cin = sum(segs)
    wt = torch.randn(cout, cin, 3, 3, generator=gen) / (3.0 * cout ** 0.5)
    layer = ConvLayer(list(segs), cout, 3, 1, 1, ops.PAD_REFLECT).to(dev)
    layer.spec.precision = prec
    with torch.no_grad():
        layer.weight.copy_(wt)
    if from_inbwd:
        # the gradient as the InstanceNorm backward of the layer's output writes it: split copy + transposed column strip
        raw = torch.randn(n, cout, H, W, generator=gen).to(dev)
        mean = raw.mean((2, 3)).reshape(-1).contiguous()
        rstd = (raw.var((2, 3), unbiased=False) + 1e-5).rsqrt().reshape(-1).contiguous()
        f = ops.Feat(raw, mean, rstd, ops.ACT_RELU)
        assert ops.instnorm_bwd_split_ok(f, 0)
        g1 = torch.randn(n, cout, H, W, generator=gen).to(dev)
        g, _, strip = ops.instnorm_bwd_split((g1, 0, None), f, None, want_xs=True, want_strip=True, want_dy=True)
        assert strip is not None and tuple(strip.data.shape) == (n, cout, 2, H)
    else:
        g, strip = ops.Feat(torch.randn(n, cout, H, W, generator=gen).to(dev)), None
    dy = g.data.cpu().double()
    c0 = 0
    for i, c in enumerate(segs):
        what = (case, arith, from_inbwd, 'segment %d' % i)
        spec, fold = autograd._dgrad_spec(layer, c)
        assert fold == 1
        w = layer.weight.detach()
        if len(segs) > 1:
            w = w[:, c0:c0 + c]
        packed = layer.packed_dgrad(i, spec, w)
        packed_t = layer.packed_dgrad((i, 'T'), spec, w.transpose(2, 3))
        assert ops.dgrad_strip_eligible(spec, g), what
        out = ops.conv2d_dgrad_strip(spec, g, packed, packed_t, strip, out_bf16=out_bf16)
        assert out.dtype == (torch.bfloat16 if out_bf16 else torch.float32), what
        assert tuple(out.shape) == (n, c, H + 2, W + 2), what
        ws = w.cpu().double()
        ref = padded_grad_ref(r16(dy) if bf16 else dy, r16(ws) if bf16 else ws)
        check_padded_grad(out, ref, bf16, what)
        # the single three-tile-column launch the strip replaces
        single = ops.conv2d(spec, [g], packed, None).data.cpu().double()
        sc = float(single.abs().max())
        if out_bf16:
            o = out.cpu().double()
            bound = torch.maximum(bf16_ulp(r16(single)), torch.full_like(single, 1e-6 * sc))
            assert bool(((o - single).abs() <= bound).all()), what
        else:
            assert linf(out, single) <= 1e-6 * sc, (what, linf(out, single) / sc)
        c0 += c


def test_trunk_layer_backward_stores_a_bf16_padded_gradient(dev, monkeypatch):
    """One trunk-like layer in plain-bf16 training, at a width other than the trunk's 64: its input is a bf16-stored raw output
    (virtual, IN + ReLU), its own raw output is stored as bf16 (conv_forward raw16), and the backward takes the strip route with
    the strip written by ap_instnorm_bwd_split.  The padded gradient on the tape is bf16 and equals the definition fed with the bf16
    dy that ap_instnorm_bwd_split wrote (the head planes of the gradient's split copy)."""
    from animateportrait_amd import ops, autograd
    from animateportrait_amd.networks import ConvLayer
    monkeypatch.setattr(ops, 'DEFAULT_PRECISION', ops.PRECISION_BF16)
    monkeypatch.setattr(ops, 'BF16_RAW', True)
    n, c, H, W = 3, 64, 32, 32
    gen = torch.Generator().manual_seed(2024)
    raw_in = (torch.randn(n, c, H, W, generator=gen) * 1.5 + 0.3).to(dev).bfloat16()
    rf = raw_in.float()
    mean = rf.mean((2, 3)).reshape(-1).contiguous()
    rstd = (rf.var((2, 3), unbiased=False) + 1e-5).rsqrt().reshape(-1).contiguous()
    gy = torch.randn(n, c, H, W, generator=gen)
    layer = ConvLayer([c], c, 3, 1, 1, ops.PAD_REFLECT).to(dev)
    layer.spec.precision = ops.PRECISION_BF16
    with torch.no_grad():
        layer.weight.copy_(torch.randn(c, c, 3, 3, generator=gen) / (3.0 * c ** 0.5)); layer.bias.zero_()
    seen = {}
    orig = ops.instnorm_bwd_split

    def spy(*a, **k):
        r = orig(*a, **k)
        seen['g'], seen['strip'] = r[0], r[2]
        return r
    monkeypatch.setattr(ops, 'instnorm_bwd_split', spy)
    tape = autograd.Tape()
    fx = tape.track(ops.Feat(raw_in, mean, rstd, ops.ACT_RELU))
    out = autograd.conv_forward(tape, layer, [fx], norm_act=ops.ACT_RELU, raw16=True)
    assert out.data.dtype == torch.bfloat16
    ops.presplit(out)            # its consumer's split pass, which finalises the statistics of a bf16 raw output
    tape.add(out, gy.to(dev), 0)
    tape.backward()
    assert 'g' in seen and seen['strip'] is not None, 'the backward did not take the strip route'
    contribs = tape.take(fx)
    assert len(contribs) == 1 and contribs[0][1] == 1
    gp = contribs[0][0]
    assert gp.dtype == torch.bfloat16 and tuple(gp.shape) == (n, c, H + 2, W + 2)
    # dy as the data gradient read it: XS[n][head|tail][C/8][H*W + 1][8 x bf16], head planes
    xs = seen['g'].xs.view(torch.bfloat16).view(n, 2, c // 8, H * W + 1, 8)[:, 0, :, :H * W]
    dy16 = xs.permute(0, 1, 3, 2).reshape(n, c, H, W).cpu().double()
    strip = seen['strip'].data.cpu()
    assert torch.equal(r16(strip), dy16[..., W - 2:].transpose(2, 3)), 'the column strip is not the split copy\'s last columns'
    ref = padded_grad_ref(dy16, r16(layer.weight.detach().cpu().double()))
    check_padded_grad(gp, ref, True, 'tape')
