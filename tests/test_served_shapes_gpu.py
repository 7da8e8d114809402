"""GPU (-m gpu): the plain-bf16 edge-layer kernels at the corners of the regions their C-ABI predicates accept
(tests/test_served_shapes_cpu.py lists those regions).  Every case asserts the route that ran (ops.LaunchProfiler) and compares with
an fp64 evaluation of the same operation on the bf16-rounded operands -- error below 3e-5 of the reference's scale, and more than
ten times that against the exact fp64 result, so a relabelled fp32 route fails too.  The kernels that take a workspace are also
called through the C ABI with a page of NaN behind the workspace, which must come back untouched."""
import contextlib
import ctypes

import pytest
import torch
import torch.nn.functional as F

from conftest import linf

pytestmark = pytest.mark.gpu

PAGE_FLOATS = 4096 // 4


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


def r16(t):
    """round to bf16 (nearest even), back in fp64"""
    return t.float().bfloat16().double()


@contextlib.contextmanager
def profiled():
    from animateportrait_amd import ops
    prof = ops.LaunchProfiler()
    ops.PROFILER = prof
    try:
        yield prof
    finally:
        ops.PROFILER = None


def check_bf16(out, ref16, exact, what):
    sc = float(ref16.abs().max())
    assert sc > 0, what
    e16, eex = linf(out, ref16) / sc, linf(out, exact) / sc
    assert e16 < 3e-5, (what, e16, eex)
    assert eex > 10 * e16, (what, e16, eex)


def nan_workspace(nfloats, dev):
    """a workspace of the reported size with one page of NaN behind it"""
    assert nfloats > 0
    return torch.full((nfloats + PAGE_FLOATS,), float('nan'), dtype=torch.float32, device=dev)


def assert_tail_untouched(ws, nfloats, what):
    torch.cuda.synchronize()
    tail = ws[nfloats:].cpu()
    ref = torch.full_like(tail, float('nan'))
    assert torch.equal(tail.view(torch.int32), ref.view(torch.int32)), what + ': wrote past its workspace'


# ---------------------------------------------------------------- the PatchGAN output layer's data gradient (dgrad_head_kernel)

HEAD = [
    # n, c, H, W, served by the kernel
    (1, 32, 2, 350, True),      # (H + 3) (W + 8) = 1790
    (2, 64, 4, 248, True),      # 1792: the staging exactly full
    (1, 96, 6, 191, True),      # 1791
    (2, 512, 34, 34, True),     # H W = 1156: the output planes' LDS bound
    (1, 32, 2, 2, True),
    (1, 64, 6, 192, False),     # H W within the plane bound, staging (1800) not: the general data gradient
    (1, 32, 4, 289, False),
]


@pytest.mark.parametrize('case', HEAD, ids=lambda c: 'N%d C%d %dx%d' % c[:4])
def test_head_dgrad_at_the_staging_limit(dev, monkeypatch, case):
    """Conv2d(C, 1, 4, 1, 1) (networks.py:2643) in plain-bf16 arithmetic, backward through autograd's layer backward: the data
    gradient runs on dgrad_head_kernel where ap_conv_head_dgrad_bf16_ok accepts the map -- the fp32-accumulated sums of
    bf16(w) x bf16(g) -- and on the general data gradient elsewhere.  (6 x 192 and 4 x 289 were accepted before (H + 3) (W + 8)
    <= 1792 was required: the kernel left the tail of its staged gradient rows unwritten and the last output row was wrong.)"""
    from animateportrait_amd import ops, autograd
    from animateportrait_amd.networks import ConvLayer
    n, c, H, W, served = case
    monkeypatch.setattr(ops, 'DEFAULT_PRECISION', ops.PRECISION_BF16)
    gen = torch.Generator().manual_seed(41 + n + c + H + W)
    w = torch.randn(1, c, 4, 4, generator=gen) * 0.05
    x = torch.randn(n, c, H, W, generator=gen)
    gy = torch.randn(n, 1, H - 1, W - 1, generator=gen)
    layer = ConvLayer([c], 1, 4, 1, 1).to(dev)
    layer.spec.precision = ops.PRECISION_BF16
    with torch.no_grad():
        layer.weight.copy_(w); layer.bias.zero_()

    def backward():
        tape = autograd.Tape()
        fx = tape.track(ops.Feat(x.to(dev)))
        out = autograd.conv_forward(tape, layer, [fx])
        assert tuple(out.data.shape) == (n, 1, H - 1, W - 1)
        tape.add(out, gy.to(dev), 0)
        with profiled() as prof:
            tape.backward()
        contribs = tape.take(fx)
        assert len(contribs) == 1 and contribs[0][1] == 0
        return contribs[0][0], prof
    gx, prof = backward()
    if served:
        assert prof.calls.get('dgrad_head') == 1 and not prof.records, (prof.calls, [r[0] for r in prof.records])
    else:
        assert 'dgrad_head' not in prof.calls and len(prof.records) == 1, (prof.calls, [r[0] for r in prof.records])
    assert tuple(gx.shape) == (n, c, H, W)

    def ref(wv, gv):
        xv = torch.zeros(n, c, H, W, dtype=torch.float64, requires_grad=True)
        (F.conv2d(xv, wv, padding=1) * gv).sum().backward()
        return xv.grad
    exact = ref(w.double(), gy.double())
    if served:
        check_bf16(gx, ref(r16(w), r16(gy)), exact, case)
    else:
        # the general data gradient of a one-channel gradient map keeps more than bf16 precision (measured: 1e-7 of the scale)
        assert linf(gx, exact) / float(exact.abs().max()) < 1e-5, case
    gx2, _ = backward()
    assert torch.equal(gx, gx2)


# ---------------------------------------------------------------- the PatchGAN first layer's weight gradient (form 2 of wgrad_k7.h)

WGRAD_D0 = [
    # n, cin, H, W
    (1, 2, 2, 480),             # two channels at the load budget (met exactly)
    (3, 2, 10, 480),
    (1, 1, 2, 512),             # one channel at the widest map
    (2, 1, 8, 512),
    (255, 2, 2, 32),            # one output row; images around the CU count
    (256, 1, 4, 32),
    (257, 2, 2, 64),
]


@pytest.mark.parametrize('case', WGRAD_D0, ids=lambda c: 'N%d Cin%d %dx%d' % c)
def test_wgrad_d0_at_the_load_budget(dev, case):
    """ap_wgrad_d0_bf16: dw of Conv2d(1 | 2, 64, 4, stride 2, pad 1) (networks.py:2620-2623) = fp32-accumulated sums of
    bf16(g) x bf16(x), deterministic."""
    from animateportrait_amd import ops
    n, cin, H, W = case
    gen = torch.Generator().manual_seed(53 + sum(case))
    x = torch.randn(n, cin, H, W, generator=gen)
    gy = torch.randn(n, 64, H // 2, W // 2, generator=gen)
    with profiled() as prof:
        dw = ops.wgrad(4, 2, 1, ops.PAD_ZERO, ops.Feat(gy.to(dev)), [ops.Feat(x.to(dev))], (64, cin, 4, 4), precision=ops.PRECISION_BF16)
    assert prof.calls.get('wgrad_k7<d0>') == 1, prof.calls

    def ref(xv, gv):
        wv = torch.zeros(64, cin, 4, 4, dtype=torch.float64, requires_grad=True)
        (F.conv2d(xv, wv, stride=2, padding=1) * gv).sum().backward()
        return wv.grad
    check_bf16(dw, ref(r16(x), r16(gy)), ref(x.double(), gy.double()), case)
    dw2 = ops.wgrad(4, 2, 1, ops.PAD_ZERO, ops.Feat(gy.to(dev)), [ops.Feat(x.to(dev))], (64, cin, 4, 4), precision=ops.PRECISION_BF16)
    assert torch.equal(dw, dw2)


@pytest.mark.parametrize('case', [(1, 2, 2, 480), (257, 1, 4, 32)], ids=lambda c: 'N%d Cin%d %dx%d' % c)
def test_wgrad_d0_c_abi_stays_in_its_workspace(dev, case):
    from animateportrait_amd import ops, _capi
    lib = _capi.lib()
    n, cin, H, W = case
    gen = torch.Generator().manual_seed(59 + sum(case))
    x = torch.randn(n, cin, H, W, generator=gen).to(dev)
    gy = torch.randn(n, 64, H // 2, W // 2, generator=gen).to(dev)
    nws = lib.ap_wgrad_d0_bf16_workspace_floats(n, 64, cin, H, W)
    ws = nan_workspace(nws, dev)
    dw = torch.empty(64, cin, 4, 4, dtype=torch.float32, device=dev)
    _capi.check(lib.ap_wgrad_d0_bf16(ops._ptr(gy), ops._ptr(x), n, 64, cin, H, W, ops._ptr(ws), ops._ptr(dw), ops._stream()), 'wgrad_d0_bf16')
    assert_tail_untouched(ws, nws, 'wgrad_d0_bf16')
    # a workspace full of NaN on entry: nothing of it is read before it is written -- the same bits as the ops route
    ref = ops.wgrad(4, 2, 1, ops.PAD_ZERO, ops.Feat(gy), [ops.Feat(x)], (64, cin, 4, 4), precision=ops.PRECISION_BF16)
    assert torch.equal(dw, ref)


# ---------------------------------------------------------------- the 7x7 edge layers' weight gradients (wgrad_k7.h)

K7 = [
    # name, final form, wide channels, narrow channels, N, H, W
    ('stem 1->32 16 columns, bpi capped at R/2', 0, 32, 1, 1, 4, 16),
    ('stem 3->64 256 columns, bpi capped at R/2', 0, 64, 3, 1, 4, 256),
    ('stem 3->32 16 columns, 257 images', 0, 32, 3, 257, 4, 16),
    ('stem 1->32 256 columns, 257 images', 0, 32, 1, 257, 4, 256),
    ('final 32->1 16 columns, bpi capped at R/2', 1, 32, 1, 1, 4, 16),
    ('final 64->1 256 columns, bpi capped at R/2', 1, 64, 1, 1, 4, 256),
    ('final 64->1 16 columns, 257 images', 1, 64, 1, 257, 4, 16),
    ('final 32->1 256 columns, 257 images', 1, 32, 1, 257, 4, 256),
]


def _k7_operands(case, dev):
    from animateportrait_amd import ops
    name, final_form, mw, cn, n, H, W = case
    gen = torch.Generator().manual_seed(61 + sum(map(ord, name)))
    if final_form:
        x = torch.randn(n, mw, H, W, generator=gen) * 1.3 + 0.2
        mean = torch.randn(n * mw, generator=gen) * 0.1
        rstd = torch.rand(n * mw, generator=gen) + 0.5
        gy = torch.randn(n, 1, H, W, generator=gen)
        src = ops.Feat(x.to(dev), mean.to(dev), rstd.to(dev), ops.ACT_RELU)
        xin = F.relu((x.double() - mean.double().view(n, mw, 1, 1)) * rstd.double().view(n, mw, 1, 1))
        xin32 = F.relu((x - mean.view(n, mw, 1, 1)) * rstd.view(n, mw, 1, 1))      # as the kernel forms it, in fp32
        out_shape = (1, mw, 7, 7)
    else:
        x = torch.randn(n, cn, H, W, generator=gen)
        gy = torch.randn(n, mw, H, W, generator=gen)
        src = ops.Feat(x.to(dev))
        xin, xin32 = x.double(), x
        out_shape = (mw, cn, 7, 7)
    return src, ops.Feat(gy.to(dev)), gy, xin, xin32, out_shape


@pytest.mark.parametrize('case', K7, ids=[c[0] for c in K7])
def test_wgrad_k7_at_the_served_corners(dev, case):
    """ap_wgrad_k7_bf16: the stems' and the last layer's 7x7 reflection-padded weight gradients at 4 rows (the fewest served), the
    narrowest and the widest rows, one workgroup per image and the block count capped at R / 2 rows."""
    from animateportrait_amd import ops
    name, final_form = case[:2]
    src, g, gy, xin, xin32, out_shape = _k7_operands(case, dev)
    with profiled() as prof:
        dw = ops.wgrad(7, 1, 3, ops.PAD_REFLECT, g, [src], out_shape, precision=ops.PRECISION_BF16)
    assert prof.calls.get('wgrad_k7<%s>' % ('final' if final_form else 'stem')) == 1, prof.calls

    def ref(xv, gv):
        wv = torch.zeros(out_shape, dtype=torch.float64, requires_grad=True)
        (F.conv2d(F.pad(xv, (3,) * 4, mode='reflect'), wv) * gv).sum().backward()
        return wv.grad
    check_bf16(dw, ref(r16(xin32), r16(gy)), ref(xin, gy.double()), name)
    dw2 = ops.wgrad(7, 1, 3, ops.PAD_REFLECT, g, [src], out_shape, precision=ops.PRECISION_BF16)
    assert torch.equal(dw, dw2)


@pytest.mark.parametrize('case', [K7[1], K7[7]], ids=[K7[1][0], K7[7][0]])
def test_wgrad_k7_c_abi_stays_in_its_workspace(dev, case):
    from animateportrait_amd import ops, _capi
    lib = _capi.lib()
    name, final_form, mw, cn, n, H, W = case
    src, g, _, _, _, out_shape = _k7_operands(case, dev)
    wide, narrow = (src, g) if final_form else (g, src)
    sw, sn = _capi.ApSrc(), _capi.ApSrc()
    sw.data, sw.C, sw.act = wide.data.data_ptr(), mw, wide.act
    if wide.virtual:
        sw.mean, sw.rstd = wide.mean.data_ptr(), wide.rstd.data_ptr()
    sn.data, sn.C, sn.act = narrow.data.data_ptr(), narrow.data.shape[1], ops.ACT_NONE
    nws = lib.ap_wgrad_k7_bf16_workspace_floats(n, mw, sn.C, H, W, final_form)
    ws = nan_workspace(nws, dev)
    dw = torch.empty(out_shape, dtype=torch.float32, device=dev)
    _capi.check(lib.ap_wgrad_k7_bf16(ctypes.byref(sw), ctypes.byref(sn), n, H, W, final_form, ops._ptr(ws), ops._ptr(dw), ops._stream()),
                'wgrad_k7_bf16')
    assert_tail_untouched(ws, nws, 'wgrad_k7_bf16')
    ref = ops.wgrad(7, 1, 3, ops.PAD_REFLECT, g, [src], out_shape, precision=ops.PRECISION_BF16)
    assert torch.equal(dw, ref)


# ---------------------------------------------------------------- the PatchGAN's first layer, forward (conv_d0.h)

CONV_D0 = [
    # n, cin, H, W, act
    (1, 1, 2, 8, 0),            # one output row of 4
    (2, 2, 2, 8, 1),
    (1, 2, 10, 8, 2),
    (2, 1, 6, 252, 2),          # W / 4 odd
    (1, 2, 2, 252, 0),
    (1, 2, 4, 256, 1),
    (3, 1, 2, 256, 2),
    (2, 1, 8, 256, 0),
]


@pytest.mark.parametrize('case', CONV_D0, ids=lambda c: 'N%d Cin%d %dx%d act%d' % c)
def test_conv_d0_at_the_served_corners(dev, monkeypatch, case):
    """ap_conv_d0_fwd_bf16: Conv2d(1 | 2, 64, 4, stride 2, pad 1) + bias + activation (networks.py:2620-2623) through
    ConvLayer.run = fp32-accumulated sums of bf16(x) x bf16(w), plus the bias, activated."""
    from animateportrait_amd import ops
    from animateportrait_amd.networks import ConvLayer
    n, cin, H, W, act = case
    monkeypatch.setattr(ops, 'DEFAULT_PRECISION', ops.PRECISION_BF16)
    gen = torch.Generator().manual_seed(67 + sum(case))
    layer = ConvLayer([cin], 64, 4, 2, 1).to(dev)
    layer.spec.precision = ops.PRECISION_BF16
    w = torch.randn(64, cin, 4, 4, generator=gen) * 0.1
    b = torch.randn(64, generator=gen) * 0.1
    x = torch.randn(n, cin, H, W, generator=gen)
    with torch.no_grad():
        layer.weight.copy_(w); layer.bias.copy_(b)
    with profiled() as prof:
        y = layer.run(ops.Feat(x.to(dev)), act=act)
    assert prof.calls.get('conv_d0<%d>' % cin) == 1, prof.calls
    assert not y.virtual and tuple(y.data.shape) == (n, 64, H // 2, W // 2)

    def ref(xv, wv):
        r = F.conv2d(xv, wv, b.double(), stride=2, padding=1)
        return F.relu(r) if act == 1 else (F.leaky_relu(r, 0.2) if act == 2 else r)
    check_bf16(y.data, ref(r16(x), r16(w)), ref(x.double(), w.double()), case)


# ---------------------------------------------------------------- the last layer's data gradient (dgrad_k7_final_kernel)

FINAL_DGRAD = [
    # n, c, H, W
    (1, 32, 1, 16),
    (2, 64, 1, 256),
    (1, 64, 2, 16),
    (3, 32, 2, 256),
    (2, 32, 3, 16),
    (1, 64, 3, 256),
]


def _final_dgrad_ref(w, gy):
    n, _, H, W = gy.shape
    c = w.shape[1]
    xp = torch.zeros(n, c, H + 6, W + 6, dtype=torch.float64, requires_grad=True)
    (F.conv2d(xp, w) * gy).sum().backward()
    return xp.grad


@pytest.mark.parametrize('case', FINAL_DGRAD, ids=lambda c: 'N%d C%d %dx%d' % c)
def test_final_dgrad_on_the_fewest_rows(dev, case):
    """ap_conv_final_dgrad_bf16 at 1-3 rows (served; below 4 rows the reflection fold is undefined, so the gradient is checked in
    padded coordinates): the fp32-accumulated sums of bf16(w) x bf16(g)."""
    from animateportrait_amd import ops, _capi
    n, c, H, W = case
    assert _capi.lib().ap_conv_final_dgrad_bf16_ok(n, c, H, W) == 1
    gen = torch.Generator().manual_seed(71 + sum(case))
    w = torch.randn(1, c, 7, 7, generator=gen) * 0.05
    gy = torch.randn(n, 1, H, W, generator=gen)
    with profiled() as prof:
        gp = ops.final_dgrad_k7(ops.Feat(gy.to(dev)), w.to(dev))
    assert prof.calls.get('dgrad_k7<final>') == 1, prof.calls
    assert tuple(gp.shape) == (n, c, H + 6, W + 6)
    check_bf16(gp, _final_dgrad_ref(r16(w), r16(gy)), _final_dgrad_ref(w.double(), gy.double()), case)
    assert torch.equal(gp, ops.final_dgrad_k7(ops.Feat(gy.to(dev)), w.to(dev)))


@pytest.mark.parametrize('case', [(1, 32, 1, 16), (3, 64, 2, 256)], ids=lambda c: 'N%d C%d %dx%d' % c)
def test_final_dgrad_c_abi_stays_in_its_workspace(dev, case):
    from animateportrait_amd import ops, _capi
    lib = _capi.lib()
    n, c, H, W = case
    gen = torch.Generator().manual_seed(73 + sum(case))
    w = (torch.randn(1, c, 7, 7, generator=gen) * 0.05).to(dev)
    gy = torch.randn(n, 1, H, W, generator=gen).to(dev)
    nws = lib.ap_conv_final_dgrad_bf16_workspace_floats(n, c, H, W)
    ws = nan_workspace(nws, dev)
    gp = torch.empty(n, c, H + 6, W + 6, dtype=torch.float32, device=dev)
    _capi.check(lib.ap_conv_final_dgrad_bf16(ops._ptr(gy), ops._ptr(w), n, c, H, W, ops._ptr(ws), ops._ptr(gp), ops._stream()), 'conv_final_dgrad_bf16')
    assert_tail_untouched(ws, nws, 'conv_final_dgrad_bf16')
    assert torch.equal(gp, ops.final_dgrad_k7(ops.Feat(gy), w))


# ---------------------------------------------------------------- the InstanceNorm backward that writes the operands (ap_instnorm_bwd_split)

def inbwd_ref(y, mean, rstd, act, g1, fold, g2):
    """fp64 InstanceNorm backward as the kernel defines it: xhat = (y - mean) rstd from the stored y and the given statistics;
    g' = act'(xhat) (fold(g1) + g2); dy = rstd (g' - mean g' - xhat mean(g' xhat)).  fold 1: g1 is the gradient of a
    reflection-padded (pad 1) consumer, folded back by the backward of F.pad."""
    n, c, h, w = y.shape
    if fold:
        t = torch.zeros(n, c, h, w, dtype=torch.float64, requires_grad=True)
        (F.pad(t, (1,) * 4, mode='reflect') * g1.double()).sum().backward()
        g = t.grad
    else:
        g = g1.double()
    if g2 is not None:
        g = g + g2.double()
    m, r = mean.double().view(n, c, 1, 1), rstd.double().view(n, c, 1, 1)
    xh = (y.double() - m) * r
    if act == 1:
        g = g * (xh > 0).double()
    elif act == 2:
        g = torch.where(xh > 0, g, 0.2 * g)
    return r * (g - g.mean((2, 3), keepdim=True) - xh * (g * xh).mean((2, 3), keepdim=True))


SPLIT = [
    # n, c, H, W, y as bf16, g1 as bf16, fold, second gradient, act, plain bf16 (head planes only)
    (2, 64, 32, 32, False, False, 0, False, 1, False),      # H W = 1024: the 256-thread kernel
    (2, 64, 13, 80, False, False, 0, True, 2, True),        # 1040: the 1024-thread kernel
    (2, 64, 32, 32, False, False, 1, True, 0, True),
    (2, 64, 13, 80, False, False, 1, False, 1, False),
    (2, 64, 32, 32, False, True, 0, False, 2, True),
    (2, 64, 13, 80, False, True, 0, True, 1, True),
    (2, 64, 32, 32, False, True, 1, False, 1, True),
    (2, 64, 13, 80, False, True, 1, True, 2, True),
    (2, 64, 32, 32, True, False, 0, True, 0, True),
    (2, 64, 13, 80, True, False, 0, False, 1, True),
    (2, 64, 32, 32, True, False, 1, False, 2, True),
    (2, 64, 13, 80, True, False, 1, True, 1, True),
    (2, 64, 32, 32, True, True, 0, False, 1, True),
    (2, 64, 13, 80, True, True, 0, True, 2, True),
    (2, 64, 32, 32, True, True, 1, True, 1, True),
    (2, 64, 13, 80, True, True, 1, False, 0, True),
    (1, 64, 8, 512, False, False, 1, False, 1, False),      # H W = 4096 as one long row band ...
    (1, 64, 512, 8, True, True, 1, True, 1, True),          # ... and as one pixel octet per row
    (3, 16, 3, 64, False, False, 0, True, 1, False),        # the fewest rows
    (2, 8, 4, 8, True, True, 1, False, 2, True),            # one channel octet, the fewest rows with the fold, the narrowest rows
    (17, 512, 32, 32, True, True, 1, False, 1, True),       # 1088 items: more than the resident 256-thread workgroups
    (9, 256, 13, 80, False, False, 1, True, 1, False),      # 288 items: more than the resident 1024-thread workgroups
]


def _split_id(s):
    n, c, h, w, yb, gb, fold, second, act, heads = s
    return 'N%d C%d %dx%d %s %s fold%d%s act%d %s' % (n, c, h, w, 'y16' if yb else 'y32', 'g16' if gb else 'g32', fold,
                                                      ' +g2' if second else '', act, 'bf16' if heads else 'bf16x3')


@pytest.mark.parametrize('case', SPLIT, ids=[_split_id(s) for s in SPLIT])
def test_instnorm_bwd_split_variants(dev, monkeypatch, case):
    """Every template variant (y and g1 stored as fp32 or bf16, fold 0 or 1) of ap_instnorm_bwd_split on both thread counts, at the
    edges of its region and with more items than resident workgroups: dy against the fp64 backward of the values the kernel
    reads; the split copy, the strip and the weight gradient's operand bitwise what the separate passes make of that dy."""
    from animateportrait_amd import ops
    n, c, H, W, yb, gb, fold, second, act, heads = case
    prec = ops.PRECISION_BF16 if heads else ops.PRECISION_BF16X3
    monkeypatch.setattr(ops, 'DEFAULT_PRECISION', prec)
    monkeypatch.delenv('APAMD_NO_INBWD_SPLIT', raising=False)
    gen = torch.Generator().manual_seed(79 + n + c + H + W + 2 * yb + 4 * gb + 8 * fold + act)
    y32 = torch.randn(n, c, H, W, generator=gen) * 1.7 + 0.4
    mean = y32.mean((2, 3)).reshape(-1)
    rstd = (y32.var((2, 3), unbiased=False) + 1e-5).rsqrt().reshape(-1)
    g1_32 = torch.randn(n, c, H + 2 * fold, W + 2 * fold, generator=gen)
    g2 = torch.randn(n, c, H, W, generator=gen) if second else None
    y = y32.bfloat16() if yb else y32
    g1 = g1_32.bfloat16() if gb else g1_32
    f = ops.Feat(y.to(dev), mean.to(dev), rstd.to(dev), act)
    assert ops.instnorm_bwd_split_ok(f, fold)
    # the weight gradient's operand with padded dimensions: what lies outside the H x W x C gradient must stay zero
    dims = (H + 2, W // 8 + 1, c + 8)
    with profiled() as prof:
        gf, gt, strip = ops.instnorm_bwd_split((g1.to(dev), fold, None if g2 is None else g2.to(dev)), f, dims,
                                               want_xs=True, want_strip=True, want_dy=True)
    assert prof.calls == {'instnorm_bwd_split<%d>' % (H * W // 4): 1}, prof.calls
    dy = gf.data
    ref = inbwd_ref(y.double(), mean, rstd, act, g1.double(), fold, g2)
    sc = float(ref.abs().max())
    err = linf(dy, ref) / sc
    assert err < 3e-5, (case, err)
    if yb or gb:
        # the stored bf16 values are what the kernel reads, not the fp32 values they were rounded from
        exact = inbwd_ref(y32.double(), mean, rstd, act, g1_32.double(), fold, g2)
        assert linf(dy, exact) / sc > 10 * err, (case, err)
    # operands: bitwise what the separate passes make of THIS dy
    xs_ref = ops.presplit(ops.Feat(dy.clone()), prec)
    a, b = gf.xs.view(n, 2, -1), xs_ref.view(n, 2, -1)
    assert torch.equal(a[:, 0], b[:, 0]), 'split copy, head planes'
    if not heads:
        assert torch.equal(a[:, 1], b[:, 1]), 'split copy, tail planes'
    assert torch.equal(strip.data, dy[:, :, :, W - 2:].transpose(2, 3).contiguous()), 'dgrad strip'
    # gt [n][part][GHp][GX8][Mp][8 pixels]: part 0 = bf16(dy), part 1 = bf16(dy - bf16(dy)); zero outside the gradient
    head = dy.bfloat16()
    parts = [head] + ([] if heads else [(dy - head.float()).bfloat16()])
    gt_ref = torch.zeros(n, 2, dims[0], dims[1], dims[2], 8, dtype=torch.bfloat16, device=dev)
    for p, v in enumerate(parts):
        gt_ref[:, p, :H, :W // 8, :c] = v.view(n, c, H, W // 8, 8).permute(0, 2, 3, 1, 4)
    got = gt.view(torch.bfloat16).view(n, 2, dims[0], dims[1], dims[2], 8)
    assert torch.equal(got[:, :len(parts)].view(torch.int16), gt_ref[:, :len(parts)].view(torch.int16)), 'weight gradient operand'
    # and the same call again gives the same bits
    gf2, gt2, strip2 = ops.instnorm_bwd_split((g1.to(dev), fold, None if g2 is None else g2.to(dev)), f, dims,
                                              want_xs=True, want_strip=True, want_dy=True)
    assert torch.equal(gf2.data, dy) and torch.equal(gt2, gt) and torch.equal(strip2.data, strip.data)


def test_instnorm_bwd_three_rows_with_the_fold_is_not_split(dev):
    """3 rows with the pad-1 fold: both border rows fold into row 1, which the split kernel's one-border-row-per-lane form cannot
    do (it dropped the second: 0.6 of the scale off) -- the predicate refuses the shape, and the general backward that serves it
    instead matches fp64."""
    from animateportrait_amd import ops
    n, c, H, W = 2, 64, 3, 16
    gen = torch.Generator().manual_seed(83)
    y = torch.randn(n, c, H, W, generator=gen) * 1.7 + 0.4
    mean = y.mean((2, 3)).reshape(-1)
    rstd = (y.var((2, 3), unbiased=False) + 1e-5).rsqrt().reshape(-1)
    g1 = torch.randn(n, c, H + 2, W + 2, generator=gen)
    f = ops.Feat(y.to(dev), mean.to(dev), rstd.to(dev), ops.ACT_RELU)
    assert not ops.instnorm_bwd_split_ok(f, 1) and ops.instnorm_bwd_split_ok(f, 0)
    dy = ops.instnorm_bwd([(g1.to(dev), 1)], f)
    ref = inbwd_ref(y.double(), mean, rstd, ops.ACT_RELU, g1.double(), 1, None)
    assert linf(dy, ref) / float(ref.abs().max()) < 3e-5
