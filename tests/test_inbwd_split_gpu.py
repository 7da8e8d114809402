"""GPU (-m gpu): ap_instnorm_bwd_split -- the InstanceNorm backward that writes the operands of the bf16 matrix kernels itself
(split copy for the data gradient, M-role operand of the weight gradient, the dgrad strip) instead of an fp32 dy that two more
passes would round to bf16.  Checked (a) against the two-pass route kernel by kernel: same dy up to the order of the plane sums,
operands BITWISE what the separate passes make of that dy; (b) against autograd of the reference's layer composition
(conv -> nn.InstanceNorm2d -> ReLU, networks.py:2329-2421) through a layer's whole backward, with the switch on and off."""
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import linf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


SHAPES = [
    # n, c, h, w, fold, second gradient, act
    (2, 64, 64, 64, 1, False, 1),
    (2, 64, 64, 64, 0, True, 0),
    (3, 128, 32, 32, 0, False, 2),
    (2, 72, 24, 40, 1, True, 1),       # C not a multiple of 64 (padded channel slots), idle threads, ragged octet rows
    (1, 256, 16, 8, 0, False, 1),
]


@pytest.mark.parametrize('heads_only', [False, True], ids=['bf16x3', 'bf16'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_kernel_outputs_match_the_two_pass_route(dev, monkeypatch, shape, heads_only):
    from animateportrait_amd import ops
    n, c, h, w, fold, second, act = shape
    prec = ops.PRECISION_BF16 if heads_only else ops.PRECISION_BF16X3
    monkeypatch.setattr(ops, 'DEFAULT_PRECISION', prec)
    g = torch.Generator().manual_seed(n * 1000 + c + h + w)
    y = (torch.randn(n, c, h, w, generator=g) * 1.7 + 0.4).to(dev)
    mean = y.mean((2, 3)).reshape(-1).contiguous()
    rstd = (y.var((2, 3), unbiased=False) + 1e-5).rsqrt().reshape(-1).contiguous()
    f = ops.Feat(y, mean, rstd, act)
    g1 = torch.randn(n, c, h + 2 * fold, w + 2 * fold, generator=g).to(dev)
    contribs = [(g1, fold)]
    if second:
        contribs.append((torch.randn(n, c, h, w, generator=g).to(dev), 0))
    assert ops.instnorm_bwd_split_ok(f, fold)
    ref = ops.instnorm_bwd(list(contribs), f)
    # the layer this gradient belongs to: 3x3 stride 1 over a 64-channel input (weight gradient on the bf16 matrix kernel)
    src = ops.Feat(torch.randn(n, 64, h, w, generator=g).to(dev))
    dims = ops.wgrad_gt_dims(3, 1, 1, ops.PAD_ZERO, (n, c, h, w), [src], prec)
    assert dims is not None and dims[0] >= h and dims[1] * 8 >= w and dims[2] >= c
    gf, gt, strip = ops.instnorm_bwd_split(ops._split_contribs(list(contribs)), f, dims, want_xs=True, want_strip=True, want_dy=True)
    sc = float(ref.abs().max())
    assert linf(gf.data, ref) <= 2e-6 * sc, 'dy (plane sums in another order)'
    # operands: bitwise what the separate passes make of THIS dy
    two = ops.Feat(gf.data.clone())
    xs_ref = ops.presplit(two, prec)
    a, b = gf.xs.view(n, 2, -1), xs_ref.view(n, 2, -1)
    assert torch.equal(a[:, 0], b[:, 0]), 'split copy, head planes'
    if not heads_only:
        assert torch.equal(a[:, 1], b[:, 1]), 'split copy, tail planes'
    assert torch.equal(strip.data, gf.data[:, :, :, w - 2:].transpose(2, 3).contiguous()), 'dgrad strip'
    dw_pre = ops.wgrad(3, 1, 1, ops.PAD_ZERO, gf, [src], (c, 64, 3, 3), precision=prec, g_t=gt)
    dw_two = ops.wgrad(3, 1, 1, ops.PAD_ZERO, two, [src], (c, 64, 3, 3), precision=prec)
    assert torch.equal(dw_pre, dw_two), 'weight gradient from the prepared operand'


LAYERS = [
    # name, cin, cout, k, stride, pad, mode, H, W
    ('trunk 3x3 reflect 64x64', 64, 64, 3, 1, 1, 'reflect', 64, 64),
    ('3x3 zero 32x32', 64, 128, 3, 1, 1, 'zero', 32, 32),
    ('patchgan 4x4 s2 -> 32x32', 64, 128, 4, 2, 1, 'zero', 64, 64),
    ('down 3x3 s2 -> 32x64', 64, 64, 3, 2, 1, 'zero', 64, 128),
]


@pytest.mark.parametrize('case', LAYERS, ids=[c[0] for c in LAYERS])
def test_layer_backward_with_prepared_operands_vs_autograd(dev, case):
    """conv -> InstanceNorm -> (upstream gradient): input and weight gradients of the layer through the tape, with the fused
    backward (default) and with APAMD_NO_INBWD_SPLIT=1, against fp64 autograd of the reference composition.  The switch changes
    which kernels run (asserted on the plan), not the result beyond fp32 rounding.  No activation here: a ReLU gate on a
    normalised value within 2^-17 of zero opens on one side and not on the other, which moves single gradient elements by O(1)
    in both routes alike (first version of this test: 4-6 % L-inf on the stride-2 cases, identical to 1e-8 between the routes);
    the gates are covered by the kernel-level test above, where both routes see the same y."""
    from animateportrait_amd import ops, autograd
    from animateportrait_amd.networks import ConvLayer
    name, cin, cout, k, stride, pad, mode, H, W = case
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    n = 2
    x = torch.randn(n, cin, H, W, generator=g)
    wt = torch.randn(cout, cin, k, k, generator=g) * 0.05
    outs = {}
    for off in ('0', '1'):
        os.environ['APAMD_NO_INBWD_SPLIT'] = off
        try:
            layer = ConvLayer([cin], cout, k, stride, pad, ops.PAD_REFLECT if mode == 'reflect' else ops.PAD_ZERO, False, 0).to(dev)
            with torch.no_grad():
                layer.weight.copy_(wt); layer.bias.zero_()
            tape = autograd.Tape()
            fx = tape.track(ops.Feat(x.to(dev)))
            out = autograd.conv_forward(tape, layer, [fx], norm_act=ops.ACT_NONE)
            gy = torch.randn(out.data.shape, generator=torch.Generator().manual_seed(5))
            plan = autograd._backward_plan(tape, layer, [fx], out, True, ops.ACT_NONE, [(gy.to(dev), 0)])
            assert (plan.norm_route == 'split') == (off == '0'), (name, off)
            tape.add(out, gy.to(dev), 0)
            tape.backward()
            g1, p, g2 = ops._split_contribs(tape.take(fx))
            dx = g1 if (p == 0 and g2 is None) else ops.fold_add(g1, p, g2)
            outs[off] = (dx.cpu(), tape.param_grads[layer.weight].cpu())
        finally:
            os.environ.pop('APAMD_NO_INBWD_SPLIT', None)
    xd = x.double().requires_grad_(True)
    wd = wt.double().requires_grad_(True)
    xp = F.pad(xd, (pad,) * 4, mode='reflect') if mode == 'reflect' else F.pad(xd, (pad,) * 4)
    yr = F.instance_norm(F.conv2d(xp, wd, None, stride=stride), eps=1e-5)
    (yr * gy.double()).sum().backward()
    errs = {off: (linf(outs[off][0], xd.grad) / float(xd.grad.abs().max()), linf(outs[off][1], wd.grad) / float(wd.grad.abs().max()))
            for off in ('0', '1')}
    for off in ('0', '1'):
        assert errs[off][0] <= 2e-4 and errs[off][1] <= 2e-4, (name, 'NO_INBWD_SPLIT=' + off, '(dgrad, wgrad) errors', errs)
    # the two routes round the same fp32 gradient to the same bf16 operands: they agree far inside the bar above
    assert linf(outs['0'][0], outs['1'][0]) <= 2e-5 * float(xd.grad.abs().max()), name
    assert linf(outs['0'][1], outs['1'][1]) <= 2e-5 * float(wd.grad.abs().max()), name
