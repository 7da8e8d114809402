"""The generator's output layer -- ReflectionPad2d(3) + Conv2d(64, 1, 7) + Tanh on a source that carries deferred InstanceNorm
statistics + ReLU -- through the product path (ConvLayer.run -> ops.conv2d -> ap_conv2d_fwd), against a float64 CPU evaluation.

In split-bf16 arithmetic the layer runs as a tap GEMM on the matrix pipe with a shift-add of its result (csrc/conv_tapgemm.h):
tiles of 58 output columns, walked in row bands whose height the launcher picks between 8 rows and the whole plane.  The shapes
below are the smallest at which that structure can go wrong: a plane that is all border (4 x 4), planes ragged against the tile
and the band in both directions, exactly one tile and one band (8 x 58) and one pixel more each way, several tiles and bands with
N = 3, different statistics per sample, ReLU active on half the inputs / on none, and single-pixel inputs, whose output is the
reflected weight stencil (tap-index and shift-direction errors show exactly).  The same cases run in exact fp32, which keeps the
vector-ALU kernel (csrc/conv_direct.h); the plan name is the same for both bodies, so ops.LaunchProfiler cannot tell which ran.

Tolerances: the relative L-inf bounds tests/test_gpu_parity.py applies to split-bf16 and exact-fp32 convolution layers against
fp64 (5e-5 and 2e-6 of the largest pre-activation magnitude); tanh is 1-Lipschitz, so the bound holds behind it.

The three-channel form (DirectCfg<7, 4>) is untouched by the matrix-pipe body: tests/golden/final_layer_cop4.npz holds its output
on a 33 x 47 plane as computed at commit 30ee566 (the parent of the change that added conv_tapgemm.h), recorded there with
``python tests/test_final_layer_gpu.py --record``; it must stay bit-equal."""
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_COP4 = os.path.join(ROOT, 'tests', 'golden', 'final_layer_cop4.npz')
GOLDEN_PLANS = os.path.join(ROOT, 'tests', 'golden', 'conv_plans.json')
TOL_BF16X3, TOL_FP32 = 5e-5, 2e-6          # as tests/test_gpu_parity.py (split-bf16 / exact-fp32 layers against fp64)

CASES = {
    # name: (N, H, W, kind)
    'all_border_4x4': (1, 4, 4, 'mixed'),
    'ragged_7x9': (1, 7, 9, 'mixed'),
    'ragged_33x47_n2': (2, 33, 47, 'mixed'),
    'one_tile_one_band_8x58': (1, 8, 58, 'mixed'),
    'one_more_each_way_9x59': (1, 9, 59, 'mixed'),
    'tiles_and_bands_64x64_n3': (3, 64, 64, 'mixed'),
    'all_positive_20x70': (2, 20, 70, 'positive'),
    'impulse_corner_and_centre_17x61': (2, 17, 61, 'impulse'),
}


def make_case(name, cout=1):
    """Inputs (CPU, fp32) and the float64 result of one case; 'mixed': about half the normalised inputs are negative."""
    n, h, w, kind = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)) + 17 * cout)
    wt = torch.randn(cout, 64, 7, 7, generator=g) * 0.05
    b = torch.randn(cout, generator=g) * 0.3
    if kind == 'impulse':
        x = torch.zeros(n, 64, h, w)
        x[0, 5, 0, 0] = 1.5             # sample 0: a corner pixel
        x[1, 41, h // 2, w // 2] = 2.0  # sample 1: the centre pixel
        m, r = torch.zeros(n, 64), torch.ones(n, 64)
    elif kind == 'positive':
        x = torch.rand(n, 64, h, w, generator=g) * 2.0 + 0.5
        m, r = torch.rand(n, 64, generator=g) * 0.4, torch.rand(n, 64, generator=g) + 0.5
    else:
        x = torch.randn(n, 64, h, w, generator=g) * 1.5 + 0.2
        m, r = torch.randn(n, 64, generator=g) * 0.3 + 0.2, torch.rand(n, 64, generator=g) + 0.4   # per sample and channel
    xn = F.relu((x.double() - m.double().view(n, 64, 1, 1)) * r.double().view(n, 64, 1, 1))
    pre = F.conv2d(F.pad(xn, (3,) * 4, mode='reflect'), wt.double(), b.double())
    return dict(x=x, m=m, r=r, w=wt, b=b, pre=pre, ref=torch.tanh(pre), negative=float((xn == 0).double().mean()))


_REFS = {}


def case(name):
    if name not in _REFS:
        _REFS[name] = make_case(name)
    return _REFS[name]


def run_layer(c, precision, dev, cout=1):
    from animateportrait_amd import ops
    from animateportrait_amd.networks import ConvLayer
    layer = ConvLayer([64], cout, 7, 1, 3, ops.PAD_REFLECT).to(dev)
    layer.spec.precision = precision
    with torch.no_grad():
        layer.weight.copy_(c['w'])
        layer.bias.copy_(c['b'])
    src = ops.Feat(c['x'].to(dev), c['m'].reshape(-1).to(dev), c['r'].reshape(-1).to(dev), ops.ACT_RELU)
    prof = ops.LaunchProfiler()
    ops.PROFILER = prof
    try:
        y = layer.run(src, act=ops.ACT_TANH)
    finally:
        ops.PROFILER = None
    torch.cuda.synchronize()
    return y.data, [rec[0] for rec in prof.records]


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(CASES))
@pytest.mark.parametrize('precision', ['bf16x3', 'fp32'])
def test_final_layer_against_fp64(dev, name, precision):
    from animateportrait_amd import ops
    c = case(name)
    kind = CASES[name][3]
    if kind == 'mixed':
        assert 0.3 < c['negative'] < 0.7        # ReLU active on about half the inputs
    if kind == 'positive':
        assert c['negative'] == 0.0
    y, names = run_layer(c, ops.PRECISION_BF16X3 if precision == 'bf16x3' else ops.PRECISION_FP32, dev)
    assert names == ['DirectCfg<7, 1>']             # one launch, the direct route, in either arithmetic
    # ... and which body of that route ran: the tap GEMM in split-bf16 arithmetic, the vector-ALU kernel in fp32
    spec = ops.ConvSpec([64], 1, 7, 1, 3, ops.PAD_REFLECT)
    spec.precision = ops.PRECISION_BF16X3 if precision == 'bf16x3' else ops.PRECISION_FP32
    route = ops.conv_fwd_route(spec, *c['x'].shape[0:1], *c['x'].shape[2:])
    assert route.split()[0] == ('tapgemm' if precision == 'bf16x3' else 'direct<7,1>'), route
    assert y.shape == c['ref'].shape
    scale = float(c['pre'].abs().max())
    err = float((y.double().cpu() - c['ref']).abs().max()) / scale
    print('%s %s: L-inf / scale = %.3g (scale %.3g)' % (name, precision, err, scale))
    assert err < (TOL_BF16X3 if precision == 'bf16x3' else TOL_FP32), err


@pytest.mark.gpu
def test_impulse_output_is_the_reflected_stencil(dev):
    """Sample 0 has one non-zero input at the corner (0, 0) of channel 5, sample 1 one at the centre of channel 41: before bias
    and tanh the output is that channel's 7x7 weights, flipped, centred on the pixel and folded back at the border."""
    from animateportrait_amd import ops
    c = case('impulse_corner_and_centre_17x61')
    n, h, w, _ = CASES['impulse_corner_and_centre_17x61']
    want = torch.zeros(n, 1, h, w, dtype=torch.float64)
    for s, ch, py, px, v in ((0, 5, 0, 0, 1.5), (1, 41, h // 2, w // 2, 2.0)):
        for ky in range(7):
            for kx in range(7):
                # the padded pixel (oy + ky - 3, ox + kx - 3) reads (py, px), directly or through the reflection
                for oy in {q - ky + 3 for q in (py, -py, 2 * (h - 1) - py)}:
                    for ox in {q - kx + 3 for q in (px, -px, 2 * (w - 1) - px)}:
                        if 0 <= oy < h and 0 <= ox < w:
                            want[s, 0, oy, ox] += v * float(c['w'][0, ch, ky, kx])
    want = torch.tanh(want + c['b'].double().view(1, 1, 1, 1))
    assert float((want - c['ref']).abs().max()) < 1e-12          # the stencil, restated, is what the fp64 convolution gives
    y, _ = run_layer(c, ops.PRECISION_BF16X3, dev)
    assert float((y.double().cpu() - want).abs().max()) < TOL_BF16X3 * float(c['pre'].abs().max())


def cop4_inputs():
    return make_case('ragged_33x47_n2', cout=3)


@pytest.mark.gpu
@pytest.mark.parametrize('precision', ['bf16x3', 'fp32'])
def test_three_channel_form_is_bit_equal_to_the_recorded_parent(dev, precision):
    from animateportrait_amd import ops
    c = cop4_inputs()
    z = np.load(GOLDEN_COP4)
    assert np.array_equal(z['x_head'], c['x'].reshape(-1)[:64].numpy())          # the generator still yields the recorded inputs
    y, names = run_layer(c, ops.PRECISION_BF16X3 if precision == 'bf16x3' else ops.PRECISION_FP32, dev, cout=3)
    assert names == ['DirectCfg<7, 4>']
    assert np.array_equal(y.cpu().numpy().view(np.uint32), z['y_' + precision].view(np.uint32))


def test_final_layer_plan_answers_are_the_recorded_rows():
    """CPU: the planner's answers for this layer's descriptor equal the rows of tests/golden/conv_plans.json -- the matrix-pipe
    body is chosen below the planner, so the status, output size, packed floats, statistics tiles, plan name and flags stay.
    The golden sweep holds the descriptor in exact fp32 and split-bf16; plain bf16 must answer as they do."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import test_conv_plan_cpu as tp
    from animateportrait_amd import _capi
    lib = _capi.lib()
    with open(GOLDEN_PLANS) as f:
        golden = json.load(f)
    layer = tp._layer((64,), 1, 7, 1, 3, tp.REFLECT)
    key = [[list(layer[0])] + list(layer[1:]), [2, 64, 48]]
    rows = {r[0]: r[3] for r in golden if r[1:3] == key}
    assert set(rows) >= {tp.FP32, tp.BF16X3}
    for prec in (tp.FP32, tp.BF16X3, tp.BF16):
        got = tp.answers(lib, prec, layer, (2, 64, 48))
        assert got == rows.get(prec, rows[tp.BF16X3]), (prec, got)
        assert got[6] == 'DirectCfg<7, 1>' and got[3] == 64 * 49 and got[5] == 0


if __name__ == '__main__' and '--record' in sys.argv:
    sys.path.insert(0, ROOT)
    from animateportrait_amd import ops
    c = cop4_inputs()
    out = {'x_head': c['x'].reshape(-1)[:64].numpy()}
    for pname, prec in (('bf16x3', ops.PRECISION_BF16X3), ('fp32', ops.PRECISION_FP32)):
        y, names = run_layer(c, prec, torch.device('cuda:0'), cout=3)
        assert names == ['DirectCfg<7, 4>']
        out['y_' + pname] = y.cpu().numpy()
    np.savez(os.environ.get('FINAL_LAYER_GOLDEN_OUT', GOLDEN_COP4), **out)
    print('recorded', {k: v.shape for k, v in out.items()})
