"""GPU (-m gpu): the luminance kernel of cartoon training (losses.luminance -> aps_luma_fwd / aps_luma_bwd,
csrc/style/style_luma.hip) against the same expression in float64 on the CPU, forward and backward, on the shapes where its two
bodies and their edges meet: the smallest input, a plane that is no multiple of four (element-wise body only), planes that are
(128-bit body, nothing left), several samples with odd rows, and an aligned shape behind a misaligned pointer."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K = (0.299, 0.587, 0.114)
EPS = float(np.finfo(np.float32).eps)
U = EPS / 2                              # unit roundoff: one fp32 rounding of a value v moves it by at most U |v|
# Forward, inputs in [-1, 1]: y = fl(fl(fl(kR r) + fl(kG g)) + fl(kB b)) with the constants themselves rounded to fp32.
#   constants:  |k_c(fp32) - k_c| <= U k_c          -> U (kR + kG + kB)
#   products:   three roundings of values <= k_c    -> U (kR + kG + kB)
#   first sum:  one rounding of a value <= kR + kG  -> U (kR + kG)
#   second sum: one rounding of a value <= 1        -> U
# (second-order terms are below 1e-14.)  That is 3.886 U: just under two ulp of 1.
TOL_FWD = U * (2 * sum(K) + (K[0] + K[1]) + 1.0) * (1 + 4 * EPS)
# Backward, dY in [-1, 1]: gx_c = fl(k_c(fp32) g): the constant's rounding and the product's, each U k_c |g|
TOL_BWD = [2 * U * k * (1 + 4 * EPS) for k in K]

SHAPES = [(1, 3, 1, 1), (2, 3, 5, 7), (1, 3, 8, 260), (3, 3, 9, 258), (4, 3, 6, 8)]


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


def _case(shape, seed):
    g = torch.Generator().manual_seed(seed)
    n, _, h, w = shape
    x = torch.rand(shape, generator=g) * 2 - 1
    dy = torch.rand((n, 1, h, w), generator=g) * 2 - 1          # differs per pixel: swapped indices would show
    x64 = x.double()
    y64 = K[0] * x64[:, 0:1] + K[1] * x64[:, 1:2] + K[2] * x64[:, 2:3]
    gx64 = torch.cat([k * dy.double() for k in K], 1)
    return x, dy, y64, gx64


def _check(y, gx, y64, gx64):
    assert y.shape == y64.shape and y.dtype == torch.float32 and gx.shape == gx64.shape
    e = float((y.double().cpu() - y64).abs().max())
    print('forward  L-inf %.3e (bound %.3e)' % (e, TOL_FWD))
    assert e <= TOL_FWD
    for c in range(3):
        e = float((gx[:, c].double().cpu() - gx64[:, c]).abs().max())
        print('backward channel %d L-inf %.3e (bound %.3e)' % (c, e, TOL_BWD[c]))
        assert e <= TOL_BWD[c]


@pytest.mark.parametrize('shape', SHAPES)
def test_luminance_forward_and_backward_vs_float64(dev, shape):
    from animateportrait_amd import losses
    x, dy, y64, gx64 = _case(shape, seed=sum(shape))
    xd = x.to(dev).requires_grad_(True)
    y = losses.luminance(xd)
    y.backward(dy.to(dev))
    _check(y.detach(), xd.grad, y64, gx64)
    # the reference's own fp32 chain (geomgm_ifw_cartoon_fore_model.py:745), evaluated by torch on the CPU: same bits
    chain = 0.299 * x[:, 0:1] + 0.587 * x[:, 1:2] + 0.114 * x[:, 2:3]
    assert torch.equal(y.detach().cpu(), chain)


def test_misaligned_pointers_take_the_elementwise_body(dev):
    """H W % 4 == 0 but neither tensor starts on a 16-byte boundary: the plan must not issue 128-bit accesses"""
    from animateportrait_amd import _styleapi as S
    from animateportrait_amd.ops import _ptr, _stream
    shape = (2, 3, 8, 260)
    x, dy, y64, gx64 = _case(shape, seed=5)
    n, _, h, w = shape
    xb = torch.full((x.numel() + 8,), float('nan'), device=dev)
    yb, gb, gxb = torch.full((n * h * w + 8,), float('nan'), device=dev), torch.full((n * h * w + 8,), float('nan'), device=dev), \
        torch.full((x.numel() + 8,), float('nan'), device=dev)
    xv, yv, gv, gxv = xb[1:1 + x.numel()], yb[3:3 + n * h * w], gb[2:2 + n * h * w], gxb[1:1 + x.numel()]
    assert xv.data_ptr() % 16 == 4 and yv.data_ptr() % 16 == 12
    xv.copy_(x.reshape(-1))
    gv.copy_(dy.reshape(-1))
    assert S.lib().aps_luma_ok(_ptr(xv), _ptr(yv), n, h, w) == 1
    S.check(S.lib().aps_luma_fwd(_ptr(xv), n, h, w, _ptr(yv), _stream()), 'luma_fwd')
    S.check(S.lib().aps_luma_bwd(_ptr(gv), n, h, w, _ptr(gxv), _stream()), 'luma_bwd')
    _check(yv.view(n, 1, h, w), gxv.view(n, 3, h, w), y64, gx64)
    for buf, lo, hi in ((yb, 3, 3 + n * h * w), (gxb, 1, 1 + x.numel())):      # nothing written outside the tensors
        assert bool(torch.isnan(buf[:lo]).all()) and bool(torch.isnan(buf[hi:]).all())


def test_refusals_need_no_launch(dev):
    from animateportrait_amd import _styleapi as S, losses
    lib = S.lib()
    assert lib.aps_luma_ok(None, None, 1, 4, 4) == 0 and lib.aps_luma_ok(16, 16, 0, 4, 4) == 0
    assert lib.aps_luma_ok(16, 16, 1, S.MAX_SIDE + 1, 4) == 0 and lib.aps_luma_ok(16, 16, 1, 4, 4) == 1
    assert lib.aps_luma_fwd(None, 1, 4, 4, None, None) < 0 and 'null' in S.last_error()
    with pytest.raises(ValueError, match='3, H, W'):
        losses.luminance(torch.zeros(1, 1, 4, 4, device=dev))
