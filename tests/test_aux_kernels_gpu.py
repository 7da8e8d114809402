"""GPU (-m gpu): the kernels outside the convolution files -- the LSTM recurrence (csrc/lstm.hip), the spline solve and warp and the
fused Adam (csrc/tps.hip), resize / grid_sample / pixel_shuffle (csrc/image_ops.hip) -- at the edges of their C contracts, each against a
float64 evaluation of the same operation on the CPU.

Every output is a window inside a larger buffer filled with a sentinel; the sentinel has to survive around the window (and, for the
LSTM's strided output, in the columns the call does not own)."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SENT = 1e30
PAD = 64          # floats of sentinel on either side of a window (an even count: the window keeps its 8-byte alignment)


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


def _linf(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


def _window(numel, dev, pad=PAD):
    """(buffer, window): `numel` floats with `pad` floats of sentinel before and behind them."""
    buf = torch.full((numel + 2 * pad,), SENT, dtype=torch.float32, device=dev)
    return buf, buf[pad:pad + numel]


def _assert_band(buf, numel, what, pad=PAD):
    assert bool((buf[:pad] == SENT).all()) and bool((buf[pad + numel:] == SENT).all()), '%s: wrote outside its window' % what


def _untouched(buf):
    return bool((buf == SENT).all())


# ================================================================================================ 1. LSTM recurrence

def _lstm_ref(xproj, whh, h0, c0, reverse, dtype):
    """The recurrence lstm.hip documents, gate order i, f, g, o: (out [B][T][H], c_T [B][H]) in `dtype` on the CPU."""
    xp, w = xproj.to(dtype), whh.to(dtype)
    B, T, G4 = xp.shape
    H = G4 // 4
    h, c = h0.to(dtype).clone(), c0.to(dtype).clone()
    out = torch.empty(B, T, H, dtype=dtype)
    for s in range(T):
        t = T - 1 - s if reverse else s
        gi, gf, gg, go = (xp[:, t] + h @ w.t()).split(H, dim=1)
        c = torch.sigmoid(gf) * c + torch.sigmoid(gi) * torch.tanh(gg)
        h = torch.sigmoid(go) * torch.tanh(c)
        out[:, t] = h
    return out, c


def _lstm_inputs(B, T, H, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    xproj = torch.randn(B, T, 4 * H, generator=g) * scale
    whh = (torch.rand(4 * H, H, generator=g) * 2 - 1) / math.sqrt(H)
    return xproj, whh, torch.randn(B, H, generator=g), torch.randn(B, H, generator=g)


def _lstm_workspace(H, dev):
    """The H > 64 workspace with a marked tail behind its ap_lstm_workspace_bytes(H) bytes."""
    from animateportrait_amd import _capi
    n = int(_capi.lib().ap_lstm_workspace_bytes(H))
    ws = torch.zeros(n + 256, dtype=torch.uint8, device=dev)
    ws[n:] = 0xA5
    return ws, n


def _lstm_device(dev, xproj, whh, h0, c0, reverse, out_stride, out_off):
    """ap_lstm_recurrence with every argument the Python wrapper leaves null: (out [B][T][H], hn, cn) on the CPU, after the
    sentinel checks, the synchronisation and the time-out flag."""
    from animateportrait_amd import ops, _capi
    lib = _capi.lib()
    B, T, G4 = xproj.shape
    H = G4 // 4
    what = 'lstm H=%d B=%d T=%d reverse=%d' % (H, B, T, reverse)
    xd, wd, h0d, c0d = (t.contiguous().to(dev) for t in (xproj, whh, h0, c0))
    obuf, o = _window(B * T * out_stride, dev)
    hbuf, hn = _window(B * H, dev)
    cbuf, cn = _window(B * H, dev)
    ws, wsn = _lstm_workspace(H, dev) if H > 64 else (None, 0)
    wsp = ctypes.c_void_p(ws.data_ptr()) if ws is not None else None
    _capi.check(lib.ap_lstm_recurrence(ops._ptr(xd), ops._ptr(wd), ops._ptr(h0d), ops._ptr(c0d), ops._ptr(o), ops._ptr(hn), ops._ptr(cn),
                                       B, T, H, int(reverse), out_stride, out_off, wsp, ops._stream()), what)
    torch.cuda.synchronize()
    assert lib.ap_lstm_timed_out(wsp, H) == 0, what
    for buf, n in ((obuf, B * T * out_stride), (hbuf, B * H), (cbuf, B * H)):
        _assert_band(buf, n, what)
    if ws is not None:
        assert bool((ws[wsn:] == 0xA5).all()), what + ': wrote behind its workspace'
    rows = o.view(B, T, out_stride).cpu()
    others = torch.cat([rows[:, :, :out_off], rows[:, :, out_off + H:]], 2)
    assert bool((others == SENT).all()), what + ': wrote columns outside [out_off, out_off + H)'
    return rows[:, :, out_off:out_off + H].contiguous(), hn.view(B, H).cpu(), cn.view(B, H).cpu()


def _lstm_check_unit(dev, B, T, H, reverse, out_stride, out_off, seed):
    xproj, whh, h0, c0 = _lstm_inputs(B, T, H, seed)
    out, hn, cn = _lstm_device(dev, xproj, whh, h0, c0, reverse, out_stride, out_off)
    ref, cref = _lstm_ref(xproj, whh, h0, c0, reverse, torch.float64)
    what = 'H=%d B=%d T=%d reverse=%d' % (H, B, T, reverse)
    eh, ec, cmax = _linf(out, ref), _linf(cn, cref), float(cref.abs().max())
    print('lstm %s: |h - h64| = %.3e  |c - c64| = %.3e  max|c| = %.3f' % (what, eh, ec, cmax))
    assert torch.equal(hn, out[:, 0 if reverse else T - 1]), what + ': hn is not the last processed output row'
    assert eh < 2e-5, (what, eh)
    assert ec < 2e-5 * max(1.0, cmax), (what, ec, cmax)


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('H', [1, 16, 48, 64])
def test_lstm_small_kernel_states_batches_and_output_window(dev, H, B):
    """lstm_small_kernel: initial states read, final states written, every batch row at its own offset of xproj / h0 / c0 / out / hn /
    cn, the output a column window of a wider row, T = 1 (no prefetch of a next step) and both directions."""
    for T in (1, 2, 40):
        for reverse in (0, 1):
            _lstm_check_unit(dev, B, T, H, reverse, 2 * H + 3, H + 1, seed=1000 + 97 * H + 11 * B + 2 * T + reverse)


@pytest.mark.parametrize('T', [1, 2, 3, 33])
@pytest.mark.parametrize('H', [256, 512])
def test_lstm_distributed_kernel_first_steps_and_states(dev, H, T):
    """lstm_dist_kernel: T = 1 leaves before the first counter bump, T = 2 and T = 3 are the first reads of either half of the 2 x H
    exchange buffer, T = 33 a short run; initial and final states, the second half of a 2H-wide row, both directions."""
    for reverse in (0, 1):
        _lstm_check_unit(dev, 1, T, H, reverse, 2 * H, H, seed=2000 + H + 2 * T + reverse)


@pytest.mark.parametrize('H,B,T,stride,off', [(64, 3, 40, 2 * 64 + 3, 64 + 1), (256, 1, 33, 512, 256)], ids=['small', 'distributed'])
def test_lstm_saturated_gates(dev, H, B, T, stride, off):
    """Input projections scaled by 30: gates deep in the flat parts of sigmoid and tanh (exp overflows to inf / underflows to 0 there).
    Bar: twice the distance of the same recurrence evaluated in float32 on the CPU from the float64 one, plus 1e-6.
    Measured on an MI355X, distance to float64 of the device / of the CPU float32 recurrence: small kernel (H = 64, B = 3, T = 40)
    h 2.9e-7 / 2.3e-7 and 2.3e-7 / 2.6e-7, c 3.7e-7 / 2.1e-7 and 5.9e-7 / 5.9e-7; distributed kernel (H = 256, T = 33) h 2.1e-7 /
    2.5e-7 and 1.9e-7 / 1.9e-7, c 2.3e-7 / 2.3e-7 and 2.8e-7 / 2.4e-7 (forward and reverse); max|c| 3.7 .. 4.8."""
    for reverse in (0, 1):
        xproj, whh, h0, c0 = _lstm_inputs(B, T, H, 3000 + H + reverse, scale=30.0)
        out, hn, cn = _lstm_device(dev, xproj, whh, h0, c0, reverse, stride, off)
        r64, c64 = _lstm_ref(xproj, whh, h0, c0, reverse, torch.float64)
        r32, c32 = _lstm_ref(xproj, whh, h0, c0, reverse, torch.float32)
        eh, eh32 = _linf(out, r64), _linf(r32, r64)
        ec, ec32, cmax = _linf(cn, c64), _linf(c32, c64), float(c64.abs().max())
        msg = ('saturated lstm H=%d reverse=%d: |h - h64| device %.3e, CPU fp32 %.3e;  |c - c64| device %.3e, CPU fp32 %.3e, max|c| %.2f'
               % (H, reverse, eh, eh32, ec, ec32, cmax))
        print(msg)
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(cn).all()), msg
        assert float(out.abs().max()) <= 1.0, msg
        assert torch.equal(hn, out[:, 0 if reverse else T - 1]), msg
        assert eh <= 2.0 * eh32 + 1e-6, msg
        assert ec <= 2.0 * ec32 + 1e-6 * max(1.0, cmax), msg


@pytest.mark.parametrize('H,B,ws,stride,off', [(128, 1, True, 128, 0), (256, 2, True, 256, 0), (256, 1, False, 256, 0), (16, 2, False, 20, 8)],
                         ids=['H=128', 'H=256 B=2', 'H=256 without workspace', 'out_off + H > out_stride'])
def test_lstm_refusals_launch_nothing(dev, H, B, ws, stride, off):
    from animateportrait_amd import ops, _capi
    lib = _capi.lib()
    T = 3
    xproj, whh, h0, c0 = (t.to(dev) for t in _lstm_inputs(B, T, H, 4000 + H))
    obuf, o = _window(B * T * (stride + off + H), dev)        # roomy enough for any reading of the refused sizes
    hbuf, hn = _window(B * H, dev)
    cbuf, cn = _window(B * H, dev)
    wsbuf = _lstm_workspace(H, dev)[0] if ws else None
    rc = lib.ap_lstm_recurrence(ops._ptr(xproj), ops._ptr(whh), ops._ptr(h0), ops._ptr(c0), ops._ptr(o), ops._ptr(hn), ops._ptr(cn), B, T, H, 0,
                                stride, off, ctypes.c_void_p(wsbuf.data_ptr()) if ws else None, ops._stream())
    torch.cuda.synchronize()
    assert rc != 0 and lib.ap_last_error()
    assert _untouched(obuf) and _untouched(hbuf) and _untouched(cbuf)


# ================================================================================================ 2. TPS solve and warp
#
# The spline system is ill-conditioned, so the bar is the one of test_tps_batched_vs_oracle: the device may be twice as far from the
# float64 oracle as the oracle's own float32 CPU evaluation, plus 1e-3.  That only means something while the float32 evaluation is
# itself close, so every seed below was chosen, on the CPU, such that the float32 oracle's flow is within 0.05 px of the float64 one
# (asserted again in _tps_check).  That distance depends on the host's LAPACK; on two hosts, flow px / warped value: non-square
# 1.2e-3 .. 1.3e-3 / 9.8e-4, three points 1.1e-6 .. 1.8e-6 / 1.8e-6 .. 2.1e-6, n = 123 3.5e-3 .. 5.0e-3 / 3.0e-3 .. 3.2e-3, clamping
# 2.7e-4 .. 3.5e-4 / 2.2e-4 .. 2.9e-4 (seeds 1 .. 8 of every case stay below 6e-3 px).  The MI355X measured 2.0e-3 / 1.9e-3,
# 7.5e-7 / 1.6e-6, 4.5e-3 / 3.1e-3 and 4.2e-4 / 3.4e-4.

def _tps_device(dev, img, src, dst):
    """ap_tps_solve + ap_tps_warp through the C ABI on windows: (warped NHWC, flow, coef) on the CPU.  The image sits inside a larger
    buffer as well, so a sample position that escaped its clamp would read sentinel, not a neighbour's memory."""
    from animateportrait_amd import ops, _capi
    lib = _capi.lib()
    b, h, w, c = img.shape
    n = src.shape[1]
    what = 'tps B=%d n=%d %dx%dx%d' % (b, n, h, w, c)
    ibuf, nchw = _window(b * c * h * w, dev, pad=4 * h * w)
    nchw.view(b, c, h, w).copy_(img.permute(0, 3, 1, 2))
    sd, dd = src.contiguous().to(dev), dst.contiguous().to(dev)
    kbuf, coef = _window(b * (n + 3) * 2, dev)
    obuf, out = _window(b * c * h * w, dev)
    fbuf, flow = _window(b * h * w * 2, dev)
    status = torch.zeros((), dtype=torch.int32, device=dev)
    _capi.check(lib.ap_tps_solve(ops._ptr(sd), ops._ptr(dd), b, n, ops._ptr(coef), ctypes.c_void_p(status.data_ptr()), ops._stream()), what)
    _capi.check(lib.ap_tps_warp(ops._ptr(nchw), ops._ptr(dd), ops._ptr(coef), b, n, c, h, w, ops._ptr(out), ops._ptr(flow), ops._stream()), what)
    torch.cuda.synchronize()
    assert int(status) == 0, what + ': reported singular'
    for buf, k in ((kbuf, b * (n + 3) * 2), (obuf, b * c * h * w), (fbuf, b * h * w * 2)):
        _assert_band(buf, k, what)
    return out.view(b, c, h, w).permute(0, 2, 3, 1).cpu(), flow.view(b, h, w, 2).cpu(), coef.view(b, n + 3, 2).cpu()


def _tps_check(tag, dev, img, src, dst):
    """Device against the float64 oracle at the bar above; returns what the callers look at further."""
    from oracle import tps as ot
    w32, f32 = ot.sparse_image_warp(img, src, dst)
    w64, f64 = ot.sparse_image_warp(img.double(), src.double(), dst.double())
    e32f, e32w = _linf(f32, f64), _linf(w32, w64)
    assert e32f < 0.05, (tag, 'seed: the float32 oracle itself is %.3e px from float64' % e32f)
    got_w, got_f, coef = _tps_device(dev, img, src, dst)
    ef, ew = _linf(got_f, f64), _linf(got_w, w64)
    print('tps %s: flow device %.3e (fp32 oracle %.3e)  warp device %.3e (fp32 oracle %.3e)' % (tag, ef, e32f, ew, e32w))
    assert ef <= 2.0 * e32f + 1e-3, (tag, ef, e32f)
    assert ew <= 2.0 * e32w + 1e-3, (tag, ew, e32w)
    return got_f, coef, f64, 2.0 * e32f + 1e-3


def _tps_nonsquare(seed=3):
    g = torch.Generator().manual_seed(seed)
    H, W = 40, 72
    src = torch.rand(3, 20, 2, generator=g) * torch.tensor([H - 8.0, W - 8.0]) + 4.0     # different points per sample
    dst = src + torch.randn(3, 20, 2, generator=g)
    return torch.rand(3, H, W, 3, generator=g), src, dst


def _tps_three_points(seed=2):
    g = torch.Generator().manual_seed(seed)
    dst = torch.tensor([[6.0, 8.0], [26.0, 14.0], [12.0, 40.0]]) + torch.rand(2, 3, 2, generator=g) * 4.0       # a proper triangle
    src = dst + torch.randn(2, 3, 2, generator=g) * 2.0
    return torch.rand(2, 32, 48, 1, generator=g), src, dst


def _tps_largest(seed=1):
    """123 control points on 64 x 64: 123 of the 132 cells of a 5 px grid, each moved by at most 1 px -- at least 3 px apart."""
    g = torch.Generator().manual_seed(seed)
    cells = torch.randperm(132, generator=g)[:123]
    dst = torch.stack([4.5 + 5.0 * (cells // 12), 4.5 + 5.0 * (cells % 12)], -1).float() + (torch.rand(123, 2, generator=g) * 2 - 1)
    src = dst + torch.randn(123, 2, generator=g)
    return torch.rand(1, 64, 64, 1, generator=g), src[None], dst[None]


def _tps_clamping(seed=4):
    """Displacements of 0.75 of the image size: four samples shifted off one side each, a fifth magnified four times about the
    centre (flow = -3 (q - centre): 0.75 of the size a quarter of the size away from it), which leaves on every side at once."""
    g = torch.Generator().manual_seed(seed)
    H, W, n = 40, 72, 8
    size = torch.tensor([float(H), float(W)])
    dst = torch.rand(5, n, 2, generator=g) * (size - 8.0) + 4.0
    shift = torch.tensor([[0.75 * H, 0.0], [-0.75 * H, 0.0], [0.0, 0.75 * W], [0.0, -0.75 * W]])
    src = dst.clone()
    src[:4] = dst[:4] - shift[:, None, :] + torch.randn(4, n, 2, generator=g) * 0.5
    centre = (size - 1.0) / 2
    src[4] = centre + 4.0 * (dst[4] - centre)
    return torch.rand(5, H, W, 2, generator=g), src, dst


def test_tps_non_square_image(dev):
    """B = 3, 40 x 72 x 3, 20 points per sample: pix / W, pix % W and the two different extents of the warp kernel."""
    _tps_check('non-square', dev, *_tps_nonsquare())


def test_tps_three_points_is_the_affine_map(dev):
    """n = 3, the smallest served system: the spline through three non-collinear displacements is the affine map through them, its
    w rows are zero up to rounding."""
    img, src, dst = _tps_three_points()
    flow, coef, f64, bar = _tps_check('three points', dev, img, src, dst)
    b, h, w, _ = img.shape
    ones = torch.ones(b, 3, 1, dtype=torch.float64)
    v = torch.linalg.solve(torch.cat([dst.double(), ones], 2), (dst - src).double())                 # [c 1] v = f
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing='ij')
    q = torch.stack([yy, xx, torch.ones_like(yy)], -1).reshape(1, h * w, 3).expand(b, -1, -1)
    affine = torch.bmm(q, v).reshape(b, h, w, 2)
    assert _linf(f64, affine) < 1e-9                       # the float64 oracle agrees that this is what the spline is
    assert _linf(flow, affine) <= bar, _linf(flow, affine)
    # "zero up to rounding": three w terms at the largest phi any pixel of this image can see stay inside the flow's bar
    r2 = float(h * h + w * w)
    phi_max = 0.5 * r2 * math.log(r2)
    wmax = float(coef[:, :3].abs().max())
    print('tps three points: max|w| = %.3e, its largest possible share of the flow %.3e px' % (wmax, 3 * wmax * phi_max))
    assert 3 * wmax * phi_max <= bar, (wmax, phi_max, bar)


def test_tps_largest_served_system(dev):
    """n = 123: 126 unknowns, 65 496 bytes of the 64 KiB of LDS."""
    img, src, dst = _tps_largest()
    d = torch.cdist(dst[0].double(), dst[0].double()) + 1e3 * torch.eye(123, dtype=torch.float64)
    assert float(d.min()) >= 3.0
    _tps_check('n=123', dev, img, src, dst)


def test_tps_sample_positions_far_outside_the_image(dev):
    """The [0, size - 2] clamp of the floor and the [0, 1] clamp of alpha, on a non-square image, compared at every pixel."""
    img, src, dst = _tps_clamping()
    _, _, f64, _ = _tps_check('clamping', dev, img, src, dst)
    b, h, w, _ = img.shape
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing='ij')
    sy, sx = yy - f64[..., 0], xx - f64[..., 1]
    shares = [float(m.double().mean()) for m in (sy < 0, sy > h - 1, sx < 0, sx > w - 1)]
    print('tps clamping: share of sample positions above / below / left / right of the image: %s' % shares)
    assert min(shares) > 0.1, shares


def test_tps_served_range_is_the_advertised_one(dev):
    """ap_tps_solve and ap_tps_warp take n = 3 .. 123 (the tests above run both ends); 2, 124 and 125 are refused before a launch,
    and the error text names the range that is served."""
    from animateportrait_amd import ops, _capi
    lib = _capi.lib()
    g = torch.Generator().manual_seed(7)
    for n in (2, 124, 125):
        dst = (torch.rand(1, n, 2, generator=g) * 56 + 4).to(dev)
        src = dst + 1.0
        img = torch.rand(1, 1, 64, 64, generator=g).to(dev)
        kbuf, coef = _window((n + 3) * 2, dev)
        obuf, out = _window(64 * 64, dev)
        status = torch.zeros((), dtype=torch.int32, device=dev)
        rc = lib.ap_tps_solve(ops._ptr(src), ops._ptr(dst), 1, n, ops._ptr(coef), ctypes.c_void_p(status.data_ptr()), ops._stream())
        assert rc != 0 and b'3..123' in lib.ap_last_error(), (n, rc, lib.ap_last_error())
        rc = lib.ap_tps_warp(ops._ptr(img), ops._ptr(dst), ops._ptr(coef), 1, n, 1, 64, 64, ops._ptr(out), None, ops._stream())
        assert rc != 0, (n, rc)
        torch.cuda.synchronize()
        assert _untouched(kbuf) and _untouched(obuf) and int(status) == 0, n


# ================================================================================================ 3. Adam

LR, BETAS, EPS, STEPS = 5e-5, (0.5, 0.999), 1e-8, 12
ADAM_BLOCKS = 8192 * 256          # elements the capped grid of adam_kernel covers in its first trip


def _adam_ref(p, grads, m, v, step0):
    """torch.optim.Adam's recurrence (no weight decay, no amsgrad) in float64."""
    p, m, v = p.double().clone(), m.double().clone(), v.double().clone()
    for k, g in enumerate(grads):
        t, g = step0 + k, g.double()
        m = BETAS[0] * m + (1 - BETAS[0]) * g
        v = BETAS[1] * v + (1 - BETAS[1]) * g * g
        denom = v.sqrt() / math.sqrt(1 - BETAS[1] ** t) + EPS
        p = p - (LR / (1 - BETAS[0] ** t)) * (m / denom)
    return p, m, v


def _adam_p_bar(p64):
    """One rounding of a value of the size of max|p| per step, plus a 1e-5 share of a step of size lr per step for the fp32 evaluation
    of the step itself (the moments' bar is 1e-6 of their maxima)."""
    return STEPS * 2.0 ** -24 * float(p64.abs().max()) + STEPS * LR * 1e-5


@pytest.mark.parametrize('n,step0', [(1, 1), (257, 1), (ADAM_BLOCKS + 77, 1), (257, 1000)],
                         ids=['n=1', 'n=257', 'n=8192*256+77', 'n=257 from step 1000'])
def test_adam_step_c_abi(dev, n, step0):
    """ap_adam_step on separate p / g / m / v: one element, one block and a bit, the grid-stride walk past the 8192-block cap; twelve
    steps with fresh gradients (exact zeros among them), both moments compared; bias correction at steps 1000 .. 1011.
    (The bar on v is what made ap_adam_step take its hyper-parameters as doubles: with float betas the kernel formed 1.f - 0.999f,
    1.3e-5 off 0.001, and v was 1.3e-5 of its maximum away from the recurrence on the first three cases.)"""
    from animateportrait_amd import ops, _capi
    lib = _capi.lib()
    gen = torch.Generator().manual_seed(900 + n % 1000 + step0)
    p0 = torch.randn(n, generator=gen)
    m0 = torch.randn(n, generator=gen) * 0.1 if step0 > 1 else torch.zeros(n)
    v0 = torch.rand(n, generator=gen) * 0.5 + 0.01 if step0 > 1 else torch.zeros(n)
    grads = []
    for _ in range(STEPS):
        g = torch.randn(n, generator=gen)
        g[torch.rand(n, generator=gen) < 0.1] = 0.0
        grads.append(g)
    if n > 1:
        assert any(bool((g == 0).any()) for g in grads)
    else:
        grads[3].zero_()
    bufs = [_window(n, dev) for _ in range(4)]
    (pb, p), (gb, g), (mb, m), (vb, v) = bufs
    p.copy_(p0)
    m.copy_(m0)
    v.copy_(v0)
    for k in range(STEPS):
        g.copy_(grads[k])
        _capi.check(lib.ap_adam_step(ops._ptr(p), ops._ptr(g), ops._ptr(m), ops._ptr(v), n, LR, BETAS[0], BETAS[1], EPS, step0 + k,
                                     ops._stream()), 'adam_step')
    torch.cuda.synchronize()
    for buf, _ in bufs:
        _assert_band(buf, n, 'adam n=%d' % n)
    p64, m64, v64 = _adam_ref(p0, grads, m0, v0, step0)
    bar_p, bar_m, bar_v = _adam_p_bar(p64), 1e-6 * float(m64.abs().max()), 1e-6 * float(v64.abs().max())
    spans = [('all', slice(0, n))]
    if n > ADAM_BLOCKS:
        spans += [('the last 77', slice(n - 77, n)), ('the first element of the second trip', slice(ADAM_BLOCKS, ADAM_BLOCKS + 1))]
    for name, sl in spans:
        ep, em, ev = _linf(p[sl], p64[sl]), _linf(m[sl], m64[sl]), _linf(v[sl], v64[sl])
        print('adam n=%d step0=%d %s: p %.3e (bar %.3e)  m %.3e (bar %.3e)  v %.3e (bar %.3e)' % (n, step0, name, ep, bar_p, em, bar_m, ev, bar_v))
        assert ep <= bar_p, (name, ep, bar_p)
        assert em <= bar_m, (name, em, bar_m)
        assert ev <= bar_v, (name, ev, bar_v)


def test_flat_adam_updates_its_parameters_in_place(dev):
    """FlatAdam over three parameters of unequal sizes: they are views of the flat buffer, the step moves them in place, and the
    result is torch.optim.Adam's in float64 on the same gradients."""
    from animateportrait_amd.optim import FlatAdam
    gen = torch.Generator().manual_seed(77)
    shapes = [(3, 5), (7,), (2, 3, 4)]
    init = [torch.randn(s, generator=gen) for s in shapes]
    params = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
    ref = [torch.nn.Parameter(t.double().clone()) for t in init]
    opt = FlatAdam(params, lr=LR, betas=BETAS, eps=EPS)
    ropt = torch.optim.Adam(ref, lr=LR, betas=BETAS, eps=EPS)
    off = 0
    for p in params:
        assert p.data_ptr() == opt.flat.data_ptr() + 4 * off and p.grad.data_ptr() == opt.flat_grad.data_ptr() + 4 * off
        off += p.numel()
    assert off == opt.flat.numel() == 46
    for _ in range(STEPS):
        opt.zero_grad()
        ropt.zero_grad()
        for p, r in zip(params, ref):
            g = torch.randn(p.shape, generator=gen)
            p.grad.copy_(g)
            r.grad = g.double()
        opt.step()
        ropt.step()
    torch.cuda.synchronize()
    bar = _adam_p_bar(torch.cat([r.detach().reshape(-1) for r in ref]))
    off = 0
    for p, r, t in zip(params, ref, init):
        assert p.data_ptr() == opt.flat.data_ptr() + 4 * off                         # still the same storage
        assert torch.equal(opt.flat[off:off + p.numel()], p.detach().reshape(-1))
        assert _linf(p, t) > 0.5 * STEPS * LR * 0.1                                  # and it moved
        assert _linf(p, r) <= bar, (tuple(p.shape), _linf(p, r), bar)
        off += p.numel()


# ================================================================================================ 4. image helpers

@pytest.mark.parametrize('shape', [(2, 3, 1, 9), (1, 2, 9, 1), (1, 1, 1, 1), (2, 3, 37, 53)], ids=lambda s: 'x'.join(map(str, s)))
def test_resize_bilinear_extents_of_one(dev, shape):
    """ap_resize_bilinear from and to extents of 1 (y1 == y0, a scale below one sample) against F.interpolate in float64."""
    from animateportrait_amd import ops, _capi
    lib = _capi.lib()
    n, c, h, w = shape
    x = torch.randn(shape, generator=torch.Generator().manual_seed(31 + h * w))
    xd = x.to(dev)
    for oh, ow in ((1, 1), (1, 17), (5, 1), (11, 16), (74, 106)):
        ybuf, y = _window(n * c * oh * ow, dev)
        _capi.check(lib.ap_resize_bilinear(ops._ptr(xd), n * c, h, w, oh, ow, ops._ptr(y), ops._stream()), 'resize_bilinear')
        torch.cuda.synchronize()
        _assert_band(ybuf, n * c * oh * ow, 'resize %s -> %s' % (shape, (oh, ow)))
        ref = F.interpolate(x.double(), size=(oh, ow), mode='bilinear', align_corners=False)
        err = _linf(y.view(n, c, oh, ow), ref)
        assert err < 1e-5, (shape, (oh, ow), err)


def _sample_grid(n, gen):
    """(n, 11, 11, 2): every pair of -1, 0, 1, +-1 +- 2^-20 and +-1e6 (81 points, all exact in fp32), then 40 random points of which
    some fall outside."""
    s = 2.0 ** -20
    sp = torch.tensor([-1.0, 0.0, 1.0, -1.0 - s, -1.0 + s, 1.0 - s, 1.0 + s, -1e6, 1e6], dtype=torch.float32)
    assert sp.double().tolist() == [-1.0, 0.0, 1.0, -1.0 - s, -1.0 + s, 1.0 - s, 1.0 + s, -1e6, 1e6]
    gx, gy = torch.meshgrid(sp, sp, indexing='ij')
    special = torch.stack([gx.reshape(-1), gy.reshape(-1)], -1)[None].expand(n, -1, -1)
    rnd = torch.rand(n, 40, 2, generator=gen) * 2.6 - 1.3
    return torch.cat([special, rnd], 1).reshape(n, 11, 11, 2).contiguous()


@pytest.mark.parametrize('align_corners', [False, True])
@pytest.mark.parametrize('shape', [(2, 3, 1, 6), (1, 2, 6, 1), (2, 3, 5, 7)], ids=lambda s: 'x'.join(map(str, s)))
def test_grid_sample_borders_and_extents_of_one(dev, shape, align_corners):
    """ap_grid_sample with grid points exactly on the border, one fp32 step to either side of it and far outside (the -2 .. W + 1
    clamp), on planes with H = 1 or W = 1 (W - 1 == 0 under align_corners) against F.grid_sample in float64."""
    from animateportrait_amd import ops, _capi
    lib = _capi.lib()
    n, c, h, w = shape
    gen = torch.Generator().manual_seed(41 + h * w)
    x = torch.randn(shape, generator=gen)
    grid = _sample_grid(n, gen)
    xd, gd = x.to(dev), grid.to(dev)
    ybuf, y = _window(n * c * 121, dev)
    _capi.check(lib.ap_grid_sample(ops._ptr(xd), ops._ptr(gd), n, c, h, w, 11, 11, int(align_corners), ops._ptr(y), ops._stream()),
                'grid_sample')
    torch.cuda.synchronize()
    _assert_band(ybuf, n * c * 121, 'grid_sample %s' % (shape,))
    ref = F.grid_sample(x.double(), grid.double(), mode='bilinear', padding_mode='zeros', align_corners=align_corners)
    err = _linf(y.view(n, c, 11, 11), ref)
    assert err < 2e-5, (shape, align_corners, err)


@pytest.mark.parametrize('shape', [(1, 4, 1, 1), (2, 12, 3, 5), (3, 8, 7, 2)], ids=lambda s: 'x'.join(map(str, s)))
def test_pixel_shuffle2_odd_planes(dev, shape):
    """ap_pixel_shuffle2 (one 8-byte store per output pixel pair) on planes of odd size and of one pixel: the bits of F.pixel_shuffle."""
    from animateportrait_amd import ops, _capi
    lib = _capi.lib()
    n, c4, h, w = shape
    x = torch.randn(shape, generator=torch.Generator().manual_seed(51 + h * w))
    xd = x.to(dev)
    ybuf, y = _window(n * c4 * h * w, dev)
    _capi.check(lib.ap_pixel_shuffle2(ops._ptr(xd), n, c4 // 4, h, w, ops._ptr(y), ops._stream()), 'pixel_shuffle2')
    torch.cuda.synchronize()
    _assert_band(ybuf, n * c4 * h * w, 'pixel_shuffle2 %s' % (shape,))
    assert torch.equal(y.view(n, c4 // 4, 2 * h, 2 * w).cpu(), F.pixel_shuffle(x, 2))
