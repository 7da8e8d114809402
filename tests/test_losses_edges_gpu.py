"""GPU (-m gpu): the loss-side kernels of csrc/losses.hip and csrc/landmark_masks.hip at three channels and at their
contract edges -- compositing with a C-channel background and an appended mask channel, crop + resize on H != W frames with overhanging / short / oversized /
one-pixel windows and the three-channel maps, the rasterisers and flow_post off their one production shape, the L1
backward's zero branch, ap_axpy, the C-side refusals, and sentinel-padded outputs behind every kernel.

Every reference is float64 (or the oracle's own float32 / numpy form where the claim is bit equality) on the CPU, built
from oracle/aux_glue.py, oracle/losses.py, oracle/cv_raster.py and torch.nn.functional; the HIP path is never its own
reference.  Bars are the project's (test_losses_gpu.py) or derived where stated; every test prints its worst figure."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import linf

pytestmark = pytest.mark.gpu

AP_ERR_INVALID = -1
SENTINEL = 0x7FA5A5A5                 # a NaN bit pattern no kernel here produces
PAD = 4096                            # sentinel elements behind every padded output


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


def _padded(dev, numel, pad=PAD):
    """(whole buffer as int32, its first ``numel`` elements as a float32 view): a sentinel-filled buffer whose front is the
    kernel's output."""
    buf = torch.full((numel + pad,), SENTINEL, dtype=torch.int32, device=dev)
    return buf, buf.view(torch.float32)[:numel]


def _tail_intact(buf, numel):
    torch.cuda.synchronize()
    return bool((buf[numel:] == SENTINEL).all())


def _front_written(buf, numel):
    return not bool((buf[:numel] == SENTINEL).any())


def _api():
    from animateportrait_amd import _capi, ops
    return _capi.lib(), ops._ptr, ops._stream


# ------------------------------------------------------------------------------------------------------- compositing
COMP_SHAPES = [(1, 1, 1, 1), (3, 3, 5, 7), (2, 4, 17, 33), (2, 3, 16, 16)]


def _comp_inputs(n, c, h, w):
    g = torch.Generator().manual_seed(7000 + 100 * c + h)
    a = torch.rand(n, c, h, w, generator=g) * 2 - 1
    s1 = torch.rand(n, 1, h, w, generator=g) * 2 - 1
    sc = torch.rand(n, c, h, w, generator=g) * 2 - 1           # distinct planes: a wrong channel index changes the result
    m = torch.rand(n, 1, h, w, generator=g)
    if h >= 3:
        m[:, :, 0] = 0.0
        m[:, :, 1] = 1.0
        masks = [m]
    else:                                                       # the one-pixel plane: exact 0, exact 1 and a fraction in turn
        masks = [torch.zeros_like(m), torch.ones_like(m), m]
    return g, a, s1, sc, masks


def _comp_cases(losses, ol, s1, sc):
    """(name, HIP function of (x, mask, to-device), oracle function of (x, mask, cast), appended channels)."""
    cases = [('masked%d' % t, (lambda x, m, to, t=t: losses.masked(x, m, t)), (lambda x, m, cast, t=t: ol.masked(x, m, t)),
              int(t >= 2)) for t in range(4)]
    cases.append(('fore', lambda x, m, to: losses.fore_composite(x, m), lambda x, m, cast: ol.fore_composite(x, m), 0))
    for name, s in (('blend_cs1', s1), ('blend_csC', sc)):
        cases.append((name, (lambda x, m, to, s=s: losses.bg_blend(x, to(s), m)),
                      (lambda x, m, cast, s=s: ol.bg_blend(x, cast(s), m)), 0))
    return cases


@pytest.mark.parametrize('shape', COMP_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_compositing_every_mode_vs_oracle(dev, shape):
    """masked() 0-3, fore_composite and bg_blend with a 1-channel and a C-channel background: forward bit-equal to the oracle
    in float32 and within 1e-6 of it in float64; backward within 1e-6 of float64 autograd; for the appended-mask types the
    upstream gradient's extra channel (large) leaves x.grad untouched."""
    from animateportrait_amd import losses
    from oracle import losses as ol
    n, c, h, w = shape
    g, a, s1, sc, masks = _comp_inputs(*shape)
    worst_f = worst_b = 0.0
    for m in masks:
        ad, md = a.to(dev), m.to(dev)
        for name, hip, ref, app in _comp_cases(losses, ol, s1, sc):
            x = ad.clone().requires_grad_(True)
            y = hip(x, md, lambda t: t.to(dev))
            assert y.shape == (n, c + app, h, w), name
            assert torch.equal(y.detach().cpu(), ref(a, m, lambda t: t)), name
            xr = a.double().requires_grad_(True)
            yr = ref(xr, m.double(), lambda t: t.double())
            worst_f = max(worst_f, linf(y, yr))
            assert linf(y, yr) < 1e-6, name
            go = torch.randn(y.shape, generator=g)
            if app:
                go[:, -1] = torch.randn(n, h, w, generator=g) * 1e4
            y.backward(go.to(dev))
            yr.backward(go.double())
            worst_b = max(worst_b, linf(x.grad, xr.grad))
            assert linf(x.grad, xr.grad) < 1e-6, name
            if app:
                go2 = go.clone()
                go2[:, -1] = torch.randn(n, h, w, generator=g) * 1e4 + 3.0
                x2 = ad.clone().requires_grad_(True)
                hip(x2, md, lambda t: t.to(dev)).backward(go2.to(dev))
                assert torch.equal(x.grad, x2.grad), name
    print('compositing %s: forward L-inf vs fp64 %.3e (bar 1e-6), backward %.3e (bar 1e-6)' % (shape, worst_f, worst_b))


def test_cartoon_blend_equals_the_oracle(dev):
    """The cartoon model's last step, fake_B = bg_blend(fake_B_fore, fakeB_static, mask1) with three-channel frames and the
    elliptic matte of test_cartoon_streaming_model: bit-equal to oracle.losses.bg_blend on the CPU (the independent
    counterpart of the model test's own-output comparison)."""
    from animateportrait_amd import losses
    from oracle import losses as ol
    g = torch.Generator().manual_seed(247)
    fore = torch.rand(1, 3, 256, 256, generator=g) * 2 - 1
    static = torch.rand(1, 3, 256, 256, generator=g) * 2 - 1
    yy, xx = torch.meshgrid(torch.arange(256.), torch.arange(256.), indexing='ij')
    matte = ((((yy - 128) / 90) ** 2 + ((xx - 120) / 70) ** 2) < 1).float().view(1, 1, 256, 256)
    mask = F.avg_pool2d(matte, 5, 1, 2)                         # soft rim, exact 0 outside and exact 1 inside
    assert float(mask.min()) == 0.0 and float(mask.max()) == 1.0 and bool(((mask > 0) & (mask < 1)).any())
    got = losses.bg_blend(fore.to(dev), static.to(dev), mask.to(dev)).cpu()
    assert torch.equal(got, ol.bg_blend(fore, static, mask))
    assert linf(got, ol.bg_blend(fore.double(), static.double(), mask.double())) < 1e-6


# ------------------------------------------------------------------------------------------------------- crop + resize
CROP_H, CROP_W = 40, 56
WINDOWS = [[5, 29, 3, 27],            # inside
           [-6, 20, -4, 22],          # left / top overhang
           [40, 64, 25, 49],          # right / bottom overhang
           [10, 40, 12, 30],          # shorter than wide: rows past y2 are ones
           [30, 70, -5, 20],          # short and overhanging
           [-3, 60, -2, 43],          # larger than the frame
           [7, 8, 9, 10]]             # size 1
CHANNEL_MAPS = [(1, (0, 0, 0)), (3, (2, 1, 0)), (3, (0, 1, 2)), (3, (1,)), (3, (0, 2)), (3, (1, 1, 2, 0))]
RESIZES = [(1, (37, 29)), (1, (7, 5)), (0, (13, 11)), (0, (1, 9)), (0, (9, 1))]       # (mode, size); 1 = bicubic


def _crop_frames(c, n=len(WINDOWS)):
    return torch.rand(n, c, CROP_H, CROP_W, generator=torch.Generator().manual_seed(560 + c)) * 2 - 1


def _crop_reference(x64, wins, channels, size, mode):
    """oa.crop_box per sample, channel selection by indexing, F.interpolate, * 0.5 + 0.5 -- float64, differentiable."""
    from oracle import aux_glue as oa
    outs = []
    for i in range(x64.shape[0]):
        box = oa.crop_box(x64[i:i + 1], wins[i])[:, list(channels)]
        if mode == 1:
            r = F.interpolate(box, size=size, mode='bicubic', align_corners=False)
        else:
            r = F.interpolate(box, size=size, mode='bilinear', align_corners=True)
        outs.append(r * 0.5 + 0.5)
    return torch.cat(outs, 0)


def _crop_check(dev, x, wins, channels, size, mode, go, fwd_bar, tag, go_dev=None, some_zero=True):
    """Forward and backward of one crop_resize call against the float64 reference; returns (forward, backward) errors, the
    backward one relative to max(1, |grad|max)."""
    from animateportrait_amd import losses
    n = x.shape[0]
    xd = x.to(dev).requires_grad_(True)
    y = losses.crop_resize(xd, losses.windows_to_device(wins, n, dev), channels, size, mode, 0.5, 0.5)
    assert y.shape == (n, len(channels)) + tuple(size), tag
    y.backward(go.to(dev) if go_dev is None else go_dev)
    xr = x.double().requires_grad_(True)
    yr = _crop_reference(xr, wins, channels, size, mode)
    yr.backward(go.double())
    ef = linf(y, yr)
    assert ef < fwd_bar, (tag, ef)
    scale = max(1.0, float(xr.grad.abs().max()))
    eb = linf(xd.grad, xr.grad) / scale
    assert eb < 1e-5, (tag, eb)
    zero = xr.grad == 0                                          # outside the window, channels absent from the map
    assert bool((xd.grad.cpu()[zero] == 0).all()), tag
    assert bool(zero.any()) or not some_zero, tag
    return ef, eb


@pytest.mark.parametrize('mode,size', RESIZES, ids=lambda v: str(v).replace(' ', ''))
@pytest.mark.parametrize('c,channels', CHANNEL_MAPS, ids=lambda v: str(v).replace(' ', ''))
def test_crop_resize_windows_maps_and_sizes(dev, c, channels, mode, size):
    """One batch of the seven windows (a different one per sample) on 40 x 56 frames, every channel map and output size:
    forward 1e-5, backward 1e-5 * max(1, |grad|max) against float64 autograd, and exactly 0.0 where that gradient is 0."""
    x = _crop_frames(c)
    go = torch.randn(len(WINDOWS), len(channels), *size, generator=torch.Generator().manual_seed(size[0] * 64 + size[1]))
    ef, eb = _crop_check(dev, x, torch.tensor(WINDOWS, dtype=torch.int32), channels, size, mode, go, 1e-5, (channels, mode, size))
    print('crop_resize C=%d map=%s mode=%d size=%s: forward %.3e (bar 1e-5), backward %.3e (bar 1e-5, relative)'
          % (c, channels, mode, size, ef, eb))


@pytest.mark.parametrize('c,channels', CHANNEL_MAPS, ids=lambda v: str(v).replace(' ', ''))
def test_crop_resize_identity_size(dev, c, channels):
    """Bicubic to the window's own size: every tap weight is exactly 0 or 1, so the forward bar is 1e-6."""
    x = _crop_frames(c)
    worst = (0.0, 0.0)
    for i, win in enumerate(WINDOWS):
        size = (win[1] - win[0],) * 2
        go = torch.randn(1, len(channels), *size, generator=torch.Generator().manual_seed(90 + i))
        e = _crop_check(dev, x[i:i + 1], torch.tensor([win], dtype=torch.int32), channels, size, 1, go, 1e-6, (channels, win),
                        some_zero=win[1] - win[0] < CROP_W)   # the oversized window with a full map reaches every pixel
        worst = (max(worst[0], e[0]), max(worst[1], e[1]))
    print('crop_resize identity C=%d map=%s: forward %.3e (bar 1e-6), backward %.3e (bar 1e-5, relative)' % ((c, channels) + worst))


def test_crop_resize_backward_takes_a_non_contiguous_gradient(dev):
    x = _crop_frames(3)
    n = len(WINDOWS)
    go1 = torch.randn(n, 1, 7, 5, generator=torch.Generator().manual_seed(75))
    go_dev = go1.to(dev).expand(n, 3, 7, 5)
    assert not go_dev.is_contiguous()
    _crop_check(dev, x, torch.tensor(WINDOWS, dtype=torch.int32), (2, 1, 0), (7, 5), 1, go1.expand(n, 3, 7, 5), 1e-5, 'expanded',
                go_dev=go_dev)


def test_crop_resize_refusals(dev):
    """Python side: empty / too-tall windows, a window tensor of the wrong dtype or device.  C side: OC = 5, a map entry >= C and
    mode 2 return the invalid-argument status and leave the output untouched."""
    from animateportrait_amd import losses
    with pytest.raises(ValueError):
        losses.windows_to_device([[10, 10, 0, 5]], 1, dev)          # empty window
    with pytest.raises(ValueError):
        losses.windows_to_device([[10, 20, 0, 50]], 1, dev)         # taller than the box: the reference's slice fails
    x = _crop_frames(3, 2).to(dev)
    win = torch.tensor(WINDOWS[:2], dtype=torch.int32)
    with pytest.raises(ValueError):
        losses.crop_resize(x, win.to(dev).long(), (0, 1, 2), (7, 5), 1)      # int64
    with pytest.raises(ValueError):
        losses.crop_resize(x, win, (0, 1, 2), (7, 5), 1)                     # int32, but on the CPU
    with pytest.raises(ValueError):
        losses.crop_resize(x, win.to(dev)[:1], (0, 1, 2), (7, 5), 1)         # one window for two samples
    lib, ptr, stream = _api()
    wd = win.to(dev)
    gout = torch.ones(2 * 5 * 7 * 5, device=dev)
    for oc, chmap, mode in ((5, 0, 1), (3, losses._chmap((0, 1, 3)), 1), (3, losses._chmap((0, 1, 2)), 2)):
        buf, out = _padded(dev, 2 * 5 * 7 * 5)
        assert lib.ap_crop_resize_fwd(ptr(x), ctypes.c_void_p(wd.data_ptr()), 2, 3, CROP_H, CROP_W, oc, chmap, 7, 5, mode, 0.5,
                                      0.5, ptr(out), stream()) == AP_ERR_INVALID
        gbuf, gx = _padded(dev, x.numel())
        assert lib.ap_crop_resize_bwd(ptr(gout), ctypes.c_void_p(wd.data_ptr()), 2, 3, CROP_H, CROP_W, oc, chmap, 7, 5, mode, 0.5,
                                      ptr(gx), stream()) == AP_ERR_INVALID
        torch.cuda.synchronize()
        assert bool((buf == SENTINEL).all()) and bool((gbuf == SENTINEL).all()), (oc, chmap, mode)


# ------------------------------------------------------------------------------------------------------- rasterisers
def _disc_points(h, w, g, n=3, p=12):
    lm = torch.rand(n, p, 2, generator=g) * torch.tensor([w + 20.0, h + 20.0]) - 10.0
    lm[0, :8] = torch.tensor([[0.0, 0.0], [w - 1.0, h - 1.0], [w - 1.0, 0.0], [0.0, h - 1.0],       # the four corners
                              [7.5, 8.5], [8.5, 7.5], [2.5, 3.5], [-0.5, 0.5]])                    # half-to-even rounding
    lm[1, :4] = torch.tensor([[-40.0, -40.0], [w + 10.0, 5.0], [12.0, h + 16.0], [-20.0, h / 2.0]])  # outside, partly visible at r >= 17
    lm[2, :] = torch.tensor([w // 4 + 0.5, h // 2 - 1.0])      # one disc alone: its rim shows even at radius 31
    lm[2, 0] = torch.tensor([-200.0, 500.0])
    return lm


@pytest.mark.parametrize('radius', [0, 5, 17, 31])
@pytest.mark.parametrize('hw', [(40, 72), (72, 40)], ids=lambda v: '%dx%d' % v)
def test_landmark_discs_off_square_every_radius(dev, hw, radius):
    from animateportrait_amd import losses
    from oracle import aux_glue as oa
    h, w = hw
    lm = _disc_points(h, w, torch.Generator().manual_seed(31 + radius))
    for lo, hi in ((-1.0, 1.0), (0.25, 3.0)):
        out = losses.landmark_discs(lm.to(dev), h, w, radius, lo, hi).cpu()
        assert out.shape == (3, 1, h, w)
        for i in range(3):
            want = oa.draw2(h, w, lm[i].numpy(), radius)
            if (lo, hi) != (-1.0, 1.0):
                want = torch.where(want > 0, torch.tensor(hi), torch.tensor(lo))
            assert torch.equal(out[i], want), (hw, radius, i, lo)
    assert float((out == 3.0).sum()) > 0


@pytest.mark.parametrize('p', [1, 4096])
def test_landmark_discs_point_count_limits(dev, p):
    """P = 1 and P = 4096 (the largest dynamic-LDS table): most of the 4096 points share six positions; the last one stands
    alone, so a table cut short loses its disc."""
    from animateportrait_amd import losses
    from oracle import aux_glue as oa
    h, w, radius = 40, 72, 5
    spots = torch.tensor([[3.0, 4.0], [70.5, 38.5], [30.0, 20.0], [-2.0, 39.0], [71.0, 0.0], [100.0, 100.0]])
    g = torch.Generator().manual_seed(4096)
    lm = spots[torch.randint(0, 6, (2, p), generator=g)]
    lm[0, p - 1] = torch.tensor([50.0, 10.0])
    lm[1, p - 1] = torch.tensor([15.0, 30.0])
    out = losses.landmark_discs(lm.to(dev), h, w, radius).cpu()
    for i in range(2):
        assert torch.equal(out[i], oa.draw2(h, w, lm[i].numpy(), radius)), (p, i)
    assert float(out[0, 0, 10, 50]) == 1.0 and float(out[1, 0, 30, 15]) == 1.0


def test_landmark_discs_refusals(dev):
    from animateportrait_amd import losses
    lib, ptr, stream = _api()
    with pytest.raises(RuntimeError):
        losses.landmark_discs(torch.zeros(1, 4, 2, device=dev), 40, 72, 32)
    with pytest.raises(RuntimeError):
        losses.landmark_discs(torch.zeros(1, 4097, 2, device=dev), 40, 72, 3)
    lm = torch.zeros(1, 4097, 2, device=dev)
    for p, radius in ((4, 32), (4097, 3), (4, -1)):
        buf, out = _padded(dev, 40 * 72)
        assert lib.ap_landmark_discs(ptr(lm), 1, p, 40, 72, radius, -1.0, 1.0, ptr(out), stream()) == AP_ERR_INVALID
        torch.cuda.synchronize()
        assert bool((buf == SENTINEL).all()), (p, radius)


def _kp_landmarks(s, p, num, den, g):
    """(2, p, 2) float32 landmarks whose scaled form covers the map and its surroundings; sample 0 holds coordinates that
    become exactly -1 only after the num / den scaling (the blanking rule, geomgm_ifw_fore_model.py:33-34)."""
    lm = torch.rand(2, p, 2, generator=g) * ((s + 8.0) * den / num) - 4.0 * den / num
    minus1 = float(np.float32(-den / num))
    assert minus1 != -1.0 and float((np.array([minus1], np.float32) * num / den)[0]) == -1.0
    inside = float(np.float32((s // 2) * den / num))
    lm[0, 0] = torch.tensor([minus1, inside])                   # x == -1 after scaling
    if p > 1:
        lm[0, 1] = torch.tensor([inside, minus1])               # y == -1 after scaling
        lm[0, 2] = torch.tensor([-1.0, inside])                 # -1 before scaling, not after: drawn (clipped)
    return lm


@pytest.mark.parametrize('num,den', [(7.0, 8.0), (5.0, 4.0)])
@pytest.mark.parametrize('p', [1, 5])
@pytest.mark.parametrize('s', [1, 17, 50])
def test_kp_to_map_small_sizes_bit_exact(dev, s, p, num, den):
    from animateportrait_amd import losses
    from oracle import aux_glue as oa
    lm = _kp_landmarks(s, p, num, den, torch.Generator().manual_seed(s * 10 + p))
    want = oa.kp_to_map_some((s, s), lm.numpy() * num / den)      # numpy float32, as the reference forms it
    got = losses.kp_to_map(lm.to(dev), s, num, den).cpu()
    assert got.shape == (2, p, s, s) and torch.equal(got, want)
    assert float(want[0, 0].sum()) == 0.0                         # blanked
    if p > 1 and s > 1:
        assert float(want[0, 1].sum()) == 0.0 and float(want[0, 2].sum()) > 0.0 and float(want.sum()) > 0.0


def test_kp_to_map_refuses_a_zero_denominator(dev):
    from animateportrait_amd import losses
    with pytest.raises(RuntimeError):
        losses.kp_to_map(torch.zeros(1, 2, 2, device=dev), 17, 7.0, 0.0)


@pytest.mark.parametrize('vc', [1, 2, 3, 5])
@pytest.mark.parametrize('s,os_', [(8, 8), (9, 20), (20, 9), (7, 1)])
def test_flow_post_ties_channel_counts_and_sizes(dev, s, os_, vc):
    """Visibility drawn from {0, 1, 2}: exact ties everywhere, resolved to the first index like torch.argmax, so not one mask
    pixel may flip.  Reference: the float64 form of oracle/aux_glue.py:98-103."""
    from animateportrait_amd import losses
    g = torch.Generator().manual_seed(1000 * s + 10 * os_ + vc)
    fo = torch.randn(3, 2, s, s, generator=g)
    vo = torch.randint(0, 3, (3, vc, s, s), generator=g).float()
    wf, rm = losses.flow_post(fo.to(dev), vo.to(dev), os_)
    vis = vo.argmax(dim=1, keepdim=True).float()
    mask = (vis < 2).double()
    if vc >= 3:
        assert 0.0 < float(mask.mean()) < 1.0
    flow = fo.double() * 20. * mask
    ref_f = F.interpolate(flow / 7 * 8, size=(os_, os_), mode='bilinear', align_corners=True)
    ref_m = F.interpolate(mask, size=(os_, os_), mode='bilinear', align_corners=True)
    assert wf.shape == (3, 2, os_, os_) and rm.shape == (3, 1, os_, os_)
    ef, em = linf(wf, ref_f) / max(1.0, float(ref_f.abs().max())), linf(rm, ref_m)
    print('flow_post S=%d OS=%d VC=%d: flow %.3e (bar 2e-5, relative), mask %.3e (bar 1e-6)' % (s, os_, vc, ef, em))
    assert int((rm.cpu().double() - ref_m).abs().gt(1e-6).sum()) == 0
    assert ef < 2e-5 and em < 1e-6


def _lip_lands(size, g):
    lands = torch.rand(3, 68, 2, generator=g) * (size * 1.6) - size * 0.3     # sample 0: on and off the frame, some segments wholly off
    lands[0, 48] = torch.tensor([-30.0, 5.0])
    lands[0, 49] = torch.tensor([-40.0, 20.0])                                # segment 48-49 lies off the frame
    lands[1, 48:68] = torch.tensor([16.3, 15.9])                              # all 20 lip points coincide
    lands[2, 48:68] = torch.rand(20, 2, generator=g) * 30 + size + 30.0       # every segment off the frame
    return lands


@pytest.mark.parametrize('thickness', [2, 16])
def test_lip_line_mask_odd_size_thickness_limits(dev, thickness):
    from animateportrait_amd import losses
    from animateportrait_amd.models.geomgm_ifw_fore_model import LIP_SEGMENTS
    from oracle import cv_raster as cr
    size = 33
    lands = _lip_lands(size, torch.Generator().manual_seed(33 + thickness))
    got = losses.lip_line_mask(lands.to(dev), LIP_SEGMENTS, size, thickness).cpu()
    assert got.shape == (3, 1, size, size)
    for i in range(3):
        want = cr.lip_line_mask(size, lands[i].double().numpy(), LIP_SEGMENTS, thickness)
        assert np.array_equal(got[i, 0].numpy(), want), (thickness, i, float(np.abs(got[i, 0].numpy() - want).sum()))
    assert float(got[0].sum()) > 0 and float(got[1].sum()) > 0 and float(got[2].sum()) == 0.0


def test_lip_line_mask_refusals(dev):
    from animateportrait_amd import losses
    lib, ptr, stream = _api()
    lands = torch.rand(2, 20, 2, generator=torch.Generator().manual_seed(2)).to(dev) * 33
    for th, segs in ((1, [(0, 1)]), (17, [(0, 1)]), (2, [(0, 20)]), (2, [(20, 0)]), (2, [(0, 1), (-1, 3)])):
        with pytest.raises(RuntimeError):
            losses.lip_line_mask(lands, segs, 33, th)
        a = (ctypes.c_int32 * len(segs))(*[s[0] for s in segs])
        b = (ctypes.c_int32 * len(segs))(*[s[1] for s in segs])
        buf, out = _padded(dev, 2 * 33 * 33)
        assert lib.ap_lip_line_mask(ptr(lands), 2, 20, a, b, len(segs), 33, th, ptr(out), stream()) == AP_ERR_INVALID
        torch.cuda.synchronize()
        assert bool((buf == SENTINEL).all()), (th, segs)


def _lip_oracle(size, lands, segs, thickness):
    from oracle import cv_raster as cr
    return np.stack([cr.lip_line_mask(size, l.double().numpy(), segs, thickness) for l in lands])


@pytest.mark.parametrize('nseg', [1, 32])
@pytest.mark.parametrize('thickness', [2, 16])
@pytest.mark.parametrize('size', [1, 16, 17])
def test_lip_line_mask_row_tile_edges(dev, size, thickness, nseg):
    """The kernel works on tiles of 16 rows: size 1 (one short tile), 16 (one full tile) and 17 (a full tile and a tile of a
    single row), with one segment and with 32, the limit.  Segment 0 runs from above the canvas to below it, so it crosses
    the tile boundary; the others are a random chain on and off the frame.  Bit-equal to oracle/cv_raster.py."""
    from animateportrait_amd import losses
    g = torch.Generator().manual_seed(1000 * size + 10 * thickness + nseg)
    lands = torch.rand(3, nseg + 1, 2, generator=g) * (size * 1.6) - size * 0.3
    lands[:, 0] = torch.tensor([0.2 * size, -2.5])
    lands[:, 1] = torch.tensor([0.8 * size, size + 1.5])
    lands[1, :2] = lands[1, :2].flip(1)                            # sample 1: the same crossing, x-major
    segs = [(i, i + 1) for i in range(nseg)]
    got = losses.lip_line_mask(lands.to(dev), segs, size, thickness).cpu()
    assert got.shape == (3, 1, size, size)
    want = _lip_oracle(size, lands, segs, thickness)
    assert np.array_equal(got[:, 0].numpy(), want), (size, thickness, nseg, float(np.abs(got[:, 0].numpy() - want).sum()))
    assert want[0, -1].sum() > 0 and want[0, 0].sum() > 0           # the crossing segment marks the first and the last row


def test_lip_line_mask_writes_every_element(dev):
    """The raw entry point into a buffer pre-filled with NaN (no memset precedes the kernel, which stores every element
    itself): bit-equal to the oracle, hence without a NaN, and nothing behind the output is touched."""
    from animateportrait_amd.models.geomgm_ifw_fore_model import LIP_SEGMENTS
    lib, ptr, stream = _api()
    size, n, th = 33, 2, 3
    lands = _lip_lands(size, torch.Generator().manual_seed(330))[:n]
    k = len(LIP_SEGMENTS)
    a = (ctypes.c_int32 * k)(*[s[0] for s in LIP_SEGMENTS])
    b = (ctypes.c_int32 * k)(*[s[1] for s in LIP_SEGMENTS])
    buf = torch.full((n * size * size + PAD,), float('nan'), device=dev)
    assert lib.ap_lip_line_mask(ptr(lands.to(dev)), n, 68, a, b, k, size, th, ptr(buf), stream()) == 0
    torch.cuda.synchronize()
    got = buf[:n * size * size].view(n, size, size).cpu()
    assert not bool(torch.isnan(got).any()) and bool(torch.isnan(buf[n * size * size:]).all())
    assert np.array_equal(got.numpy(), _lip_oracle(size, lands, LIP_SEGMENTS, th))
    assert float(got[0].sum()) > 0 and float((got == 0).sum()) > 0


@pytest.mark.parametrize('thickness', [2, 16])
def test_lip_line_mask_bounded_work_and_clamping(dev, thickness):
    """Size 33, three samples of a 20-segment ring plus one more segment.  Samples 0 and 2: the ring on and off the frame and
    a segment from -4096 to +4096 that crosses the canvas -- bit-equal to the oracle.  Sample 1: every end point at +-2^21 to
    the left of the canvas and one point NaN (which the coordinate clamp sends to the same side) -- all zero: a segment
    whose clamped box misses the canvas costs nothing and marks nothing."""
    from animateportrait_amd import losses
    size, far = 33, float(2 ** 21)
    g = torch.Generator().manual_seed(2100 + thickness)
    lands = torch.rand(3, 22, 2, generator=g) * (size * 1.6) - size * 0.3
    lands[0, 20:] = torch.tensor([[-4096.0, -4090.0], [4096.0, 4120.0]])
    lands[2, 20:] = torch.tensor([[4096.0, -4096.0], [-4096.0, 4111.0]])
    lands[1, :, 0] = -far
    lands[1, :, 1] = torch.where(torch.arange(22) % 3 == 0, -far, far)
    lands[1, 5] = torch.tensor([float('nan'), float('nan')])
    segs = [(i, (i + 1) % 20) for i in range(20)] + [(20, 21)]
    got = losses.lip_line_mask(lands.to(dev), segs, size, thickness).cpu()[:, 0].numpy()
    want = _lip_oracle(size, lands[[0, 2]], segs, thickness)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[1])
    assert want[0].sum() > 0 and want[1].sum() > 0
    assert float(np.abs(got[1]).sum()) == 0.0 and not np.isnan(got).any()


def test_landmark_discs_far_and_nan_points_contribute_nothing(dev):
    """40 x 72, radius 5: points at +-2^21 and one NaN among in-range ones.  The map equals oracle.aux_glue.draw2 of the
    in-range points alone (the far ones land on the coordinate clamp, far outside every canvas)."""
    from animateportrait_amd import losses
    from oracle import aux_glue as oa
    h, w, radius, far = 40, 72, 5, float(2 ** 21)
    lm = _disc_points(h, w, torch.Generator().manual_seed(2021))
    hostile = {1: [far, 20.0], 4: [30.0, -far], 6: [-far, far], 9: [float('nan'), 12.0], 10: [far, far]}
    keep = [i for i in range(12) if i not in hostile]
    full = lm.clone()
    for i, p in hostile.items():
        full[:, i] = torch.tensor(p)
    out = losses.landmark_discs(full.to(dev), h, w, radius).cpu()
    for i in range(3):
        want = oa.draw2(h, w, lm[i, keep].numpy(), radius)
        assert torch.equal(out[i], want), i
        assert float((want > 0).sum()) > 0
    assert not bool(torch.equal(out[0], oa.draw2(h, w, lm[0].numpy(), radius)))      # the replaced points did mark pixels


# ------------------------------------------------------------------------------------------------------- reductions, axpy
@pytest.mark.parametrize('n', [3001, 2048 * 256 + 1])
def test_l1_zero_branch_and_all_zero_weight_map(dev, n):
    """b == a on a third of the elements: gradient exactly 0 there, +-w/n elsewhere; a == b everywhere: loss exactly 0, gradient
    all zeros; an all-zero weight map: loss exactly 0.  n = 2048 * 256 + 1 puts one element into the second grid-stride pass."""
    from animateportrait_amd import losses
    g = torch.Generator().manual_seed(n)
    a = torch.randn(n, generator=g)
    b = torch.randn(n, generator=g)
    eq = torch.arange(n) % 3 == 1
    b[eq] = a[eq]
    b[n - 1] = a[n - 1] + 0.5                                       # the element of the second pass has a negative difference
    x, xb = a.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    y = losses.l1_loss(x, xb, 10.0)
    (y * 3.0).backward()
    xr = a.double().requires_grad_(True)
    yr = 10.0 * (xr - b.double()).abs().mean()
    (yr * 3.0).backward()
    y, yr = y.detach(), yr.detach()
    assert abs(float(y) - float(yr)) <= 2e-6 * abs(float(yr)) + 1e-7
    eg = linf(x.grad, xr.grad) / float(xr.grad.abs().max())
    print('l1 n=%d: loss rel. error %.3e (bar 2e-6), gradient %.3e (bar 1e-6, relative)' % (n, abs(float(y) - float(yr)) / float(yr), eg))
    assert eg <= 1e-6
    gx = x.grad.cpu()
    keep = ~eq
    keep[n - 1] = True
    assert bool((gx[~keep] == 0).all()) and bool((gx[keep] != 0).all())
    assert torch.equal(gx.sign(), (a.double() - b.double()).sign().float()) and float(gx[n - 1]) < 0
    assert torch.equal(x.grad, -xb.grad)
    x = a.to(dev).requires_grad_(True)
    y = losses.l1_loss(x, a.to(dev).clone(), 10.0)
    y.backward()
    assert float(y) == 0.0 and bool((x.grad == 0).all())
    x = a.to(dev).requires_grad_(True)
    y = losses.weighted_mean(x, torch.zeros(n, device=dev), 1.0, 50.0)
    y.backward()
    assert float(y) == 0.0 and bool((x.grad == 0).all())


def test_weight_map_gradient_is_refused(dev):
    from animateportrait_amd import losses
    a = torch.randn(300, generator=torch.Generator().manual_seed(1)).to(dev)
    for a_needs in (False, True):
        w = torch.rand(300, device=dev).requires_grad_(True)
        y = losses._ReduceMean.apply(a.clone().requires_grad_(a_needs), w, losses.RED_WMEAN, 0.0, 1.0)
        with pytest.raises(NotImplementedError):
            y.backward()


@pytest.mark.parametrize('alpha', [1.0, 0.0, -0.37])
@pytest.mark.parametrize('n', [1, 255, 257, 4 * 2048 * 256 + 5])
def test_axpy_vs_float64(dev, n, alpha):
    """dst += alpha * src.  Bar: alpha's own rounding to float32, one rounding of the product and one of the sum,
    2^-23 * (|dst| + 2 |alpha * src|) elementwise (derived, not measured).  n = 4 * 2048 * 256 + 5 reaches the grid-stride tail."""
    from animateportrait_amd import losses
    g = torch.Generator().manual_seed(n % 9973)
    dst = torch.randn(n, generator=g)
    src = torch.randn(n, generator=g) * 3
    d = dst.to(dev)
    assert losses.axpy_(d, src.to(dev), alpha) is d
    want = dst.double() + alpha * src.double()
    bar = 2.0 ** -23 * (dst.double().abs() + 2 * (alpha * src.double()).abs())
    err = (d.cpu().double() - want).abs()
    print('axpy n=%d alpha=%g: worst error / bar %.3f' % (n, alpha, float((err / bar.clamp_min(1e-300)).max())))
    assert bool((err <= bar).all())


def test_axpy_refuses_unequal_sizes(dev):
    from animateportrait_amd import losses
    with pytest.raises(ValueError):
        losses.axpy_(torch.zeros(8, device=dev), torch.zeros(9, device=dev))


# ------------------------------------------------------------------------------------------------------- bounds
@pytest.mark.parametrize('shape', [(3, 3, 5, 7), (2, 4, 17, 33)], ids=lambda s: 'x'.join(map(str, s)))
def test_composite_stays_inside_its_buffers(dev, shape):
    """HW = 35 and 561, forward with and without the appended channel and backward with GC = C and C + 1: the sentinels
    behind the output keep their bits."""
    from animateportrait_amd import losses
    lib, ptr, stream = _api()
    n, c, h, w = shape
    hw = h * w
    _, a, s1, sc, masks = _comp_inputs(*shape)
    ad, md, sd = a.to(dev), masks[0].to(dev), sc.to(dev)
    for mode, append, s, cs in ((1, 0, None, 0), (1, 1, None, 0), (3, 1, None, 0), (0, 0, None, 0), (2, 0, sd, c)):
        numel = n * (c + append) * hw
        buf, out = _padded(dev, numel)
        assert lib.ap_mask_composite(ptr(ad), ptr(md), ptr(s), n, c, cs, hw, mode, append, ptr(out), stream()) == 0
        assert _tail_intact(buf, numel) and _front_written(buf, numel), (mode, append)
        want = losses._Composite.apply(ad, md, s, mode, bool(append))
        assert torch.equal(out.view(want.shape), want)
    for mode, gc in ((1, c), (1, c + 1), (3, c + 1), (2, c)):
        gout = torch.randn(n, gc, h, w, generator=torch.Generator().manual_seed(gc)).to(dev)
        buf, ga = _padded(dev, n * c * hw)
        assert lib.ap_mask_composite_bwd(ptr(gout), ptr(md), n, c, gc, hw, mode, ptr(ga), stream()) == 0
        assert _tail_intact(buf, n * c * hw) and _front_written(buf, n * c * hw), (mode, gc)
        want = gout[:, :c] if mode == 3 else gout[:, :c] * md
        assert torch.equal(ga.view(n, c, h, w), want)


def test_crop_resize_stays_inside_its_buffers(dev):
    """Forward at 37 x 29 (1073 pixels a plane, off the 256 grid) and backward with gx padded behind N*C*H*W: the memset's
    length and the scatter both stop at the end of gx."""
    from animateportrait_amd import losses
    lib, ptr, stream = _api()
    n, c, oc = len(WINDOWS), 3, 4
    x = _crop_frames(c).to(dev)
    wd = losses.windows_to_device(WINDOWS, n, dev)
    chmap = losses._chmap((1, 1, 2, 0))
    for mode, (oh, ow) in ((1, (37, 29)), (0, (13, 11))):
        numel = n * oc * oh * ow
        buf, out = _padded(dev, numel)
        assert lib.ap_crop_resize_fwd(ptr(x), ctypes.c_void_p(wd.data_ptr()), n, c, CROP_H, CROP_W, oc, chmap, oh, ow, mode, 0.5, 0.5,
                                      ptr(out), stream()) == 0
        assert _tail_intact(buf, numel) and _front_written(buf, numel), mode
        assert torch.equal(out.view(n, oc, oh, ow), losses.crop_resize(x, wd, (1, 1, 2, 0), (oh, ow), mode, 0.5, 0.5))
        gout = torch.randn(n, oc, oh, ow, generator=torch.Generator().manual_seed(oh)).to(dev)
        gbuf, gx = _padded(dev, x.numel())
        assert lib.ap_crop_resize_bwd(ptr(gout), ctypes.c_void_p(wd.data_ptr()), n, c, CROP_H, CROP_W, oc, chmap, oh, ow, mode, 0.5,
                                      ptr(gx), stream()) == 0
        assert _tail_intact(gbuf, x.numel()) and _front_written(gbuf, x.numel()), mode
        assert bool(torch.isfinite(gx).all()) and float(gx.abs().sum()) > 0


def test_rasterisers_and_flow_post_stay_inside_their_buffers(dev):
    from animateportrait_amd import losses
    from animateportrait_amd.models.geomgm_ifw_fore_model import LIP_SEGMENTS
    lib, ptr, stream = _api()
    g = torch.Generator().manual_seed(17)
    # kp_to_map, S = 17
    lm = (torch.rand(2, 5, 2, generator=g) * 24 - 2).to(dev)
    buf, out = _padded(dev, 2 * 5 * 17 * 17)
    assert lib.ap_kp_to_map(ptr(lm), 2, 5, 17, 7.0, 8.0, 4.0, ptr(out), stream()) == 0
    assert _tail_intact(buf, out.numel()) and _front_written(buf, out.numel())
    assert torch.equal(out.view(2, 5, 17, 17), losses.kp_to_map(lm, 17))
    # flow_post, OS = 9, both outputs
    fo, vo = torch.randn(3, 2, 20, 20, generator=g).to(dev), torch.randint(0, 3, (3, 3, 20, 20), generator=g).float().to(dev)
    fbuf, wf = _padded(dev, 3 * 2 * 81)
    mbuf, rm = _padded(dev, 3 * 81)
    assert lib.ap_flow_post(ptr(fo), ptr(vo), 3, 3, 20, 9, 20.0, 8.0, 7.0, ptr(wf), ptr(rm), stream()) == 0
    assert _tail_intact(fbuf, wf.numel()) and _front_written(fbuf, wf.numel())
    assert _tail_intact(mbuf, rm.numel()) and _front_written(mbuf, rm.numel())
    want_f, want_m = losses.flow_post(fo, vo, 9)
    assert torch.equal(wf.view(3, 2, 9, 9), want_f) and torch.equal(rm.view(3, 1, 9, 9), want_m)
    # landmark_discs, 40 x 72
    pts = _disc_points(40, 72, g).to(dev)
    buf, out = _padded(dev, 3 * 40 * 72)
    assert lib.ap_landmark_discs(ptr(pts), 3, 12, 40, 72, 17, -1.0, 1.0, ptr(out), stream()) == 0
    assert _tail_intact(buf, out.numel()) and _front_written(buf, out.numel())
    assert torch.equal(out.view(3, 1, 40, 72), losses.landmark_discs(pts, 40, 72, 17))
    # lip_line_mask, size 33: the last sample's lines hang over the bottom and right edges
    lands = _lip_lands(33, g)
    lands[2, 48:68] = torch.rand(20, 2, generator=g) * 20 + 22.0
    lands = lands.to(dev)
    k = len(LIP_SEGMENTS)
    a = (ctypes.c_int32 * k)(*[s[0] for s in LIP_SEGMENTS])
    b = (ctypes.c_int32 * k)(*[s[1] for s in LIP_SEGMENTS])
    buf, out = _padded(dev, 3 * 33 * 33)
    assert lib.ap_lip_line_mask(ptr(lands), 3, 68, a, b, k, 33, 16, ptr(out), stream()) == 0
    assert _tail_intact(buf, out.numel()) and _front_written(buf, out.numel())
    want = losses.lip_line_mask(lands, LIP_SEGMENTS, 33, 16)
    assert torch.equal(out.view(3, 1, 33, 33), want) and float(want[2, 0, 32].sum()) > 0 and float(want[2, 0, :, 32].sum()) > 0


def test_reduce_backward_and_axpy_stay_inside_their_buffers(dev):
    lib, ptr, stream = _api()
    n = 257
    g = torch.Generator().manual_seed(257)
    a, b = torch.randn(n, generator=g).to(dev), torch.randn(n, generator=g).to(dev)
    gout = torch.tensor(3.0, device=dev)
    for op in (0, 1, 2):
        buf, ga = _padded(dev, n)
        assert lib.ap_reduce_mean_bwd(op, ptr(a), ptr(b), 1.0, n, 10.0, ptr(gout), ptr(ga), stream()) == 0
        assert _tail_intact(buf, n) and _front_written(buf, n), op
        want = (2 * (a.double() - 1.0), (a.double() - b.double()).sign(), b.double())[op] * (3.0 * 10.0 / n)
        assert linf(ga, want) <= 1e-6 * float(want.abs().max()), op
    buf, dst = _padded(dev, n)
    dst.copy_(a)
    assert lib.ap_axpy(ptr(dst), ptr(b), n, -0.37, stream()) == 0
    assert _tail_intact(buf, n) and _front_written(buf, n)
    assert linf(dst, a.double() - 0.37 * b.double()) < 1e-6
