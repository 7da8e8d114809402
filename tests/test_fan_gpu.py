"""The photo-landmark detector on the MI355X against its float64 statement (tests/fan_reference.py): apf_fan_crop bit for bit,
apf_fan_decode, the FAN forward at two small architectures and PhotoLandmarks.detect end to end."""
import numpy as np
import pytest
import torch

import fan_reference as R

pytestmark = pytest.mark.gpu
RES = 32


def _dev():
    return torch.device('cuda:0')


# ------------------------------------------------------------------------------------------------------------------- the crop
def _pictures():
    rs = np.random.RandomState(11)
    return {'40x56': rs.randint(0, 256, (40, 56, 3)).astype(np.uint8), '64x64': rs.randint(0, 256, (64, 64, 3)).astype(np.uint8)}


def _exact_box():
    """a box whose window is exactly RES x RES"""
    return next(b for b in ((10.0, 12.0, 10.0 + s, 12.0 + s) for s in np.arange(15.0, 18.0, 0.0125)) if R.window(b, RES)[2:] == (RES, RES))


CROP_BOXES = {
    'inside, up-scaling': (20.0, 12.0, 28.0, 20.0),
    'down-scaling': (20.0, 22.0, 44.0, 46.0),
    'over the left edge': (-6.0, 12.0, 6.0, 24.0),
    'over the right edge': (48.0, 12.0, 62.0, 26.0),
    'over the top edge': (20.0, -4.0, 32.0, 8.0),
    'over the bottom edge': (20.0, 30.0, 34.0, 44.0),
    'over the bottom right corner': (40.0, 28.0, 60.0, 47.0),
    'over the top left corner, odd sides': (-7.5, -3.25, 9.0, 11.5),
    'larger than the picture': (-10.0, -20.0, 70.0, 60.0),
    'wholly outside': (-300.0, -300.0, -200.0, -200.0),
    'window of RES x RES': None,
}


@pytest.mark.parametrize('order', ['bgr', 'rgb'])
@pytest.mark.parametrize('case', list(CROP_BOXES))
@pytest.mark.parametrize('pic', ['40x56', '64x64'])
def test_fan_crop_is_the_statement_bit_for_bit(pic, case, order):
    from animateportrait_amd import landmarks
    img = _pictures()[pic]
    box = CROP_BOXES[case] or _exact_box()
    ulx, uly, ww, wh = R.window(box, RES)
    if case == 'inside, up-scaling':
        assert ww < RES and 0 <= ulx and ulx + ww <= img.shape[1] and 0 <= uly and uly + wh <= img.shape[0]
    if case == 'down-scaling':
        assert ww > RES and wh > RES
    if case == 'window of RES x RES':
        assert 0 <= ulx and ulx + ww <= img.shape[1] and 0 <= uly and uly + wh <= img.shape[0]
    want = R.crop(img, box, RES, order, True)
    dimg = torch.from_numpy(img).to(_dev())
    got = landmarks.fan_crop(dimg, box, RES, order, True).cpu().numpy()
    assert got.shape == (2, 3, RES, RES)
    assert np.array_equal(np.rint(got * 255).astype(np.uint8), np.rint(want * 255).astype(np.uint8))      # the bytes
    assert np.array_equal(got, want)                                                                       # and byte / 255 in float32
    assert np.array_equal(got[1], got[0][:, :, ::-1])
    if case == 'wholly outside':
        assert not got.any()
    else:
        assert got.any()
    single = landmarks.fan_crop(dimg, box, RES, order, False).cpu().numpy()
    assert single.shape == (1, 3, RES, RES) and np.array_equal(single[0], want[0])


# ----------------------------------------------------------------------------------------------------------------- the decode
def _constructed_maps(B, Hm, seed):
    """asymmetric noise in +-0.1 below constructed peaks of 5: interior (with larger, smaller and equal neighbours), borders,
    corners and ties, a different construction per landmark"""
    rs = np.random.RandomState(seed)
    m = (0.2 * rs.rand(B, R.POINTS, Hm, Hm) - 0.1).astype(np.float32)
    e, c = Hm - 1, Hm // 2
    spots = [(c, c), (1, 1), (e - 1, e - 1), (0, c), (e, c), (c, 0), (c, e), (0, 0), (0, e), (e, 0), (e, e), (1, e - 1), (c - 1, c + 1 if c + 1 < e else c)]
    for b in range(B):
        for j in range(R.POINTS):
            y, x = spots[(j + 3 * b) % len(spots)]
            m[b, j, y, x] = 5.0
            kind = (j // len(spots) + b) % 4
            if kind == 1 and 0 < x < e and 0 < y < e:             # equal neighbours on x, unequal on y
                m[b, j, y, x - 1] = m[b, j, y, x + 1] = 1.0
                m[b, j, y - 1, x], m[b, j, y + 1, x] = 2.0, 1.0
            if kind == 2:                                         # a tie: a second, equal peak later in the map
                y2, x2 = spots[(j + 3 * b + 5) % len(spots)]
                m[b, j, y2, x2] = 5.0
            if kind == 3 and 0 < x < e and 0 < y < e:             # all four neighbours equal
                m[b, j, y, x - 1] = m[b, j, y, x + 1] = m[b, j, y - 1, x] = m[b, j, y + 1, x] = 3.0
    return m


def _boxes(B):
    return [(3.0 + 40 * b, 5.0 + 7 * b, 260.0 + 31 * b, 300.5 + 3 * b) for b in range(B)]


@pytest.mark.parametrize('truncate', [True, False])
@pytest.mark.parametrize('flip', [False, True])
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('Hm', [8, 64])
def test_fan_decode_is_the_statement(Hm, B, flip, truncate):
    from animateportrait_amd import landmarks
    hm = _constructed_maps(B, Hm, 100 + Hm + B)
    # flipped maps: asymmetric and strong enough to move some peaks -- a wrong pair table or a missing mirror changes the result
    hf = None
    if flip:
        rs = np.random.RandomState(7 + Hm + B)
        hf = (0.2 * rs.rand(B, R.POINTS, Hm, Hm) - 0.1).astype(np.float32)
        for b in range(B):
            for j in range(R.POINTS):
                hf[b, j, rs.randint(Hm), rs.randint(Hm)] = 3.0 + 4.0 * (j % 2)
    boxes = _boxes(B)
    want = R.decode(hm, boxes, hf, truncate)
    if flip:
        assert not np.array_equal(want, R.decode(hm, boxes, None, truncate))                                  # the flipped maps matter,
        assert not np.array_equal(want, R.decode(hm, boxes, hf[:, :, :, ::-1], truncate))                       # their mirror does,
        assert not np.array_equal(want, R.decode(hm, boxes, hf[:, R.PAIR], truncate))                          # and the pair table does
    dev = _dev()
    got = landmarks.fan_decode(torch.from_numpy(hm).to(dev), boxes, None if hf is None else torch.from_numpy(hf).to(dev), truncate).cpu().numpy()
    assert got.shape == (B, 68, 2) and got.dtype == np.float32
    err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    print('fan_decode Hm=%d B=%d flip=%d truncate=%d: max |difference| = %.3e px' % (Hm, B, flip, truncate, err))
    if truncate:
        assert np.array_equal(got, want)
    else:
        assert err <= 1e-4


# ---------------------------------------------------------------------------------------------------------------- the network
def _zero_some_gammas(sd):
    """a BatchNorm channel with g = 0 in front of a 3x3, a 1x1 (downsample) and an hourglass convolution: the affine route"""
    sd = dict(sd)
    for k in ('conv2.bn1.weight', 'conv4.downsample.0.weight', 'm0.b2_2.bn2.weight', 'top_m_0.bn3.weight'):
        v = sd[k].clone()
        v[1] = 0.0
        sd[k] = v
    return sd


_NET = {}


def network_case(num_modules, width, seed, zero_gammas=False):
    """(state_dict, input (2, 3, 128, 128) fp32, float64 maps, L-inf of the plain fp32 PyTorch statement against them), made once"""
    key = (num_modules, width, seed, zero_gammas)
    if key not in _NET:
        from animateportrait_amd import fan
        sd = fan.seeded_state_dict(num_modules, width, 4, seed)
        if zero_gammas:
            sd = _zero_some_gammas(sd)
        x = torch.rand(2, 3, 128, 128, generator=torch.Generator().manual_seed(seed + 1))
        with torch.no_grad():
            ref = R.fan_forward(R.cast(sd, torch.float64), x.double(), num_modules)
            plain = R.fan_forward(R.cast(sd, torch.float32), x, num_modules)
        _NET[key] = (sd, x, ref, float((plain.double() - ref).abs().max()))
    return _NET[key]


def device_fan(sd, num_modules, width):
    from animateportrait_amd import fan
    net = fan.FAN(num_modules, width, 4)
    net.load_state_dict(sd, strict=False)
    return net.to(_dev()).eval().prepare(_dev())


@pytest.mark.parametrize('num_modules,width,zero_gammas', [(2, 32, False), (1, 16, True)])
def test_fan_forward_against_float64(num_modules, width, zero_gammas):
    """The bar: 4 x the L-inf error of the plain fp32 PyTorch statement of the same network against float64 on the same input --
    a different but equally valid fp32 summation order (the margin profiles/speaker_embed.json uses)."""
    from animateportrait_amd import fan
    sd, x, ref, plain_err = network_case(num_modules, width, 3, zero_gammas)
    net = device_fan(sd, num_modules, width)
    routes = [bn.direct for _, blk in net._blocks() for bn, _ in blk._rt[0] + ([blk._rt[1]] if blk._rt[1] else [])]
    if zero_gammas:
        assert not net.conv2._rt[0][0][0].direct and not net.conv4._rt[1][0].direct and routes.count(False) == 4   # the affine route
    else:
        assert all(routes)
    got = net(x.to(_dev())).cpu()
    refused = [c.name for c in net.convs() if not all(c._served.values())]
    assert refused == ['conv1']                                 # the one fall-back layer was reached
    assert got.shape == ref.shape == (2, 68, 32, 32)
    err = float((got.double() - ref).abs().max())
    print('FAN(%d, %d) on 2 x 128 x 128: L-inf vs float64 = %.3e, plain fp32 statement %.3e, bar %.3e, map range %.3f'
          % (num_modules, width, err, plain_err, 4 * plain_err, float(ref.abs().max())))
    assert float(ref.abs().max()) > 1e-2 and plain_err > 0
    assert err <= 4 * plain_err


# ----------------------------------------------------------------------------------------------------------------- end to end
DETECT_SEED = 6


def detect_case():
    """picture, box and the float64 statement of one detection at FAN(2, 32) with a 128-pixel crop"""
    sd = network_case(2, 32, DETECT_SEED)[0]
    img = np.random.RandomState(DETECT_SEED).randint(0, 256, (64, 64, 3)).astype(np.uint8)
    box = (8.0, 6.0, 56.0, 58.0)
    if 'detect' not in _NET:
        with torch.no_grad():
            _NET['detect'] = R.detect(sd, img, box, 2, 4, 128, 'bgr', True, False)
    return sd, img, box, _NET['detect']


def reference_gaps(maps):
    """on the float64 maps of (plain, mirrored): per landmark the gap between the two largest values of the summed map, and the
    smallest non-zero |neighbour difference| the quarter-pixel step reads"""
    s = R.flip_sum(maps[:1], maps[1:2])[0]
    Hm = s.shape[-1]
    top, step = [], []
    for j in range(R.POINTS):
        flat = np.sort(s[j].reshape(-1))
        top.append(flat[-1] - flat[-2])
        idx = int(np.argmax(s[j]))
        px, py = idx % Hm, idx // Hm
        if 0 < px < Hm - 1 and 0 < py < Hm - 1:
            for d in (s[j, py, px + 1] - s[j, py, px - 1], s[j, py + 1, px] - s[j, py - 1, px]):
                if d != 0:
                    step.append(abs(d))
    return min(top), min(step) if step else np.inf


def test_detect_end_to_end_all_68_landmarks():
    from animateportrait_amd import landmarks
    sd, img, box, (want, maps) = detect_case()
    # the input of this comparison is the crop (bit-exact), so the maps' error is the network's: its bar at this architecture
    x = torch.from_numpy(R.crop(img, box, 128, 'bgr', True))
    with torch.no_grad():
        plain = R.fan_forward(R.cast(sd, torch.float32), x, 2).double().numpy()
    bar = 4 * float(np.abs(plain - maps).max())
    top, step = reference_gaps(maps)
    print('detect: heat-map bar %.3e; float64 reference: smallest top-two gap %.3e, smallest neighbour difference %.3e' % (bar, top, step))
    assert top > 8 * bar and step > 8 * bar, 'the seeded reference has a near-tie: pick another DETECT_SEED'
    det = landmarks.PhotoLandmarks(device_fan(sd, 2, 32), _dev(), resolution=128)
    got = det.detect(img, box, 'bgr', True, False)
    assert got.shape == (68, 3) and got.dtype == np.float32 and not got[:, 2].any()
    err = float(np.abs(got[:, :2].astype(np.float64) - want.astype(np.float64)).max())
    print('detect: max |difference| over all 68 landmarks = %.3e px' % err)
    assert err <= 1e-4
    # the public default truncates: the same positions, truncated toward zero
    trunc = det.detect(img, box)
    assert np.array_equal(trunc[:, :2], R.decode(maps[:1], [box], maps[1:2], True)[0])
