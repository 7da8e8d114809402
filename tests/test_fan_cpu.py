"""The photo-landmark detector without a GPU: the float64 statement (tests/fan_reference.py) against constructions by hand, the
BatchNorm constants, the checkpoint loader, the host-only checks of the two new libapface entries and end2end's argument errors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

import fan_reference as R

A = 0x10000          # a stand-in address
BOX64 = (0.0, 0.0, 64.0, 64.0)


# ------------------------------------------------------------------------------------------------------------------ the decode
def _peak_map(Hm, peaks, base=0.0):
    """(1, 68, Hm, Hm) float32 maps, all ``base``, map j with the values of peaks[j] = {(y, x): v}"""
    m = np.full((1, R.POINTS, Hm, Hm), base, np.float32)
    for j, cells in peaks.items():
        for (y, x), v in cells.items():
            m[0, j, y, x] = v
    return m


def _expect(box, Hm, x, y, truncate):
    X, Y = R.transform(x, y, box, Hm)
    return (np.trunc(X), np.trunc(Y)) if truncate else (X, Y)


DECODE_CASES = [
    # name, cells of the map, expected (x, y) in 1-based map units before the transform
    ('interior, larger right and upper neighbour', {(3, 4): 5.0, (3, 5): 1.0, (2, 4): 2.0}, (5 + 0.25 - 0.5, 4 - 0.25 - 0.5)),
    ('interior, larger left and lower neighbour', {(3, 4): 5.0, (3, 3): 1.0, (4, 4): 2.0}, (5 - 0.25 - 0.5, 4 + 0.25 - 0.5)),
    ('interior, equal neighbours', {(3, 4): 5.0, (3, 3): 1.0, (3, 5): 1.0, (2, 4): 2.0, (4, 4): 2.0}, (5 - 0.5, 4 - 0.5)),
    ('top border', {(0, 4): 5.0, (0, 5): 1.0}, (5 - 0.5, 1 - 0.5)),
    ('bottom border', {(7, 4): 5.0, (7, 3): 1.0}, (5 - 0.5, 8 - 0.5)),
    ('left border', {(3, 0): 5.0, (4, 0): 1.0}, (1 - 0.5, 4 - 0.5)),
    ('right border', {(3, 7): 5.0, (2, 7): 1.0}, (8 - 0.5, 4 - 0.5)),
    ('corner 0 0', {(0, 0): 5.0}, (0.5, 0.5)),
    ('corner 0 7', {(0, 7): 5.0}, (7.5, 0.5)),
    ('corner 7 0', {(7, 0): 5.0}, (0.5, 7.5)),
    ('corner 7 7', {(7, 7): 5.0}, (7.5, 7.5)),
    ('tie: the lowest flat index', {(5, 2): 5.0, (2, 5): 5.0, (2, 6): 1.0}, (6 + 0.25 - 0.5, 3 - 0.5)),
    ('flat map: index 0', {}, (0.5, 0.5)),
]


@pytest.mark.parametrize('truncate', [True, False])
@pytest.mark.parametrize('name,cells,want', DECODE_CASES, ids=[c[0] for c in DECODE_CASES])
def test_the_statements_decode_returns_the_constructed_position(name, cells, want, truncate):
    box = (3.0, 5.0, 50.0, 61.0)
    got = R.decode(_peak_map(8, {j: cells for j in range(R.POINTS)}), [box], truncate=truncate)
    X, Y = _expect(box, 8, want[0], want[1], truncate)
    assert got.shape == (1, 68, 2) and got.dtype == np.float32
    assert np.all(got[0, :, 0] == np.float32(X)) and np.all(got[0, :, 1] == np.float32(Y))


def test_the_statements_flip_sum_mirrors_and_pairs():
    rs = np.random.RandomState(0)
    hm, hf = rs.randn(2, 68, 4, 4).astype(np.float32), rs.randn(2, 68, 4, 4).astype(np.float32)
    s = R.flip_sum(hm, hf)
    for j in (0, 16, 17, 30, 36, 41, 48, 55, 62, 67):
        assert np.array_equal(s[1, j], hm[1, j] + hf[1, R.PAIR[j]][:, ::-1])
    # a peak of the mirrored image's PAIRED map lands on the mirrored column
    m, f = _peak_map(8, {}), _peak_map(8, {45: {(2, 1): 3.0}})
    got = R.decode(m, [BOX64], f, truncate=False)
    X, Y = R.transform(7 - 0.5, 3 - 0.5, BOX64, 8)
    assert got[0, 36, 0] == np.float32(X) and got[0, 36, 1] == np.float32(Y)


def test_the_mirror_table_is_an_involution():
    from animateportrait_amd import landmarks
    assert landmarks.PAIR == R.PAIR and sorted(R.PAIR) == list(range(68))
    assert all(R.PAIR[R.PAIR[j]] == j for j in range(68))
    assert [j for j in range(68) if R.PAIR[j] == j] == [8, 27, 28, 29, 30, 33, 51, 57, 62, 66]
    assert (R.PAIR[0], R.PAIR[17], R.PAIR[21], R.PAIR[31], R.PAIR[32], R.PAIR[36], R.PAIR[40], R.PAIR[48], R.PAIR[55], R.PAIR[60],
            R.PAIR[65]) == (16, 26, 22, 35, 34, 45, 47, 54, 59, 64, 67)
    # the kernel's copy of the table
    src = open(os.path.join(ROOT, 'animateportrait_amd', 'csrc', 'face', 'face_fan.hip')).read()
    body = re.search(r'kPair\[APF_FAN_POINTS\] = \{([^}]*)\}', src).group(1)
    assert [int(v) for v in body.replace('\n', ' ').split(',')] == R.PAIR


# ---------------------------------------------------------------------------------------------------------- BatchNorm constants
def _bn_case(c, seed, zero=()):
    g = torch.Generator().manual_seed(seed)
    w, b = 0.5 + torch.rand(c, generator=g), torch.randn(c, generator=g)
    w[1] = -w[1]                                  # a negative scale: the kernels' loads need no rstd > 0
    for z in zero:
        w[z] = 0.0
    mu, var = torch.randn(c, generator=g), 0.2 + torch.rand(c, generator=g)
    y = 3 * torch.randn(2, c, 5, 7, generator=g, dtype=torch.float64)
    sd = {'bn.weight': w.double(), 'bn.bias': b.double(), 'bn.running_mean': mu.double(), 'bn.running_var': var.double()}
    return (w, b, mu, var), y, R._bn_relu(sd, 'bn', y)


def test_the_feat_form_of_batchnorm_relu_is_the_statements():
    from animateportrait_amd import fan
    p, y, want = _bn_case(6, 0)
    m, s, direct = fan.feat_constants(*p)
    assert direct and float(s[1]) < 0
    got = torch.relu((y - m.view(1, -1, 1, 1)) * s.view(1, -1, 1, 1))
    assert float((got - want).abs().max()) < 1e-12
    # ... and in the kernels' arithmetic, float32: within the rounding of the affine form's own sum, 2^-22 (|b| + |mu s| + |s y|)
    got32 = torch.relu((y.float() - m.float().view(1, -1, 1, 1)) * s.float().view(1, -1, 1, 1)).double()
    bound = 2.0 ** -22 * (p[1].abs() + (p[2] * s).abs()).view(1, -1, 1, 1).double() + 2.0 ** -22 * (s.view(1, -1, 1, 1) * y).abs()
    assert bool(((got32 - want).abs() <= bound + 1e-30).all())


def test_a_channel_with_gamma_zero_takes_the_affine_form():
    from animateportrait_amd import fan
    p, y, want = _bn_case(6, 1, zero=(3,))
    m, s, direct = fan.feat_constants(*p)
    assert not direct and float(s[3]) == 0.0 and bool(torch.isfinite(m).all())
    a, b = fan.bn_constants(*p)
    got = torch.relu(a.view(1, -1, 1, 1) * y + b.view(1, -1, 1, 1))
    assert float((got - want).abs().max()) < 1e-12
    assert float(got[:, 3].min()) == float(got[:, 3].max()) == max(float(p[1][3]), 0.0)
    tiny = list(p)
    tiny[0] = p[0].clone()
    tiny[0][3] = 0.5 * fan.S_MIN * float(torch.sqrt(p[3][3] + fan.BN_EPS))          # just below the threshold
    assert not fan.feat_constants(*tiny)[2]
    tiny[0][3] = 4 * tiny[0][3]
    assert fan.feat_constants(*tiny)[2]


def test_the_folded_post_activation_batchnorm_is_the_statements():
    from animateportrait_amd import fan
    g = torch.Generator().manual_seed(2)
    p, _, _ = _bn_case(6, 2, zero=(4,))
    w, cb = torch.randn(6, 3, 1, 1, generator=g), torch.randn(6, generator=g)
    x = torch.randn(2, 3, 5, 7, generator=g, dtype=torch.float64)
    sd = {'bn.weight': p[0].double(), 'bn.bias': p[1].double(), 'bn.running_mean': p[2].double(), 'bn.running_var': p[3].double()}
    want = R._bn_relu(sd, 'bn', torch.nn.functional.conv2d(x, w.double(), cb.double()))
    w2, b2 = fan.fold_post_bn(w, cb, *p)
    assert float((torch.relu(torch.nn.functional.conv2d(x, w2, b2)) - want).abs().max()) < 1e-12


# ------------------------------------------------------------------------------------------------------------------- the crop
def test_the_crop_statement_is_the_identity_for_a_window_of_r_by_r():
    rs = np.random.RandomState(3)
    img = rs.randint(0, 256, (64, 64, 3)).astype(np.uint8)
    Rr = 32
    # a box whose h = 200 scale is exactly R: transform is then a shift, ul = (1 + shift), window R - 1 ... find one with R x R
    box = next(b for b in ((10.0 + dx, 12.0 + dy, 10.0 + dx + s, 12.0 + dy + s) for s in np.arange(15.0, 18.0, 0.0125)
                           for dx in (0.0, 0.5) for dy in (0.0, 0.5)) if R.window(b, Rr)[2:] == (Rr, Rr))
    ulx, uly, ww, wh = R.window(box, Rr)
    assert 0 <= ulx and ulx + ww <= 64 and 0 <= uly and uly + wh <= 64
    assert np.array_equal(R.crop_u8(img, box, Rr), img[uly:uly + Rr, ulx:ulx + Rr])
    x = R.crop(img, box, Rr, 'rgb', True)
    assert x.shape == (2, 3, Rr, Rr) and x.dtype == np.float32
    assert np.array_equal(x[0], np.transpose(img[uly:uly + Rr, ulx:ulx + Rr], (2, 0, 1)).astype(np.float32) / np.float32(255))
    assert np.array_equal(x[1], x[0][:, :, ::-1])
    assert np.array_equal(R.crop(img, box, Rr, 'bgr', False)[0], x[0][::-1])


def test_the_crop_statement_zero_fills_and_resizes():
    img = np.full((40, 56, 3), 200, np.uint8)
    assert not R.crop_u8(img, (-300.0, -300.0, -200.0, -200.0), 32).any()                   # wholly outside
    over = R.crop_u8(img, (-20.0, -20.0, 20.0, 20.0), 32)                                 # hangs over the top left corner
    assert over[0, 0].tolist() == [0, 0, 0] and over[-1, -1].tolist() == [200, 200, 200]
    assert R.resize_linear_u8(np.full((7, 5, 3), 77, np.uint8), 32).min() == 77            # constants survive both passes
    ramp = np.tile(np.arange(0, 64, 4, dtype=np.uint8)[None, :, None], (16, 1, 3))
    up = R.resize_linear_u8(ramp, 32)[:, :, 0]
    assert np.array_equal(up[0], up[-1]) and np.all(np.diff(up[0].astype(int)) >= 0) and up[0, 0] == 0 and up[0, -1] == 60


# -------------------------------------------------------------------------------------------------------------------- loading
def _script_holder(sd):
    """a TorchScript archive whose state_dict is ``sd``: the keys' module tree with the tensors as parameters"""
    root = torch.nn.Module()
    for k, v in sd.items():
        mod, parts = root, k.split('.')
        for part in parts[:-1]:
            if part not in mod._modules:
                mod.add_module(part, torch.nn.Module())
            mod = mod._modules[part]
        mod.register_parameter(parts[-1], torch.nn.Parameter(v.clone(), requires_grad=False))
    return torch.jit.script(root)


@pytest.fixture(scope='module')
def small_sd():
    from animateportrait_amd import fan
    return fan.seeded_state_dict(2, 16, 4, seed=5)


@pytest.fixture()
def host_only(monkeypatch):
    """load_fan's own work only: prepare() puts constants on a device there is none of here"""
    from animateportrait_amd import fan
    monkeypatch.setattr(fan.FAN, 'prepare', lambda self, device=None: self)
    monkeypatch.setattr(fan.FAN, 'to', lambda self, *a, **k: self)


def _same(net, sd):
    own = {k: v for k, v in net.state_dict().items() if not k.endswith('num_batches_tracked')}
    return sorted(own) == sorted(sd) and all(torch.equal(own[k], sd[k]) for k in sd)


def test_load_fan_round_trips_a_state_dict_and_a_scripted_archive(tmp_path, small_sd, host_only):
    from animateportrait_amd import fan
    assert fan.architecture_of(small_sd) == (2, 16, 4)
    full = fan.FAN(2, 16, 4)
    full.load_state_dict(small_sd, strict=False)
    assert any(k.endswith('num_batches_tracked') for k in full.state_dict())
    plain = str(tmp_path / '3DFAN.pth.tar')
    torch.save(full.state_dict(), plain)                                      # with the counters, as the package saves it
    net = fan.load_fan(plain, 'cpu')
    assert (net.num_modules, net.width, net.depth) == (2, 16, 4) and _same(net, small_sd)
    wrapped = str(tmp_path / 'wrapped.pth')
    torch.save({'state_dict': small_sd, 'epoch': 3}, wrapped)
    assert _same(fan.load_fan(wrapped, 'cpu'), small_sd)
    scripted = str(tmp_path / '3DFAN4.zip')
    _script_holder(small_sd).save(scripted)
    assert _same(fan.load_fan(scripted, 'cpu'), small_sd)


def test_load_fan_is_strict_and_names_the_keys(tmp_path, small_sd, host_only):
    from animateportrait_amd import fan
    sd = dict(small_sd)
    sd['m1.b2_plus_1.bn2.gamma'] = sd.pop('m1.b2_plus_1.bn2.weight')
    path = str(tmp_path / 'renamed.pth')
    torch.save(sd, path)
    with pytest.raises(RuntimeError) as e:
        fan.load_fan(path, 'cpu')
    assert "missing keys ['m1.b2_plus_1.bn2.weight']" in str(e.value) and "unexpected keys ['m1.b2_plus_1.bn2.gamma']" in str(e.value)
    torch.save({'weight': torch.zeros(3)}, path)
    with pytest.raises(ValueError, match='no FAN state_dict'):
        fan.load_fan(path, 'cpu')


def test_the_full_architecture_has_the_packages_keys():
    from animateportrait_amd import fan
    keys = set(fan.FAN().state_dict())
    for k in ('conv1.weight', 'conv1.bias', 'bn1.running_var', 'conv2.downsample.0.weight', 'conv2.downsample.2.weight', 'conv3.bn1.bias',
              'conv4.conv3.weight', 'm0.b1_4.conv1.weight', 'm3.b2_plus_1.bn3.running_mean', 'm2.b3_1.conv2.weight', 'top_m_3.bn1.weight',
              'conv_last0.bias', 'bn_end3.weight', 'l3.bias', 'bl2.weight', 'al0.weight'):
        assert k in keys, k
    assert 'bl3.weight' not in keys and 'conv3.downsample.0.weight' not in keys and 'm0.b2_plus_2.conv1.weight' not in keys
    sd = fan.FAN().state_dict()
    assert sd['conv1.weight'].shape == (64, 3, 7, 7) and sd['conv4.downsample.2.weight'].shape == (256, 128, 1, 1)
    assert sd['m0.b1_1.conv1.weight'].shape == (128, 256, 3, 3) and sd['m0.b1_1.conv3.weight'].shape == (64, 64, 3, 3)
    assert sd['l0.weight'].shape == (68, 256, 1, 1) and sd['al0.weight'].shape == (256, 68, 1, 1)
    # 13 ConvBlocks per hourglass: three per level and the innermost one
    assert len({k.split('.')[1] for k in keys if k.startswith('m0.')}) == 13


def test_the_network_has_no_host_path():
    from animateportrait_amd import fan
    net = fan.FAN(1, 16, 4)
    with pytest.raises(RuntimeError, match='prepare'):
        net(torch.zeros(1, 3, 64, 64))


# --------------------------------------------------------------------------------------------------------- the host-only checks
def _crop_ok(img=A, H=512, W=512, x0=100.0, y0=120.0, x1=400.0, y1=430.0, R=256, flip=1, order=1, out=A):
    from animateportrait_amd import _faceapi
    return _faceapi.lib().apf_fan_crop_ok(img, H, W, x0, y0, x1, y1, R, flip, order, out)


def _boxes(rows):
    flat = [v for r in rows for v in r]
    return (ctypes.c_double * len(flat))(*flat)


def _decode_ok(hm=A, hmf=A, B=1, Hm=64, boxes='one', out=A):
    from animateportrait_amd import _faceapi
    buf = _boxes([(100.0, 120.0, 400.0, 430.0)] * max(B, 1)) if boxes == 'one' else boxes
    return _faceapi.lib().apf_fan_decode_ok(hm, hmf, B, Hm, None if buf is None else ctypes.cast(buf, ctypes.c_void_p), out)


@pytest.mark.parametrize('kw', [dict(), dict(flip=0, order=0), dict(R=2), dict(R=1024), dict(H=1, W=1), dict(H=8192, W=8192),
                                dict(x0=-500.0, y0=-400.0, x1=-100.0, y1=-90.0), dict(x0=0.0, y0=0.0, x1=3.0, y1=3.0, R=2)])
def test_fan_crop_ok_accepts_the_served_region(kw):
    from animateportrait_amd import _faceapi
    assert _crop_ok(**kw) == 1, _faceapi.last_error()


CROP_REFUSED = [
    (dict(img=None), -1, 'null image'), (dict(out=None), -1, 'null out'), (dict(H=0), -2, 'image 0 x 512'), (dict(W=8193), -2, 'image 512 x 8193'),
    (dict(R=0), -2, 'R = 0'), (dict(R=1025), -2, 'R = 1025'), (dict(flip=2), -1, 'flip = 2'), (dict(order=2), -1, 'channel order 2'),
    (dict(x1=100.0), -1, 'the box'), (dict(x1=99.0), -1, 'the box'), (dict(y1=120.0), -1, 'the box'), (dict(x0=float('nan')), -1, 'the box'),
    (dict(x1=1e9), -1, 'the box'), (dict(x0=0.0, y0=0.0, x1=0.5, y1=0.5, R=256), -2, 'window 0 x 0'),
]


@pytest.mark.parametrize('kw,code,names', CROP_REFUSED)
def test_fan_crop_refuses_and_names_the_reason(kw, code, names):
    """the _ok twin says no with the reason; the launching call returns the code without touching a device (there is none)"""
    from animateportrait_amd import _faceapi
    assert _crop_ok() == 1
    assert _crop_ok(**kw) == 0
    assert names in _faceapi.last_error(), _faceapi.last_error()
    args = dict(dict(img=A, H=512, W=512, x0=100.0, y0=120.0, x1=400.0, y1=430.0, R=256, flip=1, order=1, out=A), **kw)
    assert code == {-1: _faceapi.ERR_INVALID, -2: _faceapi.ERR_UNSUPPORTED}[code]
    assert _faceapi.lib().apf_fan_crop(*args.values(), None) == code
    assert names in _faceapi.last_error(), _faceapi.last_error()
    with pytest.raises(RuntimeError, match='libapface fan_crop'):
        _faceapi.check(code, 'fan_crop')


DECODE_REFUSED = [
    (dict(hm=None), -1, 'null hm'), (dict(out=None), -1, 'null hm / boxes / out'), (dict(boxes=None), -1, 'null hm / boxes / out'),
    (dict(B=0), -1, 'B = 0'), (dict(Hm=0), -1, 'Hm = 0'), (dict(B=17), -2, 'B = 17'), (dict(Hm=1025), -2, 'Hm = 1025'),
    (dict(boxes=_boxes([(5.0, 5.0, 5.0, 9.0)])), -1, 'box 0'), (dict(B=2, boxes=_boxes([(1.0, 1.0, 9.0, 9.0), (5.0, 5.0, 9.0, 4.0)])), -1, 'box 1'),
]


@pytest.mark.parametrize('kw,code,names', DECODE_REFUSED)
def test_fan_decode_refuses_and_names_the_reason(kw, code, names):
    from animateportrait_amd import _faceapi
    assert _decode_ok() == 1 and _decode_ok(hmf=None) == 1 and _decode_ok(B=16) == 1 and _decode_ok(Hm=1) == 1 and _decode_ok(Hm=1024) == 1
    assert _decode_ok(**kw) == 0
    assert names in _faceapi.last_error(), _faceapi.last_error()
    args = dict(dict(hm=A, hmf=A, B=1, Hm=64, boxes='one', out=A), **kw)
    buf = _boxes([(100.0, 120.0, 400.0, 430.0)] * max(args['B'], 1)) if args['boxes'] == 'one' else args['boxes']
    rc = _faceapi.lib().apf_fan_decode(args['hm'], args['hmf'], args['B'], args['Hm'], None if buf is None else ctypes.cast(buf, ctypes.c_void_p),
                                       1, args['out'], None)
    assert rc == code and names in _faceapi.last_error(), _faceapi.last_error()


def test_header_and_binding_agree_on_the_fan_entries():
    from animateportrait_amd import _faceapi
    hdr = open(os.path.join(ROOT, 'include', 'animateportrait_face.h')).read()
    for macro, value in (('APF_FAN_POINTS', _faceapi.FAN_POINTS), ('APF_FAN_MAX_RES', _faceapi.FAN_MAX_RES), ('APF_FAN_MAX_B', _faceapi.FAN_MAX_B),
                         ('APF_ABI_VERSION', 1)):
        assert int(re.search(r'#define\s+%s\s+(\d+)' % macro, hdr).group(1)) == value, macro
    for name in ('apf_fan_crop', 'apf_fan_crop_ok', 'apf_fan_decode', 'apf_fan_decode_ok'):
        assert name in _faceapi.SIGNATURES and hasattr(_faceapi.lib(), name) and re.search(r'\b%s\(' % name, hdr)
    assert _faceapi.lib().apf_abi_version() == 1


def test_the_wrappers_have_no_host_path():
    from animateportrait_amd import landmarks
    with pytest.raises(TypeError, match='GPU'):
        landmarks.fan_crop(torch.zeros(8, 8, 3, dtype=torch.uint8), BOX64)
    with pytest.raises(TypeError, match='GPU'):
        landmarks.fan_decode(torch.zeros(1, 68, 8, 8), [BOX64])
    with pytest.raises(Exception):
        landmarks.parse_box('1,2,3')
    assert landmarks.parse_box('1,2.5,3,4') == [1.0, 2.5, 3.0, 4.0]


# --------------------------------------------------------------------------------------------------------------------- end2end
BASE = ['--photo', 'p.png', '--out', 'o']
WAV = BASE + ['--wav', 'a.wav', '--speaker_emb', 's.txt']


def test_end2end_parser_takes_the_photo_landmark_options():
    from animateportrait_amd import end2end
    ap = end2end.make_parser()
    a = ap.parse_args(BASE)
    assert a.photo_landmarks_from == 'txt' and a.fan_weights is None and a.face_box is None          # the default selects nothing new
    a = ap.parse_args(WAV + ['--photo_landmarks_from', 'photo', '--fan_weights', 'fan.pth', '--face_box', '10,20,300,310.5'])
    assert a.photo_landmarks_from == 'photo' and a.fan_weights == 'fan.pth' and a.face_box == [10.0, 20.0, 300.0, 310.5]
    with pytest.raises(SystemExit):
        ap.parse_args(BASE + ['--photo_landmarks_from', 'face_alignment'])
    with pytest.raises(SystemExit):
        ap.parse_args(BASE + ['--face_box', '1,2,3'])


@pytest.mark.parametrize('args,names', [
    (BASE + ['--landmarks_npy', 'l.npy', '--photo_landmarks_from', 'photo', '--fan_weights', 'f.pth'], '--photo_landmarks_from photo needs --wav'),
    (WAV + ['--photo_landmarks_from', 'photo'], '--photo_landmarks_from photo needs --fan_weights'),
    (WAV + ['--photo_landmarks_from', 'photo', '--fan_weights', 'f.pth', '--photo_landmarks', 'lm.txt'], 'does not go with --photo_landmarks'),
    (WAV + ['--photo_landmarks', 'lm.txt', '--fan_weights', 'f.pth'], '--fan_weights goes with --photo_landmarks_from photo'),
    (WAV + ['--photo_landmarks_from', 'txt', '--photo_landmarks', 'lm.txt', '--fan_weights', 'f.pth'], '--fan_weights goes with'),
    (WAV + ['--photo_landmarks', 'lm.txt', '--face_box', '1,2,3,4'], '--face_box goes with --photo_landmarks_from photo'),
    (WAV, '--wav needs --photo_landmarks'),                                       # one of the two sources
    (WAV + ['--photo_landmarks_from', 'txt'], '--wav needs --photo_landmarks'),
])
def test_end2end_refuses_contradicting_photo_landmark_options(args, names, capsys):
    """argparse errors: raised before any file is read or the device is touched"""
    from animateportrait_amd import end2end
    with pytest.raises(SystemExit) as e:
        end2end.main(args)
    assert e.value.code == 2 and names in capsys.readouterr().err
