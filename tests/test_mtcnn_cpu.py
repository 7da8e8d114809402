"""MTCNN, host side: the weight loader's two layouts and the folded Flatten, the numpy restatement of the box arithmetic
(tests/mtcnn_reference.py) against every intermediate the reference recorded (tests/golden/mtcnn.npz), the C ABI of
libapface.so and its refusals (which need no device), and the crop arithmetic of align_photo."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import mtcnn_reference as ref          # noqa: E402
import cv_resize_reference as cvr      # noqa: E402

GOLDEN = os.path.join(HERE, 'golden')
WEIGHTS = os.path.join(GOLDEN, 'mtcnn_weights')


@pytest.fixture(scope='module')
def G():
    with np.load(os.path.join(GOLDEN, 'mtcnn.npz')) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope='module')
def photos():
    from PIL import Image
    return {n: np.asarray(Image.open(os.path.join(GOLDEN, 'mtcnn_%s.png' % n)).convert('RGB')) for n in ('wflw', 'teaser', 'blank')}


# ---- weights -----------------------------------------------------------------------------------------------------------------
def test_loader_reads_both_layouts(tmp_path):
    from animateportrait_amd import mtcnn, _faceapi as F
    packed = mtcnn.load_weights(WEIGHTS)
    assert {k: v.size for k, v in packed.items()} == {'pnet': F.PNET_PARAMS, 'rnet': F.RNET_PARAMS, 'onet': F.ONET_PARAMS}
    raw = mtcnn._read_raw(WEIGHTS)
    # the reference's layout: a pickled dict in a 0-d object array per net
    refdir = tmp_path / 'weights'
    refdir.mkdir()
    for net, params in raw.items():
        np.save(str(refdir / (net + '.npy')), np.array(params, dtype=object), allow_pickle=True)
    again = mtcnn.load_weights(str(refdir))
    # one plain .npz
    one = str(tmp_path / 'all.npz')
    np.savez(one, **{'%s/%s' % (net, k): v for net, params in raw.items() for k, v in params.items()})
    single = mtcnn.load_weights(one)
    for net in packed:
        assert np.array_equal(packed[net], again[net]) and np.array_equal(packed[net], single[net])
    with pytest.raises(FileNotFoundError):
        mtcnn.load_weights(str(tmp_path / 'nothing'))


def test_flatten_is_folded():
    """x.transpose(3, 2).view(n, -1) @ W.T == x.view(n, -1) @ folded, for the reference's Flatten and R-Net's first FC"""
    from animateportrait_amd import mtcnn
    rng = np.random.RandomState(0)
    w = mtcnn._read_raw(WEIGHTS)['rnet']['features.conv4.weight'].astype(np.float64)
    x = rng.randn(3, 64, 3, 3)
    x[:, :, 0, 1] += 5.0                                               # make h and w tell apart
    want = x.transpose(0, 1, 3, 2).reshape(3, -1) @ w.T
    folded = mtcnn.fold_flatten(w, (64, 3, 3))
    assert folded.shape == (576, 128)
    assert np.abs(x.reshape(3, -1) @ folded - want).max() < 1e-12
    assert np.abs(x.reshape(3, -1) @ w.T - want).max() > 1e-3          # and without the fold it is another function
    packed = mtcnn.load_weights(WEIGHTS)['rnet']
    start = 756 + 56 + 12096 + 96 + 12288 + 128
    assert np.array_equal(packed[start:start + 576 * 128].reshape(576, 128), folded.astype(np.float32))


# ---- the restatement against the golden ----------------------------------------------------------------------------------------
def test_pyramid_matches_golden(G, photos):
    from animateportrait_amd import mtcnn
    for name, a in photos.items():
        H, W = a.shape[:2]
        scales = ref.scales(W, H)
        assert np.array_equal(np.asarray(scales), G[name + '/scales'])
        sizes = [ref.level_size(W, H, s)[::-1] for s in scales]
        assert np.array_equal(np.asarray(sizes), G[name + '/sizes'])
        assert mtcnn.pyramid(W, H) == [(s, h, w) for s, (h, w) in zip(scales, sizes)]
        for k, (h, w) in enumerate(sizes):
            assert ref.pnet_map_size(h, w) == G['%s/L%d/prob' % (name, k)].shape


def test_bilinear_restatement_equals_pil(photos):
    from PIL import Image
    rng = np.random.RandomState(3)
    a = rng.randint(0, 256, (37, 53, 3)).astype(np.uint8)
    for oh, ow in ((12, 12), (13, 12), (24, 24), (48, 48), (80, 70), (37, 20)):
        assert np.array_equal(ref.resize_bilinear(a, oh, ow), np.asarray(Image.fromarray(a).resize((ow, oh), Image.BILINEAR)))
    t = photos['teaser']
    assert np.array_equal(ref.resize_bilinear(t, 96, 96), np.asarray(Image.fromarray(t).resize((96, 96), Image.BILINEAR)))


def test_box_arithmetic_reproduces_every_intermediate(G, photos):
    for name in ('wflw', 'teaser'):
        H, W = photos[name].shape[:2]
        levels = []
        for k, s in enumerate(G[name + '/scales']):
            cand = ref.generate_bboxes(G['%s/L%d/prob' % (name, k)], G['%s/L%d/off' % (name, k)], float(s), np.float32(0.6))
            assert np.array_equal(cand, G['%s/L%d/cand' % (name, k)])
            pick = ref.nms(cand, ref.LEVEL_NMS)
            assert np.array_equal(pick, G['%s/L%d/pick' % (name, k)])
            levels.append(cand[pick])
        merged = np.vstack(levels)
        assert np.array_equal(merged, G[name + '/s1/merged'])
        pick = ref.nms(merged, 0.7)
        assert np.array_equal(pick, G[name + '/s1/pick'])
        cal = ref.calibrate(merged[pick], merged[pick, 5:9])
        sq = ref.square(cal)
        b = ref.rounded(sq)
        for got, key in ((cal, 'cal'), (sq, 'sq'), (b, 'round')):
            assert np.array_equal(got, G['%s/s1/%s' % (name, key)]), key
        assert np.array_equal(ref.cutouts(photos[name], b, 24), G[name + '/s2/cut'])
        b = ref.clip_to_image(b, W, H)
        assert np.array_equal(b, G[name + '/s1/clipped'])

        prob, off = G[name + '/s2/prob'], G[name + '/s2/off']
        keep = np.nonzero(prob[:, 1] > np.float32(0.7))[0]
        b = b[keep]
        b[:, 4] = prob[keep, 1]
        assert np.array_equal(b, G[name + '/s2/filtered'])
        pick = ref.nms(b, 0.7)
        assert np.array_equal(pick, G[name + '/s2/pick'])
        cal = ref.calibrate(b[pick], off[keep][pick])
        sq = ref.square(cal)
        b = ref.rounded(sq)
        for got, key in ((cal, 'cal'), (sq, 'sq'), (b, 'round')):
            assert np.array_equal(got, G['%s/s2/%s' % (name, key)]), key
        assert np.array_equal(ref.cutouts(photos[name], b, 48), G[name + '/s3/cut'])
        b = ref.clip_to_image(b, W, H)
        assert np.array_equal(b, G[name + '/s2/clipped'])

        prob, off, lm = G[name + '/s3/prob'], G[name + '/s3/off'], G[name + '/s3/lm']
        keep = np.nonzero(prob[:, 1] > np.float32(0.8))[0]
        b = b[keep]
        b[:, 4] = prob[keep, 1]
        lm = ref.landmarks_to_image(b, lm[keep])
        cal = ref.calibrate(b, off[keep])
        assert np.array_equal(cal, G[name + '/s3/cal'])
        pick = ref.nms(cal, 0.7, 'min')
        assert np.array_equal(pick, G[name + '/s3/pick'])
        assert np.array_equal(cal[pick], G[name + '/boxes']) and np.array_equal(lm[pick], G[name + '/landmarks'])
    assert len(G['blank/boxes']) == 0 and all(len(G['blank/L%d/cand' % k]) == 0 for k in range(len(G['blank/scales'])))


def test_nms_tie_takes_the_higher_index_first():
    b = np.array([[0, 0, 10, 10, 0.5], [100, 0, 110, 10, 0.5], [200, 0, 210, 10, 0.25]], np.float64)
    assert list(ref.nms(b, 0.5)) == [1, 0, 2]
    assert list(ref.nms(np.zeros((0, 5)), 0.5)) == []


# ---- align_photo's crop arithmetic ---------------------------------------------------------------------------------------------
def test_align_window_hand_computed(G, photos):
    from animateportrait_amd import mtcnn
    # w = h = 101: size = int(121.2) = 121, cx = 100 + 50, size1 = int(round(172.857)) = 173,
    # x11 = int(150 - 86) = 64, y11 = int(150 - (173 * 11) // 20) = 150 - 95 = 55
    assert mtcnn.align_window([[100, 100, 200, 200, 0.9]]) == (64, 55, 173)
    # fractional corners: w = 61.0, h = 81.5: size = int(73.2) = 73, cx = 10.5 + 30.0, cy = 20.25 + 40.0,
    # size1 = int(round(104.29)) = 104, x11 = int(40.5 - 52) = -11, y11 = int(60.25 - 57) = 3
    assert mtcnn.align_window([[10.5, 20.25, 70.5, 100.75, 0.9]]) == (-11, 3, 104)
    # the largest `size` wins, the first of equals stays
    faces = [[0, 0, 20, 20, 0.99], [100, 100, 200, 200, 0.9], [300, 100, 400, 200, 0.95]]
    assert mtcnn.align_window(faces) == (64, 55, 173)
    assert mtcnn.align_window(np.zeros((0, 5))) is None
    for name in ('wflw', 'teaser'):
        assert mtcnn.align_window(G[name + '/boxes']) == ref.align_window(G[name + '/boxes']) == tuple(G[name + '/align_window'])
    # a face in the top-left corner of a 120 x 90 image: the padded square leaves the image on two sides
    img = np.arange(90 * 120 * 3, dtype=np.uint32).reshape(90, 120, 3).astype(np.uint8)
    win = mtcnn.align_window([[5, 8, 45, 48, 0.9]])                  # size 49, cx = 25, cy = 28, size1 = 70
    assert win == (-10, -10, 70)
    cut = ref.align_cut(img, win)
    assert cut.shape == (70, 70, 3) and (cut[:10] == 255).all() and (cut[:, :10] == 255).all()
    assert np.array_equal(cut[10:, 10:], img[:60, :60])
    # and on the other two
    cut = ref.align_cut(img, (80, 50, 70))
    assert np.array_equal(cut[:40, :40], img[50:, 80:]) and (cut[40:] == 255).all() and (cut[:, 40:] == 255).all()


def test_cubic_restatement_basics():
    a = np.random.RandomState(4).randint(0, 256, (9, 11, 3)).astype(np.uint8)
    assert np.array_equal(cvr.resize_cubic(a, 9, 11), a)                                 # same size: taps (0, 2048, 0, 0)
    flat = np.full((5, 7, 3), 93, np.uint8)
    assert np.array_equal(cvr.resize_cubic(flat, 32, 20), np.full((32, 20, 3), 93, np.uint8))   # weights sum to 2^11 per axis
    taps, weights = cvr.cubic_table(70, 512)
    assert abs(weights.sum(1) - 2048).max() <= 1 and taps.min() == 0 and taps.max() == 69      # each weight is rounded on its own


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_names_are_declared_and_exported():
    from animateportrait_amd import _faceapi as F, _capi, _dataapi, _styleapi
    header = open(os.path.join(ROOT, 'include', 'animateportrait_face.h')).read()
    declared = set(re.findall(r'\b(apf_\w+)\s*\(', header))
    assert declared == set(F.SIGNATURES)
    assert '#define APF_ABI_VERSION 1' in header and F.ABI_VERSION == 1
    lib = F.lib()
    assert all(hasattr(lib, n) for n in F.SIGNATURES) and lib.apf_abi_version() == 1
    for macro, value in (('APF_MAX_SIDE', F.MAX_SIDE), ('APF_MIN_LEVEL', F.MIN_LEVEL), ('APF_CAP_LEVEL', F.CAP_LEVEL),
                         ('APF_CAP_MERGED', F.CAP_MERGED), ('APF_CAP_RNET', F.CAP_RNET), ('APF_CAP_ONET', F.CAP_ONET),
                         ('APF_CAP_SORT', F.CAP_SORT), ('APF_PNET_PARAMS', F.PNET_PARAMS), ('APF_RNET_PARAMS', F.RNET_PARAMS),
                         ('APF_ONET_PARAMS', F.ONET_PARAMS), ('APF_OVF_LEVEL', F.OVF_LEVEL), ('APF_OVF_MERGED', F.OVF_MERGED),
                         ('APF_OVF_STAGE', F.OVF_STAGE)):
        assert re.search(r'#define %s %d\b' % (macro, value), header), macro
    for other in (_capi, _dataapi, _styleapi):                           # the other libraries' ABIs are untouched
        assert not any(n.startswith('apf_') for n in other.SIGNATURES)


def test_predicates_and_refusals_need_no_device():
    """*_ok accepts and refuses without a device; a refused call returns a negative code and a message before anything is
    launched: the pointers are never dereferenced, any non-null value stands in."""
    from animateportrait_amd import _faceapi as F
    lib = F.lib()
    p = 0x1000
    assert lib.apf_resize_level_ok(p, 106, 320, 64, 192, p) == 1
    assert lib.apf_resize_level_ok(None, 106, 320, 64, 192, p) == 0
    assert lib.apf_resize_level_ok(p, 106, 320, 0, 192, p) == 0
    assert lib.apf_resize_level_ok(p, 106, F.MAX_SIDE + 1, 64, 192, p) == 0
    assert lib.apf_pnet_ok(p, 12, 12, p, p) == 1 and lib.apf_pnet_ok(p, 12, 13, p, p) == 1
    assert lib.apf_pnet_ok(p, 11, 12, p, p) == 0 and lib.apf_pnet_ok(p, 12, 12, None, p) == 0
    assert lib.apf_stage1_level_ok(p, p, 91, 0.6, p, p, p) == 1
    assert lib.apf_stage1_level_ok(p, p, 0, 0.6, p, p, p) == 0 and lib.apf_stage1_level_ok(p, p, 91, 0.0, p, p, p) == 0
    assert lib.apf_box_stage_ok(p, 9, p, F.CAP_SORT, F.NMS_UNION, 0, None, p, p, F.CAP_RNET, p) == 1
    assert lib.apf_box_stage_ok(p, 5, p, 512, F.NMS_MIN, 1, p, p, p, 512, p) == 1
    assert lib.apf_box_stage_ok(p, 5, p, 512, F.NMS_MIN, 1, None, p, p, 512, p) == 0          # the last stage needs landmarks
    assert lib.apf_box_stage_ok(p, 7, p, 512, F.NMS_MIN, 0, None, p, p, 512, p) == 0          # stride
    assert lib.apf_box_stage_ok(p, 5, p, F.CAP_SORT + 1, F.NMS_MIN, 0, None, p, p, 512, p) == 0
    assert lib.apf_box_stage_ok(p, 5, p, 512, 2, 0, None, p, p, 512, p) == 0                  # mode
    assert lib.apf_cutouts_ok(p, 106, 320, p, p, F.CAP_RNET, 24, p) == 1 and lib.apf_cutouts_ok(p, 106, 320, p, p, 64, 48, p) == 1
    assert lib.apf_cutouts_ok(p, 106, 320, p, p, 64, 32, p) == 0 and lib.apf_cutouts_ok(p, 106, 320, p, p, 0, 24, p) == 0
    assert lib.apf_net_ok(F.NET_R, p, p, 64, p, p, p, p, None) == 1 and lib.apf_net_ok(F.NET_O, p, p, 64, p, p, p, p, p) == 1
    assert lib.apf_net_ok(F.NET_R, p, p, 64, p, p, p, p, p) == 0 and lib.apf_net_ok(F.NET_O, p, p, 64, p, p, p, p, None) == 0
    assert lib.apf_net_ok(2, p, p, 64, p, p, p, p, None) == 0
    assert lib.apf_crop_resize_cubic_ok(p, 106, 320, -10, -10, 70, 512, p) == 1
    assert lib.apf_crop_resize_cubic_ok(p, 106, 320, -10, -10, 0, 512, p) == 0
    assert lib.apf_crop_resize_cubic_ok(p, 106, 320, 1 << 20, 0, 70, 512, p) == 0
    # workspace sizes: R-Net keeps 28 x 22 x 22 and 28 x 11 x 11 floats per box, O-Net 32 x 46 x 46 and 32 x 23 x 23
    assert lib.apf_net_ws_bytes(F.NET_R, 10) == 10 * 4 * (13552 + 3388)
    assert lib.apf_net_ws_bytes(F.NET_O, 10) == 10 * 4 * (67712 + 16928)
    assert lib.apf_net_ws_bytes(F.NET_R, 0) < 0 and lib.apf_box_stage_ws_bytes(F.CAP_SORT + 1) < 0
    assert lib.apf_box_stage_ws_bytes(100) == 100 * 120
    # refused calls
    rc = lib.apf_pnet(p, 11, 40, p, 0.6, None, None, p, p, p, p, None)
    assert rc == -2 and 'level 11 x 40' in F.last_error()
    rc = lib.apf_cutouts(p, 106, 320, p, p, 64, 32, p, None)
    assert rc == -2 and 'size 32' in F.last_error()
    rc = lib.apf_net(F.NET_R, p, p, 64, p, p, p, p, p, None)
    assert rc == -1 and 'O-Net' in F.last_error()
    rc = lib.apf_crop_resize_cubic(p, 106, 320, 0, 0, 70, 256, 512, p, None)
    assert rc == -1 and 'fill' in F.last_error()
    with pytest.raises(RuntimeError, match='libapface'):
        F.check(lib.apf_resize_level(None, 1, 1, 1, 1, p, None), 'resize_level')
