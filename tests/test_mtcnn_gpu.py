"""MTCNN on the device (libapface.so, animateportrait_amd/mtcnn.py) against the reference's recorded stages
(tests/golden/mtcnn.npz, written by make_mtcnn_golden.py), PIL itself and the numpy restatements (mtcnn_reference.py,
cv_resize_reference.py).

Tolerances.  Nets: L-inf against the golden's float64 outputs at most 8 x the reference's own fp32 error against them
(e_ref_*; both sides are fp32 with another summation order over up to 1152 terms), and below 1e-4, a tenth of the 1e-3
margin the fixtures keep from every decision.  End to end: 0.05 px (a 1e-4 score-class error times boxes below 200 px).
Resamplers and box arithmetic: exact.

Measured on an MI355X: see DESIGN.md section 4c-7."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import mtcnn_reference as ref          # noqa: E402
import cv_resize_reference as cvr      # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(HERE, 'golden')
IMAGES = ('wflw', 'teaser', 'blank')
FACES = {'wflw': 8, 'teaser': 1, 'blank': 0}


@pytest.fixture(scope='module')
def G():
    with np.load(os.path.join(GOLDEN, 'mtcnn.npz')) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope='module')
def photos():
    from PIL import Image
    return {n: np.asarray(Image.open(os.path.join(GOLDEN, 'mtcnn_%s.png' % n)).convert('RGB')) for n in IMAGES}


@pytest.fixture(scope='module')
def det():
    from animateportrait_amd import mtcnn
    return mtcnn.Detector(os.path.join(GOLDEN, 'mtcnn_weights'))


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype else t).cuda()


def i32(v):
    return torch.tensor([v], dtype=torch.int32, device='cuda')


def pil_resize(a, oh, ow):
    from PIL import Image
    return np.asarray(Image.fromarray(a).resize((ow, oh), Image.BILINEAR))


# ---- pyramid and cut-outs: bit-exact against PIL ---------------------------------------------------------------------------
def test_pyramid_levels_equal_pil(det, photos, G):
    rng = np.random.RandomState(0)
    src = rng.randint(0, 256, (37, 53, 3)).astype(np.uint8)
    cases = [(src, 12, 12), (src, 12, 13), (src, 13, 12), (src, 37, 53), (src, 80, 70)]
    for name in IMAGES:
        cases += [(photos[name], int(h), int(w)) for h, w in G[name + '/sizes']]
    for a, oh, ow in cases:
        got = det.resize_level(dev(a), oh, ow).cpu().numpy()
        assert np.array_equal(got, pil_resize(a, oh, ow)), (a.shape, oh, ow)


def _pil_cutouts(image, boxes, size):
    """get_image_boxes with PIL, from the window arithmetic of mtcnn_reference"""
    H, W = image.shape[:2]
    out = np.zeros((len(boxes), size, size, 3), np.uint8)
    for i, (x1, y1, w, h) in enumerate(ref.cutout_windows(boxes, W, H)):
        win = np.zeros((h, w, 3), np.uint8)
        xa, xb, ya, yb = max(x1, 0), min(x1 + w, W), max(y1, 0), min(y1 + h, H)
        win[ya - y1:yb - y1, xa - x1:xb - x1] = image[ya:yb, xa:xb]
        out[i] = pil_resize(win, size, size)
    return out


@pytest.mark.parametrize('size', [24, 48])
def test_cutouts_equal_pil(det, photos, size):
    image = photos['teaser']                                           # 160 x 160
    boxes = np.array([[20, 30, 70, 90, 0], [100, 40, 123, 63, 0],      # inside (the second: exactly 24 wide)
                      [-15, 50, 40, 110, 0], [120, 60, 190, 130, 0],   # across the left / the right edge
                      [-10, -20, 60, 50, 0], [110, 120, 180, 200, 0],  # across two edges
                      [-40, -30, 220, 230, 0], [5, 7, 9, 12, 0]],      # larger than the image; smaller than the cut
                     np.float64)
    b = dev(boxes)
    got = det.cutouts(dev(image), b, i32(len(boxes)), 16, size).cpu().numpy()
    assert np.array_equal(got[:len(boxes)], _pil_cutouts(image, boxes, size))
    assert np.array_equal(b.cpu().numpy(), ref.clip_to_image(boxes, 160, 160))       # the side effect of correct_bboxes


def test_cutouts_equal_golden(det, photos, G):
    for name in ('wflw', 'teaser'):
        for stage, size, key in (('s1', 24, 's2/cut'), ('s2', 48, 's3/cut')):
            boxes = G['%s/%s/round' % (name, stage)]
            b = dev(boxes)
            got = det.cutouts(dev(photos[name]), b, i32(len(boxes)), len(boxes), size).cpu().numpy()
            assert np.array_equal(got, G['%s/%s' % (name, key)])
            assert np.array_equal(b.cpu().numpy(), G['%s/%s/clipped' % (name, stage)])


# ---- nets ------------------------------------------------------------------------------------------------------------------
def _bound(G, key):
    return min(8 * float(G[key]), 1e-4)


def test_pnet_maps(det, photos, G):
    worst = 0.0
    rng = np.random.RandomState(1)
    for name in IMAGES:
        for k, (h, w) in enumerate(G[name + '/sizes']):
            level = pil_resize(photos[name], int(h), int(w))
            prob, off = det.pnet(dev(level), 0.6, maps=True)[:2]
            assert prob.shape == G['%s/L%d/prob64' % (name, k)].shape
            worst = max(worst, np.abs(prob.cpu().numpy() - G['%s/L%d/prob64' % (name, k)]).max(),
                        np.abs(off.cpu().numpy() - G['%s/L%d/off64' % (name, k)]).max())
    print('P-Net L-inf vs float64: %.3e (bound %.3e)' % (worst, _bound(G, 'e_ref_pnet')))
    assert worst <= _bound(G, 'e_ref_pnet')
    # one output; an odd H-2 / W-2: the partial pool window adds a second row / column
    for (h, w), shape in (((12, 12), (1, 1)), ((13, 12), (2, 1)), ((12, 13), (1, 2))):
        prob, off = det.pnet(dev(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)), 0.6, maps=True)[:2]
        assert prob.shape == shape and off.shape == (4,) + shape and bool(torch.isfinite(prob).all())


def test_pnet_small_levels_match_torch(det):
    """12 x 12, 13 x 12, 12 x 13 and a level that is no multiple of the tile, against the same layers in float64 torch"""
    import torch.nn.functional as Fn
    from animateportrait_amd import mtcnn
    raw = mtcnn._read_raw(os.path.join(GOLDEN, 'mtcnn_weights'))['pnet']
    p = {k: torch.from_numpy(v).double() for k, v in raw.items()}
    rng = np.random.RandomState(2)
    for h, w in ((12, 12), (13, 12), (12, 13), (45, 31)):
        level = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        x = ((torch.from_numpy(level).double() - 127.5) * 0.0078125).permute(2, 0, 1)[None]
        x = Fn.prelu(Fn.conv2d(x, p['features.conv1.weight'], p['features.conv1.bias']), p['features.prelu1.weight'])
        x = Fn.max_pool2d(x, 2, 2, ceil_mode=True)
        x = Fn.prelu(Fn.conv2d(x, p['features.conv2.weight'], p['features.conv2.bias']), p['features.prelu2.weight'])
        x = Fn.prelu(Fn.conv2d(x, p['features.conv3.weight'], p['features.conv3.bias']), p['features.prelu3.weight'])
        want_p = Fn.softmax(Fn.conv2d(x, p['conv4_1.weight'], p['conv4_1.bias']), 1)[0, 1].numpy()
        want_o = Fn.conv2d(x, p['conv4_2.weight'], p['conv4_2.bias'])[0].numpy()
        prob, off = det.pnet(dev(level), 0.6, maps=True)[:2]
        assert np.abs(prob.cpu().numpy() - want_p).max() < 1e-5 and np.abs(off.cpu().numpy() - want_o).max() < 1e-5, (h, w)


@pytest.mark.parametrize('which', ['r', 'o'])
def test_rnet_onet_on_golden_cutouts(det, G, which):
    stage = 's2' if which == 'r' else 's3'
    worst = 0.0
    for name in ('wflw', 'teaser'):
        cuts = G['%s/%s/cut' % (name, stage)]
        n = len(cuts)
        probs, offs, lm = det.net(which, dev(cuts), i32(n), n + 3)
        worst = max(worst, np.abs(probs[:n].cpu().numpy() - G['%s/%s/prob64' % (name, stage)]).max(),
                    np.abs(offs[:n].cpu().numpy() - G['%s/%s/off64' % (name, stage)]).max())
        if which == 'o':
            worst = max(worst, np.abs(lm[:n].cpu().numpy() - G['%s/s3/lm64' % name]).max())
        assert float(probs[n:].abs().max()) == 0.0                       # rows beyond the count are not touched
    key = 'e_ref_rnet' if which == 'r' else 'e_ref_onet'
    print('%s-Net L-inf vs float64: %.3e (bound %.3e)' % (which.upper(), worst, _bound(G, key)))
    assert worst <= _bound(G, key)


# ---- box arithmetic: exact ---------------------------------------------------------------------------------------------------
def test_candidates_and_level_nms(det, G):
    from animateportrait_amd import _faceapi as F
    for name in ('wflw', 'teaser'):
        merged = torch.zeros((F.CAP_MERGED, 9), dtype=torch.float64, device='cuda')
        n_merged, status, n_level = i32(0), i32(0), i32(0)
        for k, s in enumerate(G[name + '/scales']):
            prob, off = G['%s/L%d/prob' % (name, k)], G['%s/L%d/off' % (name, k)]
            iy, ix = np.nonzero(prob > np.float32(0.6))
            order = np.random.RandomState(k).permutation(iy.size)         # the kernel appends in no fixed order
            idx = (iy * prob.shape[1] + ix)[order].astype(np.int32)
            cand = (None, None, dev(idx), dev(prob[iy, ix][order]), dev(off[:, iy, ix].T[order]), i32(iy.size))
            boxes = det.stage1_level(cand, prob.shape[1], float(s), merged, n_merged, status, n_level)
            want = G['%s/L%d/cand' % (name, k)]
            assert np.array_equal(boxes[:len(want)].cpu().numpy(), want)
            assert int(n_level) == len(G['%s/L%d/pick' % (name, k)])
        want = G[name + '/s1/merged']
        assert int(n_merged) == len(want) and int(status) == 0
        assert np.array_equal(merged[:len(want)].cpu().numpy(), want)


def test_box_stages_equal_golden(det, G):
    from animateportrait_amd import _faceapi as F
    for name in ('wflw', 'teaser'):
        m = G[name + '/s1/merged']
        out, _, n, (picks, cal, sq) = det.box_stage(dev(m), i32(len(m)), len(m) + 5, len(m), 0.7, F.NMS_UNION, trace=True)
        k = int(n)
        assert np.array_equal(picks[:k].cpu().numpy(), G[name + '/s1/pick']) and int(picks[k]) == -1
        for got, key in ((cal, 'cal'), (sq, 'sq'), (out, 'round')):
            assert np.array_equal(got[:k].cpu().numpy(), G['%s/s1/%s' % (name, key)]), key
        b = G[name + '/s1/clipped']
        out, _, n, (picks, cal, sq) = det.box_stage(dev(b), i32(len(b)), len(b), len(b), 0.7, F.NMS_UNION, probs=dev(G[name + '/s2/prob']),
                                                    offsets=dev(G[name + '/s2/off']), score_threshold=0.7, trace=True)
        k = int(n)
        assert np.array_equal(picks[:k].cpu().numpy(), G[name + '/s2/pick'])
        for got, key in ((cal, 'cal'), (sq, 'sq'), (out, 'round')):
            assert np.array_equal(got[:k].cpu().numpy(), G['%s/s2/%s' % (name, key)]), key
        b = G[name + '/s2/clipped']
        out, lm, n, (picks, cal, _) = det.box_stage(dev(b), i32(len(b)), len(b), len(b), 0.7, F.NMS_MIN, late=True,
                                                    probs=dev(G[name + '/s3/prob']), offsets=dev(G[name + '/s3/off']),
                                                    landmarks=dev(G[name + '/s3/lm']), score_threshold=0.8, trace=True)
        k = int(n)
        assert k == FACES[name] and np.array_equal(picks[:k].cpu().numpy(), G[name + '/s3/pick'])
        assert np.array_equal(cal[:len(G[name + '/s3/cal'])].cpu().numpy(), G[name + '/s3/cal'])
        assert np.array_equal(out[:k].cpu().numpy(), G[name + '/boxes'])
        assert np.array_equal(lm[:k].cpu().numpy(), G[name + '/landmarks'])


def _random_boxes(n, seed):
    rng = np.random.RandomState(seed)
    xy = rng.randint(0, 300, (n, 2)).astype(np.float64)
    wh = rng.randint(10, 60, (n, 2)).astype(np.float64)
    score = rng.permutation(n).astype(np.float32) / np.float32(n) * np.float32(0.5) + np.float32(0.4)      # distinct fp32 scores
    off = (rng.rand(n, 4).astype(np.float32) - np.float32(0.5)) * np.float32(0.2)
    return np.concatenate([xy, xy + wh, score[:, None].astype(np.float64), off.astype(np.float64)], 1)


@pytest.mark.parametrize('mode', ['union', 'min'])
@pytest.mark.parametrize('n', [0, 1, 257, 4096])
def test_nms_sizes_and_modes(det, n, mode):
    """n = 0, 1, more than one sort round, and the capacity; both modes; against the restatement, order included"""
    from animateportrait_amd import _faceapi as F
    b = _random_boxes(n, n + 1)
    cap = max(n, 1)
    out, _, n_out, (picks, cal, sq) = det.box_stage(dev(b.reshape(-1, 9)) if n else torch.zeros((1, 9), dtype=torch.float64, device='cuda'),
                                                    i32(n), cap, cap, 0.5, F.NMS_MIN if mode == 'min' else F.NMS_UNION, trace=True)
    want = ref.nms(b, 0.5, mode) if n <= 257 else _fast_nms(b, 0.5, mode)
    k = int(n_out)
    assert k == len(want) and np.array_equal(picks[:k].cpu().numpy(), want)
    if n:
        c = ref.calibrate(b[want], b[want, 5:9])
        assert np.array_equal(cal[:k].cpu().numpy(), c)
        assert np.array_equal(sq[:k].cpu().numpy(), ref.square(c))
        assert np.array_equal(out[:k].cpu().numpy(), ref.rounded(ref.square(c)))


def _fast_nms(b, thr, mode):
    """the same greedy sweep, vectorised over the lower-ranked boxes (for the capacity-sized case)"""
    order = np.lexsort((np.arange(len(b)), b[:, 4]))
    area = (b[:, 2] - b[:, 0] + 1.0) * (b[:, 3] - b[:, 1] + 1.0)
    alive = np.ones(len(b), bool)
    pick = []
    for r in range(len(b) - 1, -1, -1):
        if not alive[r]:
            continue
        i, rest = order[r], order[:r]
        pick.append(i)
        w = np.maximum(0.0, np.minimum(b[i, 2], b[rest, 2]) - np.maximum(b[i, 0], b[rest, 0]) + 1.0)
        h = np.maximum(0.0, np.minimum(b[i, 3], b[rest, 3]) - np.maximum(b[i, 1], b[rest, 1]) + 1.0)
        inter = w * h
        o = inter / np.minimum(area[i], area[rest]) if mode == 'min' else inter / (area[i] + area[rest] - inter)
        alive[:r] &= ~(o > thr)
    return np.asarray(pick, np.int64)


def test_capacity_plus_one_reports_overflow(det):
    """more picks than cap_out: the status says so, the first cap_out picks are kept and nothing is written past them; and a
    level with one candidate more than APF_CAP_LEVEL"""
    from animateportrait_amd import _faceapi as F
    n = 40
    b = np.zeros((n, 9))
    b[:, 0] = np.arange(n) * 100.0                                      # disjoint boxes: every one is a pick
    b[:, 2] = b[:, 0] + 20
    b[:, 3] = 20
    b[:, 4] = (np.arange(n, dtype=np.float32) + np.float32(1)) / np.float32(64)
    status = i32(0)
    cap_out = n - 1
    out = torch.full((cap_out + 8, 5), -7.0, dtype=torch.float64, device='cuda')
    n_out = i32(0)
    ws = torch.empty(int(det.lib.apf_box_stage_ws_bytes(n)), dtype=torch.uint8, device='cuda')
    b_dev, n_dev = dev(b), i32(n)
    F.check(det.lib.apf_box_stage(b_dev.data_ptr(), 9, n_dev.data_ptr(), n, None, None, None, 0.0, 0.5, F.NMS_UNION, 0, out.data_ptr(), None,
                                  n_out.data_ptr(), cap_out, None, None, None, status.data_ptr(), ws.data_ptr(), None))
    torch.cuda.synchronize()
    assert int(n_out) == cap_out and int(status) == F.OVF_STAGE
    assert np.array_equal(out[:cap_out, 0].cpu().numpy(), b[::-1][:cap_out, 0])          # highest score first
    assert bool((out[cap_out:] == -7.0).all())
    # a level: CAP_LEVEL + 1 candidates announced, CAP_LEVEL stored
    cap = F.CAP_LEVEL
    k = torch.arange(cap, dtype=torch.int32, device='cuda')
    idx = (k // 8) * 10 * 64 + (k % 8) * 8                                                # 8 columns, 10 rows apart: every one is a pick
    score = (torch.arange(cap, dtype=torch.float32, device='cuda') + 1) / 8192 + 0.25
    merged = torch.full((F.CAP_MERGED + 4, 9), -7.0, dtype=torch.float64, device='cuda')
    n_merged, status = i32(3), i32(0)
    cand = (None, None, idx, score, torch.zeros((cap, 4), device='cuda'), i32(cap + 1))
    det.stage1_level(cand, 64, 0.6, merged, n_merged, status)
    assert int(n_merged) == F.CAP_MERGED and int(status) == (F.OVF_LEVEL | F.OVF_MERGED)
    assert bool((merged[F.CAP_MERGED:] == -7.0).all()) and bool((merged[:3] == -7.0).all())


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def test_detect_matches_golden(det, photos, G):
    singles = {}
    worst = 0.0
    for name in IMAGES:
        boxes, lm = det.detect(photos[name])
        singles[name] = (boxes, lm)
        assert boxes.shape == (FACES[name], 5) and lm.shape == (FACES[name], 10) and boxes.dtype == np.float64
        if FACES[name]:
            worst = max(worst, np.abs(boxes - G[name + '/boxes']).max(), np.abs(lm - G[name + '/landmarks']).max())
    print('end to end: max |box, landmark| difference %.3e px' % worst)
    assert worst <= 0.05
    batch = det.detect_batch([photos[n] for n in IMAGES])
    for name, (boxes, lm) in zip(IMAGES, batch):
        assert np.array_equal(boxes, singles[name][0]) and np.array_equal(lm, singles[name][1])


def test_align_photo_and_cli(det, photos, G, tmp_path):
    from PIL import Image
    from animateportrait_amd import align
    with np.load(os.path.join(GOLDEN, 'mtcnn_aligned.npz')) as z:
        want = {k: z[k] for k in z.files}
    for name in ('wflw', 'teaser'):
        got = det.align_photo(photos[name])
        assert got.shape == (512, 512, 3) and got.dtype == np.uint8
        assert np.array_equal(got, want[name])
        window = tuple(int(v) for v in G[name + '/align_window'])
        assert np.array_equal(got, cvr.resize_cubic(ref.align_cut(photos[name], window), 512, 512))
    assert det.align_photo(photos['blank']) is None
    out = str(tmp_path / 'ori.png')
    align.main(['--photo', os.path.join(GOLDEN, 'mtcnn_teaser.png'), '--out', out, '--mtcnn_weights', os.path.join(GOLDEN, 'mtcnn_weights')])
    im = Image.open(out)
    assert im.size == (512, 512) and im.mode == 'RGB' and np.array_equal(np.asarray(im), want['teaser'])
