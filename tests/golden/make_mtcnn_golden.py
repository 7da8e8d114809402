#!/usr/bin/env python3
"""Record the reference's MTCNN detector stage by stage: tests/golden/mtcnn.npz, mtcnn_aligned.npz, the three fixture
photos and the weights re-saved without pickle (mtcnn_weights/*.npz).  Needs the reference checkout:

    python tests/golden/make_mtcnn_golden.py /path/to/reference

The stages are driven from here with the reference's own functions (MTCNN.first_stage, MTCNN.box_utils, MTCNN.get_nets), so
that every intermediate can be kept; the final boxes and landmarks are asserted equal to what MTCNN.detector returns.  The
script fails when a fixture sits closer than 1e-3 (the project's parity budget) to a decision: a score to its threshold, an
overlap to its NMS threshold, a rounded value to a half-integer, or when two scores meeting in an NMS are equal."""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
MARGIN = 1e-3
PART_BYTES = 900 * 1024            # committed files stay below 1 MiB


def check_threshold(what, scores, thr):
    d = np.abs(np.asarray(scores, np.float64) - thr)
    assert d.size == 0 or d.min() > MARGIN, '%s: a score lies %.2e from its threshold %g' % (what, d.min(), thr)


def check_round(what, values):
    v = np.asarray(values, np.float64)
    d = np.abs(v - np.floor(v) - 0.5)
    assert d.size == 0 or d.min() > MARGIN, '%s: a rounded value lies %.2e from a half-integer' % (what, d.min())


def check_nms(what, boxes, thr, mode):
    import mtcnn_reference as ref
    n = len(boxes)
    assert len(np.unique(boxes[:, 4])) == n, '%s: equal scores meet in an NMS' % what
    if np.array_equal(boxes[:, 0:4], np.round(boxes[:, 0:4])) and np.abs(boxes[:, 0:4]).max() < 2 ** 20:
        # Corners that are integers (every NMS but the last: they come out of np.round) make areas and intersections exact
        # integers in float64, and the one division is correctly rounded: the overlap is the same bits on every IEEE-754
        # machine, so no margin is at stake.  Overlaps of exactly 1/2 are common here (two 21 x 21 windows 7 px apart).
        return
    worst = 1.0                      # over the pairs the greedy sweep evaluates: a picked box against every box still alive
    order = sorted(range(n), key=lambda i: (boxes[i, 4], i))
    alive = [True] * n
    for r in range(n - 1, -1, -1):
        if not alive[r]:
            continue
        for q in range(r):
            if alive[q]:
                o = ref.overlap(boxes[order[r]], boxes[order[q]], mode)
                worst = min(worst, abs(o - thr))
                alive[q] = o <= thr
    assert worst > MARGIN, '%s: an overlap lies %.2e from its threshold %g' % (what, worst, thr)


def save_weights(src_dir, out_dir):
    """the three pickled dicts as plain float32 arrays, keys net/parameter; a tensor too large for one committed file is
    split along axis 0 into keys name@0, name@1, ... (animateportrait_amd.mtcnn.load_weights joins them)"""
    os.makedirs(out_dir, exist_ok=True)
    for net in ('pnet', 'rnet', 'onet'):
        w = np.load(os.path.join(src_dir, net + '.npy'), allow_pickle=True)[()]
        parts, cur, size = [], {}, 0
        for name, a in w.items():
            a = np.ascontiguousarray(a, np.float32)
            pieces = [a] if a.nbytes <= PART_BYTES else np.array_split(a, math.ceil(a.nbytes / PART_BYTES), axis=0)
            for k, p in enumerate(pieces):
                key = '%s/%s' % (net, name) + ('@%d' % k if len(pieces) > 1 else '')
                if size + p.nbytes > PART_BYTES and cur:
                    parts.append(cur)
                    cur, size = {}, 0
                cur[key] = p
                size += p.nbytes
        parts.append(cur)
        for k, part in enumerate(parts):
            np.savez(os.path.join(out_dir, '%s_%d.npz' % (net, k)), **part)


def record(name, rgb, det, out):
    """one image through the reference's stages; every intermediate into out[name/...]"""
    import torch
    from PIL import Image
    from MTCNN.box_utils import nms, calibrate_box, convert_to_square, get_image_boxes, _preprocess
    from MTCNN.first_stage import _generate_bboxes
    import mtcnn_reference as ref
    import cv_resize_reference as cvr

    image = Image.fromarray(rgb)
    W, H = image.size
    thr, nthr = ref.THRESHOLDS, ref.NMS_THRESHOLDS
    put = lambda k, v: out.__setitem__('%s/%s' % (name, k), np.asarray(v))
    nets64 = {k: __import__('copy').deepcopy(n).double() for k, n in (('p', det.pnet), ('r', det.rnet), ('o', det.onet))}
    nets64['o'].eval()
    e_ref = {'p': 0.0, 'r': 0.0, 'o': 0.0}

    def run(key, net, x):
        with torch.no_grad():
            y32 = [t.numpy() for t in net(torch.from_numpy(x))]
            y64 = [t.numpy() for t in nets64[key](torch.from_numpy(x).double())]
        e_ref[key] = max([e_ref[key]] + [float(np.abs(a - b).max()) for a, b in zip(y32, y64) if a.size])
        return y32, y64

    scales = ref.scales(W, H)
    put('scales', np.asarray(scales, np.float64))
    sizes, levels = [], []
    for k, s in enumerate(scales):
        sw, sh = math.ceil(W * s), math.ceil(H * s)
        sizes.append((sh, sw))
        lvl = np.asarray(image.resize((sw, sh), Image.BILINEAR), 'uint8')
        (off, prob), (off64, prob64) = run('p', det.pnet, _preprocess(np.asarray(lvl, 'float32')).astype(np.float32))
        put('L%d/prob' % k, prob[0, 1])
        put('L%d/off' % k, off[0])
        put('L%d/prob64' % k, prob64[0, 1])
        put('L%d/off64' % k, off64[0])
        check_threshold('%s level %d' % (name, k), prob[0, 1], thr[0])
        cand = _generate_bboxes(prob[0, 1], off, s, thr[0])
        cand = cand.reshape(-1, 9)
        put('L%d/cand' % k, cand)
        if len(cand):
            iy, ix = np.nonzero(prob[0, 1] > thr[0])
            for q in ((2 * ix + 1.0) / s, (2 * iy + 1.0) / s, (2 * ix + 13.0) / s, (2 * iy + 13.0) / s):
                check_round('%s level %d' % (name, k), q)
            check_nms('%s level %d' % (name, k), cand, ref.LEVEL_NMS, 'union')
            keep = nms(cand[:, 0:5], overlap_threshold=ref.LEVEL_NMS)
            put('L%d/pick' % k, np.asarray(keep, np.int64))
            levels.append(cand[keep])
        else:
            put('L%d/pick' % k, np.zeros(0, np.int64))
    put('sizes', np.asarray(sizes, np.int64))

    def finish(boxes, lm):
        put('boxes', np.asarray(boxes, np.float64).reshape(-1, 5))
        put('landmarks', np.asarray(lm, np.float32).reshape(-1, 10))
        win = ref.align_window(out[name + '/boxes'])
        put('align_window', np.asarray(win if win else (0, 0, 0), np.int64))
        if win:
            out['aligned'][name] = cvr.resize_cubic(ref.align_cut(rgb, win), 512, 512)

    if not levels:
        finish(np.zeros((0, 5)), np.zeros((0, 10)))
        return e_ref
    b = np.vstack(levels)
    put('s1/merged', b)
    check_nms(name + ' stage 1', b, nthr[0], 'union')
    keep = nms(b[:, 0:5], nthr[0])
    put('s1/pick', np.asarray(keep, np.int64))
    b = b[keep]
    b = calibrate_box(b[:, 0:5], b[:, 5:])
    put('s1/cal', b.copy())
    b = convert_to_square(b)
    put('s1/sq', b.copy())
    check_round(name + ' stage 1', b[:, 0:4])
    b[:, 0:4] = np.round(b[:, 0:4])
    put('s1/round', b.copy())

    cut = get_image_boxes(b, image, size=24)                          # clips b to the image as a side effect
    put('s1/clipped', b.copy())
    cut8 = np.rint(cut / 0.0078125 + 127.5).astype(np.uint8).transpose(0, 2, 3, 1)
    assert np.array_equal(((cut8.astype(np.float32) - 127.5) * 0.0078125).transpose(0, 3, 1, 2), cut)
    put('s2/cut', cut8)
    (off, prob), (off64, prob64) = run('r', det.rnet, cut)
    for k, v in (('off', off), ('prob', prob), ('off64', off64), ('prob64', prob64)):
        put('s2/' + k, v)
    check_threshold(name + ' R-Net', prob[:, 1], thr[1])
    keep = np.where(prob[:, 1] > thr[1])[0]
    b = b[keep]
    b[:, 4] = prob[keep, 1].reshape((-1,))
    off = off[keep]
    put('s2/filtered', b.copy())
    check_nms(name + ' stage 2', b, nthr[1], 'union')
    keep = nms(b, nthr[1])
    put('s2/pick', np.asarray(keep, np.int64))
    b = b[keep]
    b = calibrate_box(b, off[keep])
    put('s2/cal', b.copy())
    b = convert_to_square(b)
    put('s2/sq', b.copy())
    check_round(name + ' stage 2', b[:, 0:4])
    b[:, 0:4] = np.round(b[:, 0:4])
    put('s2/round', b.copy())

    cut = get_image_boxes(b, image, size=48)
    put('s2/clipped', b.copy())
    if len(cut) == 0:
        finish(np.zeros((0, 5)), np.zeros((0, 10)))
        return e_ref
    put('s3/cut', np.rint(cut / 0.0078125 + 127.5).astype(np.uint8).transpose(0, 2, 3, 1))
    (lm, off, prob), (lm64, off64, prob64) = run('o', det.onet, cut)
    for k, v in (('lm', lm), ('off', off), ('prob', prob), ('lm64', lm64), ('off64', off64), ('prob64', prob64)):
        put('s3/' + k, v)
    check_threshold(name + ' O-Net', prob[:, 1], thr[2])
    keep = np.where(prob[:, 1] > thr[2])[0]
    b = b[keep]
    b[:, 4] = prob[keep, 1].reshape((-1,))
    off = off[keep]
    lm = lm[keep]
    width = b[:, 2] - b[:, 0] + 1.0
    height = b[:, 3] - b[:, 1] + 1.0
    lm[:, 0:5] = np.expand_dims(b[:, 0], 1) + np.expand_dims(width, 1) * lm[:, 0:5]
    lm[:, 5:10] = np.expand_dims(b[:, 1], 1) + np.expand_dims(height, 1) * lm[:, 5:10]
    b = calibrate_box(b, off)
    put('s3/cal', b.copy())
    check_nms(name + ' stage 3', b, nthr[2], 'min')
    keep = nms(b, nthr[2], mode='min')
    put('s3/pick', np.asarray(keep, np.int64))
    finish(b[keep], lm[keep])
    return e_ref


def main():
    from PIL import Image
    refdir = os.path.abspath(sys.argv[1])
    os.chdir(refdir)                                   # the reference loads MTCNN/weights/*.npy by relative path
    sys.path.insert(0, refdir)
    from MTCNN import detector
    det = detector()

    wflw = Image.open('Module1/thirdparty/AdaptiveWingLoss/images/wflw.png').convert('RGB')
    teaser = Image.open('Module1/thirdparty/face_of_art/old/teaser.png').convert('RGB')
    rng = np.random.RandomState(5)
    images = {
        # crops chosen so that the conditions above hold (the uncropped 2979 x 996 photo and the crop at (0, 0) of the
        # teaser each put a P-Net score within 1e-3 of the threshold)
        'wflw': np.asarray(wflw.crop((12, 0, 2952, 974)).resize((320, 106), Image.BILINEAR)),
        'teaser': np.asarray(teaser.crop((4, 0, 484, 480)).resize((160, 160), Image.BILINEAR)),
        'blank': np.clip(128 + rng.randint(-3, 4, (48, 64, 3)), 0, 255).astype(np.uint8),
    }
    out = {'aligned': {}}
    e_ref = {'p': 0.0, 'r': 0.0, 'o': 0.0}
    for name, rgb in images.items():
        Image.fromarray(rgb).save(os.path.join(HERE, 'mtcnn_%s.png' % name))
        e = record(name, rgb, det, out)
        e_ref = {k: max(e_ref[k], e[k]) for k in e_ref}
        n = len(out[name + '/boxes'])
        if name == 'blank':
            assert n == 0
        else:
            boxes, lm = det(Image.fromarray(rgb))
            assert np.array_equal(boxes, out[name + '/boxes']) and np.array_equal(lm, out[name + '/landmarks'])
        print('%-7s %d faces' % (name, n))
    aligned = out.pop('aligned')
    out['e_ref_pnet'], out['e_ref_rnet'], out['e_ref_onet'] = (np.float64(e_ref[k]) for k in 'pro')
    print('e_ref', e_ref)
    np.savez_compressed(os.path.join(HERE, 'mtcnn.npz'), **out)
    np.savez_compressed(os.path.join(HERE, 'mtcnn_aligned.npz'), **aligned)
    save_weights(os.path.join(refdir, 'MTCNN', 'weights'), os.path.join(HERE, 'mtcnn_weights'))


if __name__ == '__main__':
    main()
