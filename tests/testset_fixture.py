"""What the umlvdfw_test tests add to dataset_fixture.py: the test-phase lists of the same tree (one B path of the
'Alm' style, two of the 'Drawing' style), the options test.py runs the dataset with, the fixture copy of
faceLmarkLookup.npy, the rasteriser cases the device and the host check share, and draw2 restated with oracle/cv_raster."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dataset_fixture as fx          # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
LOOKUP = os.path.join(HERE, 'golden', 'faceLmarkLookup.npy')
NAME = fx.NAME
# golden items: (index, draw_op, serial_batches, seed)
ITEMS = [(0, 0, True, 11), (1, 1, True, 12), (2, 1, False, 13)]


def write_test_tree(root, list_dir):
    """the dataset_fixture tree plus <list_dir>/testA|B/<NAME>.txt; returns (A paths, B paths), sorted as the dataset sorts"""
    fx.write_tree(root, list_dir)
    a = sorted(os.path.join(root, 'Photo', n + '.png') for n, _, _ in fx.PHOTOS)
    # B's image is never opened (umlvdfw_test_dataset.py:136): only its landmark txt is read, through the path rules
    b = sorted([os.path.join(root, 'Alm', 'MTCNN', 'p1.png')] + [os.path.join(root, 'Drawing', 'real', n + '.png') for n, _, _ in fx.DRAWINGS])
    for side, paths in (('A', a), ('B', b)):
        d = os.path.join(list_dir, 'test' + side)
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, NAME + '.txt'), 'w') as f:
            f.write('\n'.join(paths) + '\n')
    return a, b


def options(list_dir, **over):
    """what test.py hands the dataset: load 286 / crop 256 (the reference's README command), serial, no flip"""
    o = dict(dataroot=NAME, list_dir=list_dir, phase='test', isTrain=False, serial_batches=True, max_dataset_size=float('inf'),
             preprocess='resize_and_crop', load_size=286, crop_size=256, no_flip=True, direction='AtoB', input_nc=3,
             output_nc=1, batch_size=3, num_threads=4, gpu_ids=[0], data_prep='device', cache_decoded=False, draw_op=0,
             lmark_lookup=LOOKUP)
    o.update(over)
    return argparse.Namespace(**o)


def draw2_reference(lm, segments, height, width, radius, thickness, op):
    """draw2 (umlvdfw_test_dataset.py:34-52) for one sample with the cv_raster rules: (height, width) uint8 in {0, 255}"""
    from oracle import cv_raster
    frame = np.zeros((height, width), np.uint8)
    lands = np.round(np.asarray(lm, dtype=np.float32)).astype(int)
    for x, y in lands:
        cv_raster.fill_circle(frame, int(x), int(y), radius)
    if op == 1:
        for a, b in segments:
            cv_raster.thick_line(frame, (lands[a, 0], lands[a, 1]), (lands[b, 0], lands[b, 1]), thickness)
    return frame


def _chain(p):
    return [(i, i + 1) for i in range(p - 1)]


def raster_cases():
    """name -> (H, W, lm (P, 2) float32, segments (S, 2) int32, radius, thickness): the shapes and the hostile geometry the
    issue lists.  Small on purpose: every path of the rasteriser shows at 32 x 32."""
    cases = {}
    # 32 x 32, P = 6, thickness 2: a horizontal, a vertical and a 45-degree segment, a zero-length one, two identical points
    lm = np.array([[4, 5], [20, 5], [20, 25], [10, 15], [10, 15], [27.4, 8.6]], np.float32)
    seg = np.array([(0, 1), (1, 2), (2, 3), (3, 3), (3, 4), (4, 5)], np.int32)
    cases['square32_t2'] = (32, 32, lm, seg, 3, 2)
    # 40 x 24 (ragged: H 40 is no multiple of the 16-row tile, W 24 none of the wavefront): .5 ties (2.5 -> 2, 3.5 -> 4,
    # 11.5 -> 12, 12.5 -> 12), a point outside, a segment crossing the border, a segment wholly outside
    lm = np.array([[2.5, 3.5], [11.5, 12.5], [20, 30], [30, 36], [-9, 20], [-40, -30], [-25, -60], [5, 38], [18, 7], [60, 200]],
                  np.float32)
    seg = np.array([(0, 1), (1, 2), (2, 3), (3, 4), (5, 6), (7, 8), (6, 9), (8, 8)], np.int32)
    for t in (1, 4, 16):
        cases['ragged40x24_t%d' % t] = (40, 24, lm, seg, 2, t)
    rng = np.random.RandomState(3)
    lm = (rng.uniform(-6, 38, (12, 2))).astype(np.float32)
    cases['s0'] = (32, 32, lm, np.zeros((0, 2), np.int32), 3, 2)
    cases['s1'] = (32, 32, lm, np.array([(0, 11)], np.int32), 3, 2)
    cases['s128'] = (32, 32, lm, rng.randint(0, 12, (128, 2)).astype(np.int32), 1, 3)
    # many directions and lengths, odd and even thickness: the slopes of both scanline chains and of all four outline runs
    lm = (rng.uniform(-10, 70, (40, 2))).astype(np.float32)
    for t in (2, 5):
        cases['random64x48_t%d' % t] = (64, 48, lm, rng.randint(0, 40, (48, 2)).astype(np.int32), 2, t)
    return cases
