#!/usr/bin/env python3
"""Builds tools/raster_host_check.cpp (the predicates of apd_landmark_map compiled for the host) with
-fsanitize=address,undefined, runs the rasteriser cases of tests/testset_fixture.py -- and the 64-segment table on the
fixture landmarks at 256 x 256 -- through it and compares every map with draw2 restated on oracle/cv_raster.

    python tools/raster_host_check.py [--cxx g++]
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    import testset_fixture as tf
    ap = argparse.ArgumentParser()
    ap.add_argument('--cxx', default='g++')
    args = ap.parse_args()
    work = tempfile.mkdtemp()
    exe = os.path.join(work, 'raster_host_check')
    subprocess.check_call([args.cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-ffp-contract=off', os.path.join(ROOT, 'tools', 'raster_host_check.cpp'), '-o', exe])
    cases = dict(tf.raster_cases())
    rng = np.random.RandomState(1)
    lm = np.stack([np.linspace(60, 200, 68) + rng.uniform(-20, 20, 68), 128 + 70 * np.sin(np.arange(68)) + rng.uniform(-5, 5, 68)], 1)
    cases['table256'] = (256, 256, lm.astype(np.float32), np.load(tf.LOOKUP).astype(np.int32), 3, 2)
    cases['table512'] = (512, 512, (2 * lm).astype(np.float32), np.load(tf.LOOKUP).astype(np.int32), 5, 4)
    runs = [(name, op) + c for name, c in sorted(cases.items()) for op in (0, 1)]
    with open(os.path.join(work, 'cases.bin'), 'wb') as f:
        for name, op, h, w, pts, seg, radius, thickness in runs:
            f.write(np.array([h, w, len(pts), len(seg), radius, thickness, op], np.int32).tobytes())
            f.write(np.ascontiguousarray(pts, np.float32).tobytes())
            f.write(np.ascontiguousarray(seg, np.int32).tobytes())
    subprocess.check_call([exe, os.path.join(work, 'cases.bin'), os.path.join(work, 'maps.bin')])
    got = np.fromfile(os.path.join(work, 'maps.bin'), np.uint8)
    at, bad = 0, 0
    for name, op, h, w, pts, seg, radius, thickness in runs:
        g = got[at:at + h * w].reshape(h, w)
        at += h * w
        want = tf.draw2_reference(pts, seg, h, w, radius, thickness, op) > 0
        diff = int((g.astype(bool) != want).sum())
        bad += diff
        print('%-22s op %d: %5d marked, %d pixels differ' % (name, op, int(want.sum()), diff))
    assert at == got.size
    print('FAILED' if bad else 'all maps equal')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
