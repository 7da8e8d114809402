#!/usr/bin/env python3
"""Builds tools/landmark_vis_host_check.cpp (the per-pixel rule of apd_landmark_vis compiled for the host) with
-fsanitize=address,undefined, draws every frame of tests/landmark_vis_reference.cases() through it and compares each
picture, byte for byte, with the composition of oracle/cv_raster primitives in that file.

    python tools/landmark_vis_host_check.py [--cxx g++]
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


def build(work, cxx='g++'):
    exe = os.path.join(work, 'landmark_vis_host_check')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-ffp-contract=off', os.path.join(ROOT, 'tools', 'landmark_vis_host_check.cpp'), '-o', exe])
    return exe


def run(exe, work, cases):
    """cases: name -> a tuple of landmark_vis_reference.cases() -> name -> (N, H, W, 3) uint8 from the host program"""
    names = sorted(cases)
    with open(os.path.join(work, 'frames.bin'), 'wb') as f:
        for name in names:
            h, w, pts, seg, rgb, radius, thickness, disc_rgb, bg_rgb = cases[name]
            for frame in pts:
                f.write(np.array([h, w, frame.shape[0], len(seg), radius, thickness], np.int32).tobytes())
                f.write(np.array([disc_rgb, bg_rgb], np.uint32).tobytes())
                f.write(np.ascontiguousarray(frame, np.int32).tobytes())
                f.write(np.ascontiguousarray(seg, np.int32).tobytes())
                f.write(np.ascontiguousarray(rgb, np.uint32).tobytes())
    subprocess.check_call([exe, os.path.join(work, 'frames.bin'), os.path.join(work, 'pictures.bin')])
    got = np.fromfile(os.path.join(work, 'pictures.bin'), np.uint8)
    out, at = {}, 0
    for name in names:
        h, w, pts = cases[name][:3]
        count = pts.shape[0] * h * w * 3
        out[name] = got[at:at + count].reshape(pts.shape[0], h, w, 3)
        at += count
    assert at == got.size
    return out


def compare(cases, got, expected):
    """prints one line per case; returns the number of differing pixels"""
    bad = 0
    for name in sorted(cases):
        want = expected[name]
        diff = int((got[name] != want).any(-1).sum())
        bad += diff
        drawn = int((want != want[0, 0, 0]).any(-1).sum())
        print('%-18s %d frames %4d x %4d: %6d pixels off the corner colour, %d pixels differ' %
              ((name, want.shape[0]) + want.shape[1:3] + (drawn, diff)))
    return bad


def main():
    import landmark_vis_reference as ref
    ap = argparse.ArgumentParser()
    ap.add_argument('--cxx', default='g++')
    args = ap.parse_args()
    work = tempfile.mkdtemp()
    cases = ref.cases()
    bad = compare(cases, run(build(work, args.cxx), work, cases), {name: ref.expected(c) for name, c in cases.items()})
    print('FAILED' if bad else 'all pictures equal')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
