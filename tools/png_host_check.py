#!/usr/bin/env python3
"""Builds tools/png_host_check.cpp (the PNG encoder of apd_png_encode compiled for the host from png_deflate.h) with
-fsanitize=address,undefined, runs the images of tests/png_fixture.py through it and decodes every file with the
independent decoder of that module and with PIL; prints each file's size beside PIL's own.

    python tools/png_host_check.py [--cxx g++]
"""
import argparse
import io
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def build(work, cxx='g++'):
    exe = os.path.join(work, 'png_host_check')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           os.path.join(ROOT, 'tools', 'png_host_check.cpp'), '-o', exe])
    return exe


def encode(exe, work, images):
    """[(H, W, channels) uint8] -> [(file bytes, bound)] by the host program"""
    cases, out = os.path.join(work, 'cases.bin'), os.path.join(work, 'out.bin')
    with open(cases, 'wb') as f:
        for im in images:
            f.write(np.array(im.shape, np.int32).tobytes())
            f.write(np.ascontiguousarray(im).tobytes())
    subprocess.check_call([exe, cases, out])
    blob = open(out, 'rb').read()
    at, files = 0, []
    for _ in images:
        size, bound = np.frombuffer(blob[at:at + 8], np.int32)
        files.append((blob[at + 8:at + 8 + size], int(bound)))
        at += 8 + int(size)
    assert at == len(blob)
    return files


def main():
    import png_fixture as pf
    from PIL import Image
    ap = argparse.ArgumentParser()
    ap.add_argument('--cxx', default='g++')
    args = ap.parse_args()
    work = tempfile.mkdtemp()
    exe = build(work, args.cxx)
    cases = pf.images()
    names = sorted(cases)
    bad = 0
    for name, (data, bound) in zip(names, encode(exe, work, [cases[n] for n in names])):
        im = cases[name]
        try:
            pf.check_both(data, im)
            verdict = 'equal'
        except AssertionError as e:
            verdict, bad = 'FAILED: %s' % e, bad + 1
        ref = io.BytesIO()
        Image.fromarray(im if im.shape[2] == 3 else im[:, :, 0]).save(ref, format='PNG')
        print('%-18s %4d x %4d x %d: %7d bytes (bound %7d, raw %7d, PIL %7d)  %s'
              % (name, im.shape[0], im.shape[1], im.shape[2], len(data), bound, im.size, len(ref.getvalue()), verdict))
        if len(data) > bound:
            bad += 1
            print('  beyond its bound')
    print('FAILED' if bad else 'all files decode to their images')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
