#!/usr/bin/env python3
"""Builds tools/jpeg_host_check.cpp (the JPEG encoder of apd_jpeg_encode compiled for the host from jpeg_core.h) with
-fsanitize=address,undefined, runs the images of tests/jpeg_fixture.py through it, walks every file's markers, decodes it
with PIL and compares its error with that of PIL's own encoder at the same tables.

    python tools/jpeg_host_check.py [--cxx g++]          the golden cases: every image at quality 90, noise at 1, 50, 100
    python tools/jpeg_host_check.py --measure            every image at 50, 90 and 100: the shortfall table of DESIGN.md
    python tools/jpeg_host_check.py --write-golden       store the golden cases' bytes as tests/golden/jpeg_host.npz
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
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'jpeg_host.npz')


def build(work, cxx='g++'):
    exe = os.path.join(work, 'jpeg_host_check')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           os.path.join(ROOT, 'tools', 'jpeg_host_check.cpp'), '-o', exe])
    return exe


def encode(exe, work, cases):
    """[((H, W, channels) uint8, quality)] -> [(file bytes, bound)] by the host program"""
    src, out = os.path.join(work, 'cases.bin'), os.path.join(work, 'out.bin')
    with open(src, 'wb') as f:
        for im, quality in cases:
            f.write(np.array(im.shape + (quality,), np.int32).tobytes())
            f.write(np.ascontiguousarray(im).tobytes())
    subprocess.check_call([exe, src, out])
    blob = open(out, 'rb').read()
    at, files = 0, []
    for _ in cases:
        size, bound = np.frombuffer(blob[at:at + 8], np.int32)
        files.append((blob[at + 8:at + 8 + size], int(bound)))
        at += 8 + int(size)
    assert at == len(blob)
    return files


def main():
    import jpeg_fixture as jf
    ap = argparse.ArgumentParser()
    ap.add_argument('--cxx', default='g++')
    ap.add_argument('--measure', action='store_true')
    ap.add_argument('--write-golden', action='store_true')
    args = ap.parse_args()
    work = tempfile.mkdtemp()
    exe = build(work, args.cxx)
    images = jf.images()
    cases = [(n, q) for n in sorted(images) for q in (50, 90, 100)] if args.measure else jf.golden_cases()
    files = encode(exe, work, [(images[n], q) for n, q in cases])
    bad, short, excess = 0, -1e9, -10 ** 9
    for (name, quality), (data, bound) in zip(cases, files):
        im = images[name]
        try:
            psnr, worst, ref_psnr, ref_worst = jf.measure(data, im, quality) if args.measure else jf.check_file(data, im, quality)
            verdict = 'within bounds'
            short, excess = max(short, ref_psnr - psnr), max(excess, worst - ref_worst)
        except AssertionError as e:
            psnr = worst = ref_psnr = ref_worst = float('nan')
            verdict, bad = 'FAILED: %s' % e, bad + 1
        print('%-16s q%-3d %4d x %4d x %d: %7d bytes (bound %8d, PIL %7d)  PSNR %6.3f dB (PIL %6.3f)  max error %3s (PIL %3s)  %s'
              % (name, quality, im.shape[0], im.shape[1], im.shape[2], len(data), bound, len(jf.pil_file(im, quality)), psnr,
                 ref_psnr, worst, ref_worst, verdict))
        if len(data) > bound:
            bad += 1
            print('  beyond its bound')
    print('worst PSNR shortfall against PIL %.3f dB, worst max-error excess %d' % (short, excess))
    if args.write_golden and not bad:
        np.savez_compressed(GOLDEN, **{jf.key(n, q): np.frombuffer(data, np.uint8) for (n, q), (data, _) in zip(cases, files)})
        print('wrote %s: %d bytes' % (GOLDEN, os.path.getsize(GOLDEN)))
    print('FAILED' if bad else 'every file decodes within bounds')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
