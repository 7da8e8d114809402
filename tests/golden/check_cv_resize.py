#!/usr/bin/env python3
"""One-minute check for a maintainer WITH opencv-python installed -- it is absent from the build image, and pytest does not run
this file: does tests/cv_resize_reference.py (the rule the device's aligned picture is held to) equal
cv2.resize(..., (512, 512), interpolation=cv2.INTER_CUBIC) on the cuts align_photo makes of the two fixture photos, and on
random images across up- and down-scaling?  Until this has printed OK everywhere, the documents say "parity with cv2 itself
unpinned".  (cv2's vectorised vertical pass may round through float; a report of +-1 differences points there.)

    python tests/golden/check_cv_resize.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def main():
    import cv2
    from PIL import Image
    import cv_resize_reference as cvr
    import mtcnn_reference as ref
    cases = []
    with np.load(os.path.join(HERE, 'mtcnn.npz')) as z:
        for name in ('wflw', 'teaser'):
            rgb = np.asarray(Image.open(os.path.join(HERE, 'mtcnn_%s.png' % name)).convert('RGB'))
            cases.append((name, ref.align_cut(rgb, tuple(int(v) for v in z[name + '/align_window'])), 512))
    rng = np.random.RandomState(0)
    for side, out in ((70, 512), (173, 512), (512, 512), (700, 512), (33, 64)):
        cases.append(('random %d -> %d' % (side, out), rng.randint(0, 256, (side, side, 3)).astype(np.uint8), out))
    bad = 0
    for name, a, out in cases:
        want = cv2.resize(a, (out, out), interpolation=cv2.INTER_CUBIC)
        got = cvr.resize_cubic(a, out, out)
        diff = np.abs(want.astype(np.int32) - got.astype(np.int32))
        bad += int(diff.max() > 0)
        print('%-22s %d values differ, max %d %s' % (name, int((diff > 0).sum()), int(diff.max()), 'OK' if diff.max() == 0 else 'MISMATCH'))
    raise SystemExit(1 if bad else 0)


if __name__ == '__main__':
    main()
