"""Align a photo the way the reference's end-to-end driver does (align_mtcnn, main_end2end_module2.py:12-45): detect the
faces with MTCNN on the device, cut the white-padded square about the largest one, resize it to 512 x 512.

    python -m animateportrait_amd.align --photo IN --out ori.png [--mtcnn_weights DIR]

IN is a file, or a directory: then OUT is a directory too and every image of IN is written there under its name as a PNG.
A photo without a face is an error."""
import argparse
import os

import numpy as np

from . import mtcnn

EXTENSIONS = ('.png', '.jpg', '.jpeg', '.bmp')


def align_file(detector, src, dst, size=512):
    from PIL import Image
    image = np.asarray(Image.open(src).convert('RGB'))
    aligned = detector.align_photo(image, size)
    if aligned is None:
        raise SystemExit('align: MTCNN finds no face in %s' % src)
    if os.path.dirname(dst):
        os.makedirs(os.path.dirname(dst), exist_ok=True)
    Image.fromarray(aligned).save(dst)
    return dst


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--photo', required=True, help='an image, or a directory of images')
    ap.add_argument('--out', required=True, help='the aligned PNG (a directory when --photo is one)')
    ap.add_argument('--mtcnn_weights', default=mtcnn.DEFAULT_WEIGHTS, help='directory with pnet.npy / rnet.npy / onet.npy, or .npz')
    ap.add_argument('--size', type=int, default=512)
    a = ap.parse_args(argv)
    detector = mtcnn.Detector(a.mtcnn_weights)
    if os.path.isdir(a.photo):
        names = sorted(n for n in os.listdir(a.photo) if n.lower().endswith(EXTENSIONS))
        if not names:
            raise SystemExit('align: no image in %s' % a.photo)
        for n in names:
            print('wrote', align_file(detector, os.path.join(a.photo, n), os.path.join(a.out, os.path.splitext(n)[0] + '.png'), a.size))
    else:
        print('wrote', align_file(detector, a.photo, a.out, a.size))


if __name__ == '__main__':
    main()
