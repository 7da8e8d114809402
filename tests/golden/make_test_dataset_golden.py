#!/usr/bin/env python3
"""Golden items of the umlvdfw_test dataset from the REFERENCE's own ``UMLVDFWTestDataset.__getitem__``
(Module2/data/umlvdfw_test_dataset.py:114-167), imported read-only and run on the tree tests/testset_fixture.py writes, at
load 286 / crop 256, from a working directory that holds the fixture copy of faceLmarkLookup.npy (the reference loads it
at import).  Import-time stubs as in make_dataset_golden.py (PIL-backed torchvision.transforms, cv2.circle ->
oracle.cv_raster.fill_circle, np.int) plus ``cv2.line`` -> oracle.cv_raster.thick_line, which returns the frame.

So ``draw2`` is pinned only as far as oracle/cv_raster.py restates OpenCV 4.2 -- the same disclosed gap as for the discs:
cv2 cannot be imported here, and tests/golden/check_opencv_rules.py is the check a maintainer with opencv-python runs.

Three items (testset_fixture.ITEMS): draw_op 0 and 1, a B path of the 'Alm' style (item 0) and of the 'Drawing' style,
--serial_batches on and off under fixed seeds (the item without it also flips).  Recorded per item: paths relative to the
tree, B's index, the (x, y, flip) of both get_params2 calls, landmarks and window, image_paths, A and both landmark maps as
the uint8 they hold (checked lossless), warp_motion and realA_static_warp at every 4th pixel.

    python tests/golden/make_test_dataset_golden.py          (build container only)
"""
import os
import random
import shutil
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
REF = '/root/reference/Module2'
STEP = 4


def main():
    import make_dataset_golden as base
    import testset_fixture as tf
    from animateportrait_amd.data import image_prep
    from oracle import cv_raster
    base._torchvision_stub()
    base._cv2_stub()

    def line(img, p0, p1, color, thickness):
        return cv_raster.thick_line(img, (int(p0[0]), int(p0[1])), (int(p1[0]), int(p1[1])), thickness, color)
    sys.modules['cv2'].line = line
    if not hasattr(np, 'int'):
        np.int = int

    work = tempfile.mkdtemp()
    root = os.path.join(work, 'tree')
    tf.write_test_tree(root, os.path.join(work, 'datasets', 'list'))
    shutil.copy(tf.LOOKUP, os.path.join(work, 'faceLmarkLookup.npy'))
    os.chdir(work)                                   # the lists and the lookup table are read relative to the working directory
    sys.path.insert(0, REF)
    import data.umlvdfw_test_dataset as ref
    calls = []

    def recording(fn):
        def wrapped(*a, **k):
            out = fn(*a, **k)
            calls.append((int(out['crop_pos'][0]), int(out['crop_pos'][1]), int(out['flip'])))
            return out
        return wrapped
    ref.get_params2 = recording(ref.get_params2)
    lut = image_prep.lut('image')
    out = {'step': np.array(STEP), 'items': np.array(tf.ITEMS, dtype=np.int64)}
    for s, (index, draw_op, serial, seed) in enumerate(tf.ITEMS):
        opt = tf.options(os.path.join(work, 'datasets', 'list'), draw_op=draw_op, serial_batches=bool(serial), no_flip=bool(serial))
        ds = ref.UMLVDFWTestDataset(opt)
        random.seed(seed)
        torch.manual_seed(seed)
        del calls[:]
        it = ds[index]
        assert len(calls) == 2
        out['params_%d' % s] = np.array(calls, dtype=np.int32)                 # rows: A, B -- (x, y, flip)
        out['paths_%d' % s] = np.array([os.path.relpath(it[k], root) for k in ('A_paths', 'B_paths')])
        out['index_B_%d' % s] = np.array(ds.B_paths.index(it['B_paths']))
        out['image_paths_%d' % s] = np.array(it['image_paths'])
        out['winB_%d' % s] = it['winB'].numpy()
        for k in ('A_lm_68', 'tB_lm_68'):
            out['%s_%d' % (k, s)] = it[k].numpy().astype(np.float32)
        for k in ('A', 'A_lm', 'B_lm', 'tB_lm'):
            t = it[k].float()
            u8 = torch.round((t * 0.5 + 0.5) * 255).clamp(0, 255).to(torch.uint8)
            assert torch.equal(lut[u8.long()], t), k                            # lossless: the tensor is the table of its bytes
            out['%s_u8_%d' % (k, s)] = u8.numpy()
        out['warp_motion_%d' % s] = it['warp_motion'].numpy().astype(np.float32)[::STEP, ::STEP]
        out['realA_static_warp_%d' % s] = it['realA_static_warp'].numpy().astype(np.float32)[:, ::STEP, ::STEP]
        print('item %d: %s  B index %d  params %s  marked %d / %d' % (s, it['image_paths'], int(out['index_B_%d' % s]), calls,
                                                                      int((it['A_lm'] > 0).sum()), int((it['B_lm'] > 0).sum())))
    path = os.path.join(HERE, 'test_dataset.npz')
    np.savez_compressed(path, **out)
    print('test_dataset.npz %.1f KB' % (os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
