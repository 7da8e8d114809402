"""A tiny seeded umlvd_ifw tree written with PIL (own code): a few photos and drawings, the 34 clips of 2 frames each, and
every sibling file the dataset reads (landmark maps and txt, the three masks, static drawings, _win.txt).  Sources are
small and not square (300x280, 120x100 ...), so every image is resampled on both axes, up and down."""
import os

import numpy as np

NAME = 'fixture'            # --dataroot: the name of the list files
PHOTOS = [('p0', 300, 280), ('p1', 256, 320), ('p2', 280, 300)]          # name, height, width
DRAWINGS = [('d0', 280, 300), ('d1', 300, 280)]
CLIP_HW = (100, 120)
CLIPS, FRAMES = 34, 2


def _picture(rng, h, w, channels):
    """smooth shading, a few flat shapes, a patch of noise and a 0/255 checker (both clip points of the resampler).  Integer
    arithmetic only: the tree is regenerated where the tests run, and the golden tensors are compared exactly."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
    img = np.zeros((h, w, channels), np.int64)
    for c in range(channels):
        py, px, ph = int(rng.randint(h // 2, 2 * h)), int(rng.randint(w // 2, 2 * w)), int(rng.randint(0, 512))
        ty = np.abs((yy * 512 // py + ph) % 512 - 256)              # triangle waves, 0 .. 256
        tx = np.abs((xx * 512 // px) % 512 - 256)
        img[..., c] = 28 + (ty * tx * 200) // 65536
    for _ in range(4):
        y0, x0 = rng.randint(0, h - 20), rng.randint(0, w - 20)
        img[y0:y0 + rng.randint(8, 40), x0:x0 + rng.randint(8, 40)] = rng.randint(0, 256, channels)
    img[4:20, 4:28] = rng.randint(0, 256, (16, 24, channels))
    img[h - 24:h - 8, 6:30] = ((((yy // 2 + xx // 2) % 2) * 255)[h - 24:h - 8, 6:30])[..., None]
    return np.clip(img, 0, 255).astype(np.uint8)


def _landmarks(rng, h, w):
    gy, gx = np.meshgrid(np.linspace(0.3, 0.8, 9), np.linspace(0.3, 0.7, 8), indexing='ij')
    pts = np.stack([gx.ravel() * w, gy.ravel() * h], 1)[:68]
    return pts + rng.uniform(-0.01 * w, 0.01 * w, (68, 2))


def _save(path, arr):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(arr).save(path)


def _write_face(rng, root, rel, h, w, side, static, window):
    """one photo (side 'A') or drawing / clip frame (side 'B') with everything beside it"""
    top = 'Photo' if side == 'A' else 'Drawing'
    _save(os.path.join(root, top, rel + '.png'), _picture(rng, h, w, 3))
    lm = _landmarks(rng, h, w)
    lm_map = np.zeros((h, w), np.uint8)
    for x, y in lm:
        lm_map[max(0, int(y) - 2):int(y) + 3, max(0, int(x) - 2):int(x) + 3] = 255
    # landmark maps: RGB for photos (converted to L on the way), L for drawings
    _save(os.path.join(root, side + 'lm', 'MTCNN', rel + '.png'), np.repeat(lm_map[..., None], 3, 2) if side == 'A' else lm_map)
    txt = os.path.join(root, side + 'lm_txt', 'MTCNN', rel + '.txt')
    os.makedirs(os.path.dirname(txt), exist_ok=True)
    with open(txt, 'w') as f:
        f.write('\n'.join('%.4f %.4f' % (x, y) for x, y in lm) + '\n')
    for part, (cy, cx) in (('nose', (0.55, 0.5)), ('eyes', (0.4, 0.5)), ('lips', (0.7, 0.5))):
        m = np.zeros((h, w), np.uint8)
        m[int((cy - 0.08) * h):int((cy + 0.08) * h), int((cx - 0.15) * w):int((cx + 0.15) * w)] = 255
        _save(os.path.join(root, side + 'mask', part, rel + '.png'), m)
    if static:
        _save(os.path.join(root, 'fakeB_static', rel + '.png'), _picture(rng, h, w, 3))
    if window is not None:
        with open(txt[:-4] + '_win.txt', 'w') as f:
            f.write('%.2f %.2f %.2f %.2f\n' % window)


def write_tree(root, list_dir, seed=5):
    """Writes the tree under ``root`` and the list files under ``list_dir``; returns (A paths, B paths)."""
    rng = np.random.RandomState(seed)
    for name, h, w in PHOTOS:
        _write_face(rng, root, name, h, w, 'A', True, None)
    for name, h, w in DRAWINGS:
        _write_face(rng, root, 'real/' + name, h, w, 'B', False, None)
    h, w = CLIP_HW
    for c in range(CLIPS):
        for f in range(FRAMES):
            # windows [x1, x2, y1, y2]: most inside the frame, clip 3 past the left edge, clip 7 past the right edge
            x1 = -4.0 if c == 3 else (w * 0.35 if c == 7 else w * 0.2 + f)
            x2 = x1 + w * (0.7 if c == 7 else 0.6)
            y1 = h * 0.2 + f
            _write_face(rng, root, 'scanner_frag_%d_MTCNN/f%d' % (c, f), h, w, 'B', False, (x1, x2, y1, y1 + (x2 - x1)))
    a = [os.path.join(root, 'Photo', n + '.png') for n, _, _ in PHOTOS]
    b = [os.path.join(root, 'Drawing', 'real', n + '.png') for n, _, _ in DRAWINGS]
    for side, paths in (('A', a), ('B', b)):
        d = os.path.join(list_dir, 'train' + side)
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, NAME + '.txt'), 'w') as f:
            f.write('\n'.join(paths) + '\n')
    return a, b


def options(list_dir, **over):
    """the options the dataset reads, at the reference's training defaults (load 286, crop 256, 3 -> 1 channels)"""
    import argparse
    o = dict(dataroot=NAME, list_dir=list_dir, phase='train', isTrain=True, serial_batches=False, max_dataset_size=float('inf'),
             preprocess='resize_and_crop', load_size=286, crop_size=256, no_flip=False, direction='AtoB', input_nc=3,
             output_nc=1, use_mask=1, use_eye_mask=1, use_lip_mask=1, max_offset=3, select_target12_thre=0.2,
             select_noniden_thre=0.9, coh_use_more=2, warp_loss=2, identity_loss=2, batch_size=3, num_threads=4, gpu_ids=[0],
             data_prep='device', cache_decoded=False)
    o.update(over)
    return argparse.Namespace(**o)
