"""A tiny seeded umlvd_ifw_cartoon tree written with PIL (own code), beside dataset_fixture.py and from its picture / landmark
helpers: a few photos under Photo/, a few RGB cartoons under Cartoon/, and every sibling file the cartoon dataset reads -- landmark
maps and txt, the three masks, and the static cartoons under fakeB5_static/.  No scanner_frag_* clips: the cartoon data has none."""
import os

import numpy as np

import dataset_fixture as fx

NAME = 'cartoon_fixture'    # --dataroot: the name of the list files
PHOTOS = [('p0', 300, 280), ('p1', 256, 320), ('p2', 280, 300)]          # name, height, width
CARTOONS = [('c0', 280, 300), ('c1', 300, 280), ('c2', 264, 272)]


def _write_face(rng, root, rel, h, w, side):
    """one photo (side 'A', with its static cartoon) or cartoon (side 'B') with everything beside it"""
    top = 'Photo' if side == 'A' else 'Cartoon'
    fx._save(os.path.join(root, top, rel + '.png'), fx._picture(rng, h, w, 3))
    lm = fx._landmarks(rng, h, w)
    lm_map = np.zeros((h, w), np.uint8)
    for x, y in lm:
        lm_map[max(0, int(y) - 2):int(y) + 3, max(0, int(x) - 2):int(x) + 3] = 255
    fx._save(os.path.join(root, side + 'lm', 'MTCNN', rel + '.png'), np.repeat(lm_map[..., None], 3, 2) if side == 'A' else lm_map)
    txt = os.path.join(root, side + 'lm_txt', 'MTCNN', rel + '.txt')
    os.makedirs(os.path.dirname(txt), exist_ok=True)
    with open(txt, 'w') as f:
        f.write('\n'.join('%.4f %.4f' % (x, y) for x, y in lm) + '\n')
    for part, (cy, cx) in (('nose', (0.55, 0.5)), ('eyes', (0.4, 0.5)), ('lips', (0.7, 0.5))):
        m = np.zeros((h, w), np.uint8)
        m[int((cy - 0.08) * h):int((cy + 0.08) * h), int((cx - 0.15) * w):int((cx + 0.15) * w)] = 255
        fx._save(os.path.join(root, side + 'mask', part, rel + '.png'), m)
    if side == 'A':
        fx._save(os.path.join(root, 'fakeB5_static', rel + '.png'), fx._picture(rng, h, w, 3))


def write_tree(root, list_dir, seed=9):
    """Writes the tree under ``root`` and the list files under ``list_dir``; returns (A paths, B paths)."""
    rng = np.random.RandomState(seed)
    for name, h, w in PHOTOS:
        _write_face(rng, root, name, h, w, 'A')
    for name, h, w in CARTOONS:
        _write_face(rng, root, 'real/' + name, h, w, 'B')
    a = [os.path.join(root, 'Photo', n + '.png') for n, _, _ in PHOTOS]
    b = [os.path.join(root, 'Cartoon', 'real', n + '.png') for n, _, _ in CARTOONS]
    for side, paths in (('A', a), ('B', b)):
        d = os.path.join(list_dir, 'train' + side)
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, NAME + '.txt'), 'w') as f:
            f.write('\n'.join(paths) + '\n')
    return a, b


def options(list_dir, **over):
    """the options the cartoon dataset reads, at the cartoon model's training defaults (load 286, crop 256, 3 -> 3 channels, no
    coherence discriminator)"""
    o = dict(dataroot=NAME, output_nc=3, coherent=0, coh_use_more=0, batch_size=2)
    o.update(over)
    opt = fx.options(list_dir, **o)
    del opt.select_target12_thre        # the cartoon model never registers it
    return opt
