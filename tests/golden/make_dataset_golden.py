#!/usr/bin/env python3
"""Golden items of the umlvd_ifw dataset from the REFERENCE's own ``UMLVDIFWDataset.__getitem__``
(Module2/data/umlvd_ifw_dataset.py:149-428), imported read-only and run on the tree tests/dataset_fixture.py writes, at
load 286 / crop 256.  Import-time stubs for what this image lacks: a PIL-backed minimal ``torchvision.transforms`` (own
code: the five transforms get_transform composes), ``cv2.circle`` -> oracle.cv_raster.fill_circle, ``np.int = int``.

Recorded per sample (seeds chosen so that the three target branches occur): the decisions (paths relative to the tree,
crop / flip of the three get_params calls, branch), the image tensors as the uint8 they hold before ToTensor / Normalize
(checked lossless here), landmarks and windows, and the float maps at every 4th pixel.

    python tests/golden/make_dataset_golden.py          (build container only)
"""
import os
import random
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
REF = '/root/reference/Module2'
STEP = 4


def _torchvision_stub():
    tv, tr = types.ModuleType('torchvision'), types.ModuleType('torchvision.transforms')

    class Compose:
        def __init__(self, ts):
            self.ts = ts

        def __call__(self, x):
            for t in self.ts:
                x = t(x)
            return x

    class Lambda:
        def __init__(self, fn):
            self.fn = fn

        def __call__(self, x):
            return self.fn(x)

    class Grayscale:
        def __init__(self, n=1):
            assert n == 1

        def __call__(self, img):
            return img.convert('L')

    class Resize:
        def __init__(self, size, method):
            self.size, self.method = size, method

        def __call__(self, img):
            return img.resize((self.size[1], self.size[0]), self.method)

    class ToTensor:
        def __call__(self, img):
            a = np.asarray(img)
            a = a[:, :, None] if a.ndim == 2 else a
            return torch.from_numpy(np.ascontiguousarray(a)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)

    class Normalize:
        def __init__(self, mean, std):
            self.mean, self.std = torch.tensor(mean, dtype=torch.float32), torch.tensor(std, dtype=torch.float32)

        def __call__(self, t):
            return t.clone().sub_(self.mean[:, None, None]).div_(self.std[:, None, None])

    for c in (Compose, Lambda, Grayscale, Resize, ToTensor, Normalize):
        setattr(tr, c.__name__, c)
    tv.transforms = tr
    sys.modules['torchvision'], sys.modules['torchvision.transforms'] = tv, tr


def _cv2_stub():
    from oracle import cv_raster
    cv2 = types.ModuleType('cv2')

    def circle(img, center, radius, color, thickness):
        assert thickness == -1
        cv_raster.fill_circle(img, int(center[0]), int(center[1]), radius, color)
    cv2.circle = circle
    sys.modules['cv2'] = cv2


def main():
    import dataset_fixture as fx
    from animateportrait_amd.data import image_prep
    _torchvision_stub()
    _cv2_stub()
    if not hasattr(np, 'int'):
        np.int = int
    sys.path.insert(0, REF)
    import data.umlvd_ifw_dataset as ref
    calls = []

    def recording(fn):
        def wrapped(*a, **k):
            out = fn(*a, **k)
            calls.append((int(out['crop_pos'][0]), int(out['crop_pos'][1]), int(out['flip'])))
            return out
        return wrapped
    ref.get_params2, ref.get_params3 = recording(ref.get_params2), recording(ref.get_params3)

    work = tempfile.mkdtemp()
    root = os.path.join(work, 'tree')
    fx.write_tree(root, os.path.join(work, 'datasets', 'list'))
    os.chdir(work)                                   # the reference reads datasets/list/... relative to the working directory
    opt = fx.options(os.path.join(work, 'datasets', 'list'))
    ds = ref.UMLVDIFWDataset(opt)
    luts = {'image': image_prep.lut('image'), 'mask': image_prep.lut('mask')}

    def item_for(seed, index):
        random.seed(seed)
        torch.manual_seed(seed)
        del calls[:]
        it = ds[index]
        if torch.equal(it['tB_lm_68'], it['B1_lm_68']):
            branch = 0
        else:
            branch = 1 if torch.equal(it['tB_lm_68'], it['B_lm_68']) else 2
        return it, branch, list(calls)

    chosen, seed = {}, 0
    while len(chosen) < 3:                           # the first seed that reaches each branch; sample index = branch
        seed += 1
        for index in range(3):
            _, branch, _ = item_for(seed, index)
            if branch == index and branch not in chosen:
                chosen[branch] = seed
    out = {'seeds': np.array([chosen[b] for b in range(3)]), 'indices': np.arange(3), 'step': np.array(STEP)}
    for s in range(3):
        it, branch, params = item_for(chosen[s], s)
        out['branch_%d' % s] = np.array(branch)
        out['params_%d' % s] = np.array(params, dtype=np.int32)             # rows: A, B, B1 -- (x, y, flip)
        out['paths_%d' % s] = np.array([os.path.relpath(it[k], root) for k in ('A_paths', 'B_paths', 'B1_path', 'B2_path')])
        out['image_paths_%d' % s] = np.array(it['image_paths'])
        for k, v in it.items():
            if not torch.is_tensor(v):
                continue
            if v.dtype == torch.int32:
                out['%s_%d' % (k, s)] = v.numpy()
            elif v.dim() == 2:
                out['%s_%d' % (k, s)] = v.numpy().astype(np.float32)
            elif k.startswith('warp_motion'):
                out['%s_%d' % (k, s)] = v.numpy().astype(np.float32)[::STEP, ::STEP]
            elif k.startswith('realA_static_warp'):
                out['%s_%d' % (k, s)] = v.numpy().astype(np.float32)[:, ::STEP, ::STEP]
            else:
                kind = 'mask' if 'mask' in k else 'image'
                t = v.float()
                u8 = torch.round((t * 0.5 + 0.5) * 255 if kind == 'image' else t * 255).clamp(0, 255).to(torch.uint8)
                assert torch.equal(luts[kind][u8.long()], t), k             # lossless: the tensor is the table of its bytes
                out['%s_u8_%d' % (k, s)] = u8.numpy()
    path = os.path.join(HERE, 'dataset.npz')
    np.savez_compressed(path, **out)
    print('dataset.npz %.1f KB, seeds %s' % (os.path.getsize(path) / 1024, out['seeds'].tolist()))


if __name__ == '__main__':
    main()
