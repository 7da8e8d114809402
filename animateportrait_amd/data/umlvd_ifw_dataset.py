"""The reference's training dataset (Module2/data/umlvd_ifw_dataset.py:111-436 UMLVDIFWDataset, with the transforms of
base_dataset.py:81-213), with the batch prepared on the device.

Same files (photo / drawing lists, the landmark maps, landmark txt, masks and static drawings beside them, the 34 video
clips), same random decisions in the same order on ``random`` and ``torch.rand`` -- ``plan_sample`` -- and the same item,
but yielded as one already-batched dict per step:

  * the ~23 PIL transforms per sample run as a few ``apd_image_prep_u8`` launches per batch (data/image_prep.py; one pinned
    upload and one launch per group of images of equal size, channels and mode), bit-exact against PIL;
  * the 68 cv2.circle calls are ``losses.landmark_discs``, the two scipy.griddata grids are
    ``cal_motion256(triangulate='device')``, the two F.grid_sample calls the project's grid-sample kernel.

``--data_prep host`` prepares the images through PIL on the CPU instead (same bits); the geometry stages are the same.
The windows (winA ...) stay on the host: the model validates them there (losses.windows_to_device)."""
import concurrent.futures
import glob
import os
import random

import numpy as np
import torch

from . import image_prep
from .motion import cal_motion256, check_triangulations

# left <-> right mirror of the 68 landmarks, and of the 10 extra points some files carry (umlvd_ifw_dataset.py:23-25)
FLIP68 = [16, 15, 14, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0, 26, 25, 24, 23, 22, 21, 20, 19, 18, 17, 27, 28, 29, 30, 35, 34, 33,
          32, 31, 45, 44, 43, 42, 47, 46, 39, 38, 37, 36, 41, 40, 54, 53, 52, 51, 50, 49, 48, 59, 58, 57, 56, 55, 64, 63, 62, 61, 60,
          67, 66, 65]
FLIP_EXTRA = [69, 68, 70, 72, 71, 74, 73, 75, 77, 76]
IMG_EXTENSIONS = ('.jpg', '.jpeg', '.png', '.ppm', '.bmp', '.tif', '.tiff')
CLIPS = 34
MASK_PARTS = (('use_mask', '', 'nose'), ('use_eye_mask', 'e', 'eyes'), ('use_lip_mask', 'l', 'lips'))


def _round_int(v):
    return int(np.round(v))


def crop_params_face(opt, size, rx=0.15, ry=0.2, rs=0.7):
    """get_params2: a crop that keeps the default face window inside; draws randint x, randint y, random flip"""
    new_w = new_h = opt.load_size
    x1 = max(0, _round_int((rx + rs) * new_w) - opt.crop_size)
    x2 = min(max(0, new_w - opt.crop_size), _round_int(rx * new_w))
    x = random.randint(x1, x2)
    y1 = max(0, _round_int((ry + rs) * new_h) - opt.crop_size)
    y2 = min(max(0, new_h - opt.crop_size), _round_int(ry * new_h))
    y = random.randint(y1, y2)
    flip = random.random() > 0.5
    return x, y, flip


def crop_params_windows(opt, size, win1, win2):
    """get_params3: a crop that keeps the union of two frame windows inside; draws randint only where the window leaves a
    choice, then the random flip"""
    w, h = size
    rx1, rx2 = min(win1[0], win2[0]) / w, max(win1[1], win2[1]) / w
    ry1, ry2 = min(win1[2], win2[2]) / h, max(win1[3], win2[3]) / h
    new_w = new_h = opt.load_size

    def axis(r1, r2, new):
        if r1 < 0:
            return 0
        if r2 > 1:
            return new - opt.crop_size
        lo = max(0, _round_int(r2 * new) - opt.crop_size)
        hi = min(max(0, new - opt.crop_size), _round_int(r1 * new))
        return random.randint(lo, hi) if lo <= hi else lo
    x = axis(rx1, rx2, new_w)
    y = axis(ry1, ry2, new_h)
    flip = random.random() > 0.5
    return x, y, flip


def trans_lm(lm, params, opt, size, win=None, rx=0.15, ry=0.2, rs=0.7):
    """Landmarks (P, 2) float32 (x, y) of the file -> of the cropped, flipped image, and the face window [x1, x2, y1, y2]
    there, in the reference's float32 tensor arithmetic (umlvd_ifw_dataset.py:13-42).  Changes ``lm`` in place."""
    w, h = size
    tx, ty, flip = params
    flip = flip and not opt.no_flip
    lm[:, 0] = lm[:, 0] * opt.load_size / w - tx
    lm[:, 1] = lm[:, 1] * opt.load_size / h - ty
    if flip:
        lm[:, 0] = opt.crop_size - lm[:, 0]
        lm[:68, :] = lm[FLIP68, :]
        if lm.shape[0] > 68:
            lm[68:, :] = lm[FLIP_EXTRA, :]
    if win is None:
        x1 = int(round(rx * opt.load_size - tx))
        x2 = x1 + int(round(rs * opt.load_size))
        y1 = int(round(ry * opt.load_size - ty))
        y2 = y1 + int(round(rs * opt.load_size))
    else:
        x1, x2, y1, y2 = win
        box = int(round((x2 - x1) * opt.load_size / w))
        x1 = int(round(x1 * opt.load_size / w - tx))
        x2 = x1 + box
        y1 = int(round(y1 * opt.load_size / h - ty))
        y2 = y1 + box
    if flip:
        x1, x2 = opt.crop_size - x2, opt.crop_size - x1
    return lm, torch.IntTensor([x1, x2, y1, y2])


def read_landmarks(path):
    return torch.Tensor([[float(e.split()[0]), float(e.split()[1])] for e in open(path).read().splitlines()])


def read_window(path):
    e = open(path).read().splitlines()[0].split()
    return [float(e[0]), float(e[1]), float(e[2]), float(e[3])]


def transform_mask(mask, dx, dy):
    """One (1, H, W) mask shifted by the affine grid [[1, 0, dx], [0, 1, dy]] (umlvd_ifw_dataset.py:99-107): torch ops, one
    call per sample as in the reference -- this is the --max_offset > 3 branch, off the common path."""
    theta = torch.tensor([[1, 0, float(dx)], [0, 1, float(dy)]], dtype=torch.float32, device=mask.device)
    grid = torch.nn.functional.affine_grid(theta.unsqueeze(0), mask.unsqueeze(0).size(), align_corners=False)
    return torch.nn.functional.grid_sample(mask.unsqueeze(0), grid, align_corners=False)[0]


def _siblings(path, kind, b_folder='/Drawing/', static_folder='/fakeB_static/'):
    """the reference's path rules: a photo under /Photo/ or a drawing under /Drawing/ (the cartoon dataset: /Cartoon/) -> the
    files that go with it"""
    a, b = ('/Photo/', 'A') if '/Photo/' in path else (b_folder, 'B')
    if kind == 'lm':
        return path.replace(a, '/%slm/MTCNN/' % b)
    if kind == 'txt':
        return path.replace(a, '/%slm_txt/MTCNN/' % b)[:-4] + '.txt'
    if kind == 'win':
        return path.replace(a, '/%slm_txt/MTCNN/' % b)[:-4] + '_win.txt'
    if kind == 'static':
        return path.replace('/Photo/', static_folder)
    return path.replace(a, '/%smask/%s/' % (b, kind))


def _list_images(folder, limit):
    out = []
    for root, _, names in sorted(os.walk(folder)):
        out += [os.path.join(root, n) for n in names if n.lower().endswith(IMG_EXTENSIONS)]
    return out[:int(min(limit, len(out)))]


class UMLVDIFWDataset:
    """Iterable of batches (already batched: ``opt.batch_size`` samples per item), tensors on ``cuda:<gpu_ids[0]>``."""
    # what umlvd_ifw_cartoon_dataset.py changes: the folder of the B images, the folder of the static pictures, and whether the
    # B side has video clips (scanner_frag_*: the B1 / B2 items, the get_params3 draws, the select_target12 branch)
    B_FOLDER, STATIC_FOLDER, HAS_CLIPS = '/Drawing/', '/fakeB_static/', True

    def sib(self, path, kind):
        return _siblings(path, kind, self.B_FOLDER, self.STATIC_FOLDER)

    @staticmethod
    def modify_commandline_options(parser, is_train):
        parser.add_argument('--list_dir', type=str, default='datasets/list',
                            help='prefix of the list files <list_dir>/<phase>A|B/<dataroot>.txt')
        parser.add_argument('--data_prep', type=str, default='device', choices=['device', 'host'],
                            help='image transforms of a batch: device = apd_image_prep_u8 launches, host = PIL on the CPU')
        parser.add_argument('--cache_decoded', action='store_true', help='keep the decoded 8-bit images in host memory')
        parser.add_argument('--shuffle_seed', type=int, default=0,
                            help='the order of epoch e is drawn from a generator seeded with (shuffle_seed, e): equal on every rank')
        return parser

    def __init__(self, opt):
        self.opt = opt
        if opt.preprocess != 'resize_and_crop':
            raise NotImplementedError("umlvd_ifw: --preprocess %s is not served; the reference trains with resize_and_crop" % opt.preprocess)
        if getattr(opt, 'isTrain', True) and getattr(opt, 'warp_loss', 2) == 1:
            raise NotImplementedError('umlvd_ifw: --warp_loss 1 warps the static drawing with cv2.remap(INTER_CUBIC) while loading, '
                                      'which this data layer does not have; use --warp_loss 2 (the default: the warp runs on the device)')
        self.rank, self.world = getattr(opt, 'rank', 0), getattr(opt, 'world_size', None)
        if self.world is None:
            self.world = torch.distributed.get_world_size() if (torch.distributed.is_available() and torch.distributed.is_initialized()) else 1
        list_dir = getattr(opt, 'list_dir', 'datasets/list')
        list_a = '%s/%s/%s.txt' % (list_dir, opt.phase + 'A', opt.dataroot)
        list_b = '%s/%s/%s.txt' % (list_dir, opt.phase + 'B', opt.dataroot)
        if os.path.exists(list_a) and os.path.exists(list_b):
            self.A_paths = sorted(open(list_a).read().splitlines())
            self.B_paths = sorted(open(list_b).read().splitlines())
        else:
            self.A_paths = sorted(_list_images(os.path.join(opt.dataroot, opt.phase + 'A'), opt.max_dataset_size))
            self.B_paths = sorted(_list_images(os.path.join(opt.dataroot, opt.phase + 'B'), opt.max_dataset_size))
        if not self.A_paths or not self.B_paths:
            raise RuntimeError('umlvd_ifw: no images: neither the lists %s / %s nor %s/%sA|B hold any' % (list_a, list_b, opt.dataroot, opt.phase))
        clip_root = '/'.join(self.B_paths[0].split('/')[:-2])
        self.B12_paths = [sorted(glob.glob(clip_root + '/scanner_frag_%d_MTCNN/*.png' % c)) for c in range(CLIPS)] if self.HAS_CLIPS else []
        self.A_size, self.B_size = len(self.A_paths), len(self.B_paths)
        self.B12_size = sum(len(c) for c in self.B12_paths)
        print('A size:', self.A_size)
        print('B size:', self.B_size)
        if self.HAS_CLIPS:
            print('B12 size:', self.B12_size)
        btoa = opt.direction == 'BtoA'
        self.input_nc = opt.output_nc if btoa else opt.input_nc
        self.output_nc = opt.input_nc if btoa else opt.output_nc
        self.data_prep = getattr(opt, 'data_prep', 'device')
        self._cache = {} if getattr(opt, 'cache_decoded', False) else None
        self._sizes = {}
        self._pool = None
        self.epoch = 0               # counts __iter__ calls: every rank iterates once per epoch, so the counts agree
        gpu_ids = getattr(opt, 'gpu_ids', [0]) or [0]
        self.device = torch.device('cuda:%d' % gpu_ids[0])

    def __len__(self):
        return max(self.A_size, self.B_size)

    # ------------------------------------------------------------------ decisions
    def _size(self, path):
        if path not in self._sizes:
            from PIL import Image
            with Image.open(path) as im:
                self._sizes[path] = im.size
        return self._sizes[path]

    def plan_sample(self, index):
        """Every random decision and every landmark of item ``index``, drawn in the reference's order (the call sequence on
        ``random`` / ``torch.rand`` is the contract): B index; get_params2 for A and for B; clip, frame, get_params3; the
        branch draw r; the offsets of branches 1 / 2; the four coh_use_more draws.  Decodes nothing."""
        opt = self.opt
        p = {'index': index}
        p['A_path'] = A_path = self.A_paths[index % self.A_size]
        index_b = index % self.B_size if opt.serial_batches else random.randint(0, self.B_size - 1)
        p['B_path'] = B_path = self.B_paths[index_b]
        size_a, size_b = self._size(A_path), self._size(B_path)
        lm_a, lm_b = read_landmarks(self.sib(A_path, 'txt')), read_landmarks(self.sib(B_path, 'txt'))
        p['pA'] = crop_params_face(opt, size_a)
        p['pB'] = crop_params_face(opt, size_b)
        p['A_lm_68'], p['winA'] = trans_lm(lm_a, p['pA'], opt, size_a)
        p['B_lm_68'], p['winBr'] = trans_lm(lm_b, p['pB'], opt, size_b)
        p['image_paths'] = os.path.basename(A_path)[:-4] + '->' + os.path.basename(B_path)[:-4] + '.png'

        if self.HAS_CLIPS:
            clip = random.randint(0, len(self.B12_paths) - 1)
            frame = random.randint(0, len(self.B12_paths[clip]) - 2)
            p['B1_path'], p['B2_path'] = B1_path, B2_path = self.B12_paths[clip][frame], self.B12_paths[clip][frame + 1]
            size_b1 = self._size(B1_path)
            lm_b1, lm_b2 = read_landmarks(self.sib(B1_path, 'txt')), read_landmarks(self.sib(B2_path, 'txt'))
            win1, win2 = read_window(self.sib(B1_path, 'win')), read_window(self.sib(B2_path, 'win'))
            p['pB1'] = crop_params_windows(opt, size_b1, win1, win2)
            p['B1_lm_68'], p['winBr1'] = trans_lm(lm_b1, p['pB1'], opt, size_b1, win1)
            p['B2_lm_68'], p['winBr2'] = trans_lm(lm_b2, p['pB1'], opt, size_b1, win2)

        p['r'] = r = random.random()
        p['dxdy'] = None
        if self.HAS_CLIPS and r <= opt.select_target12_thre:
            p['branch'] = 0
            p['tB_lm_68'], p['tB2_lm_68'] = p['B1_lm_68'].clone(), p['B2_lm_68'].clone()
            p['winB'], p['winB2'] = p['winBr1'].clone(), p['winBr2'].clone()
        else:
            p['branch'], base, win = (1, p['B_lm_68'], p['winBr']) if r <= opt.select_noniden_thre else (2, p['A_lm_68'], p['winA'])
            p['tB_lm_68'] = base.clone()
            offset = torch.rand(p['tB_lm_68'].shape) * opt.max_offset
            offset2 = torch.rand([1, 2]) * opt.max_offset
            offset[48:68, :] = offset2.repeat(20, 1)
            if opt.max_offset > 3:
                offset = torch.rand([1, 2]) * opt.max_offset
                p['dxdy'] = (-offset[0, 0] / opt.crop_size, -offset[0, 1] / opt.crop_size)
                offset = offset.repeat(68, 1)
            p['offset'] = offset
            p['tB2_lm_68'] = p['tB_lm_68'] + offset
            p['winB'], p['winB2'] = win.clone(), win.clone()
        if opt.coh_use_more:
            c3 = random.randint(0, len(self.B12_paths) - 1)
            c4 = random.randint(0, len(self.B12_paths) - 1)
            f3 = random.randint(0, len(self.B12_paths[c3]) - 1)
            f4 = random.randint(0, len(self.B12_paths[c4]) - 1)
            p['B3_path'], p['B4_path'] = self.B12_paths[c3][f3], self.B12_paths[c4][f4]
        return p

    # ------------------------------------------------------------------ images
    def _jobs(self, plans):
        """The image transforms a batch needs: (path, as_rgb, (x, y, flip), to_gray, kind, [(key, sample), ...]).  One
        transform may fill several keys: the reference clones it."""
        opt = self.opt
        gray_in, gray_out = self.input_nc == 1, self.output_nc == 1
        parts = [(suf, folder) for flag, suf, folder in MASK_PARTS if getattr(opt, flag)]
        jobs = []
        for i, p in enumerate(plans):
            def par(q):
                return (q[0], q[1], int(q[2] and not opt.no_flip))
            pa, pb = par(p['pA']), par(p['pB'])
            br = p['branch']
            A, B = p['A_path'], p['B_path']
            if self.HAS_CLIPS:
                pb1, B1, B2 = par(p['pB1']), p['B1_path'], p['B2_path']
            jobs.append((A, True, pa, gray_in, 'image', [('A', i)]))
            jobs.append((B, True, pb, gray_out, 'image', [('B', i)]))
            jobs.append((self.sib(A, 'lm'), False, pa, True, 'image', [('A_lm', i), ('tA_lm', i)] + ([('tB_lm', i)] if br == 2 else [])))
            jobs.append((self.sib(B, 'lm'), False, pb, True, 'image', [('B_lm', i)] + ([('tB_lm', i)] if br == 1 else [])))
            for suf, folder in parts:
                both = [('B_mask' + suf, i), ('B2_mask' + suf, i)]
                jobs.append((self.sib(A, folder), False, pa, True, 'mask', [('A_mask' + suf, i)] + (both if br == 2 else [])))
                jobs.append((self.sib(B, folder), False, pb, True, 'mask', [('Br_mask' + suf, i)] + (both if br == 1 else [])))
            if self.HAS_CLIPS:
                jobs.append((B1, True, pb1, gray_out, 'image', [('B1', i)]))
                jobs.append((B2, True, pb1, gray_out, 'image', [('B2', i)]))
            if br == 0:           # the clip's own landmark maps and masks are the targets (the reference prepares them always)
                jobs.append((self.sib(B1, 'lm'), False, pb1, True, 'image', [('tB_lm', i)]))
                jobs.append((self.sib(B2, 'lm'), False, pb1, True, 'image', [('tB2_lm', i)]))
                for suf, folder in parts:
                    jobs.append((self.sib(B1, folder), False, pb1, True, 'mask', [('B_mask' + suf, i)]))
                    jobs.append((self.sib(B2, folder), False, pb1, True, 'mask', [('B2_mask' + suf, i)]))
            if opt.coh_use_more:
                jobs.append((p['B3_path'], True, pb, gray_out, 'image', [('B3', i)]))
                jobs.append((p['B4_path'], True, pb, gray_out, 'image', [('B4', i)]))
            if getattr(opt, 'isTrain', True) and (getattr(opt, 'warp_loss', 2) == 2 or getattr(opt, 'identity_loss', 2) == 2):
                jobs.append((self.sib(A, 'static'), True, pa, gray_out, 'image', [('fakeB_static', i)]))
        return jobs

    def _decode_one(self, key):
        path, as_rgb = key
        if self._cache is not None and key in self._cache:
            return self._cache[key]
        from PIL import Image
        with Image.open(path) as im:
            if as_rgb:
                im = im.convert('RGB')
            elif im.mode not in ('L', 'RGB'):
                im = im.convert('L')          # these files go through Grayscale(1) first, which is convert('L')
            arr = np.asarray(im)
            arr = np.ascontiguousarray(arr)
        if self._cache is not None:
            self._cache[key] = arr
        return arr

    def decode(self, jobs):
        """{(path, as_rgb): uint8 array} of every file the jobs read, decoded by PIL in a pool of at most 16 threads"""
        keys = sorted({(j[0], j[1]) for j in jobs})
        return dict(zip(keys, self.pool().map(self._decode_one, keys)))

    def pool(self):
        if self._pool is None:
            self._pool = concurrent.futures.ThreadPoolExecutor(max_workers=min(16, max(1, getattr(self.opt, 'num_threads', 4))))
        return self._pool

    def image_tensors(self, plans, mode=None, decoded=None):
        """{key: (B, C, crop, crop) float32} of every image-derived key: on the device for mode 'device' (one pinned upload
        and one launch per group of equal source size, channels and mode), on the host for mode 'host' (PIL, in the decode pool's threads).  Samples of
        ``tB2_lm`` that are drawn from landmarks (branches 1 and 2) are left zero here."""
        mode = mode or self.data_prep
        opt = self.opt
        jobs = self._jobs(plans)
        decoded = decoded if decoded is not None else self.decode(jobs)
        n, crop = len(plans), opt.crop_size
        device = self.device if mode == 'device' else torch.device('cpu')
        groups = {}
        for j in jobs:
            a = decoded[(j[0], j[1])]
            groups.setdefault((a.shape, j[3] and a.ndim == 3, j[4]), []).append(j)
        out = {}
        for (shape, gray, kind), js in groups.items():
            params = torch.tensor([j[2] for j in js], dtype=torch.int32)
            if mode == 'device':
                hs, ws = shape[0], shape[1]
                c = 1 if len(shape) == 2 else shape[2]
                stage = torch.empty((len(js), hs, ws, c), dtype=torch.uint8).pin_memory()
                buf = stage.numpy()
                for k, j in enumerate(js):
                    buf[k] = decoded[(j[0], j[1])].reshape(hs, ws, c)
                res = image_prep.prep_device(stage.to(device, non_blocking=True), params, opt.load_size, crop, gray, kind)
            else:
                res = image_prep.prep_host([decoded[(j[0], j[1])] for j in js], params.tolist(), opt.load_size, crop, gray, kind,
                                            pool=self.pool())
            by_key = {}
            for k, j in enumerate(js):
                for key, i in j[5]:
                    by_key.setdefault(key, ([], []))
                    by_key[key][0].append(k)
                    by_key[key][1].append(i)
            for key, (src, dst) in by_key.items():
                if key not in out:
                    out[key] = torch.zeros((n,) + tuple(res.shape[1:]), dtype=torch.float32, device=device)
                if dst == list(range(n)) and src == list(range(src[0], src[0] + n)):
                    out[key] = res[src[0]:src[0] + n]
                else:
                    out[key][torch.tensor(dst, device=device)] = res[torch.tensor(src, device=device)]
        return out

    # ------------------------------------------------------------------ batches
    def make_batch(self, plans, mode=None):
        """The batched item of ``plans``: every key of the reference's item that set_input reads, plus realA_static_warp,
        realA_static_warp2, B_lm and tA_*.  Needs the device."""
        from .. import losses, ops
        opt, dev = self.opt, self.device
        n = len(plans)
        item = {k: v.to(dev, non_blocking=True) for k, v in self.image_tensors(plans, mode).items()}

        def stack(key):
            return torch.stack([p[key] for p in plans])
        clips = self.HAS_CLIPS
        lm_keys = ('A_lm_68', 'B_lm_68', 'tB_lm_68', 'tB2_lm_68') + (('B1_lm_68', 'B2_lm_68') if clips else ())
        lms = torch.stack([stack(k) for k in lm_keys]).to(dev)
        for j, k in enumerate(lm_keys):
            item[k] = lms[j]
        item['tA_lm_68'] = item['A_lm_68'].clone()
        for k in ('winA', 'winBr') + (('winBr1', 'winBr2') if clips else ()) + ('winB', 'winB2'):
            item[k] = stack(k)
        for key, k in (('A_paths', 'A_path'), ('B_paths', 'B_path')) + ((('B1_path', 'B1_path'), ('B2_path', 'B2_path')) if clips else ()) \
                + (('image_paths', 'image_paths'),):
            item[key] = [p[k] for p in plans]

        drawn = [i for i, p in enumerate(plans) if p['branch'] != 0]     # second target drawn from landmarks: cv2.circle, radius 3 / 5
        if drawn:
            discs = losses.landmark_discs(item['tB2_lm_68'], opt.crop_size, opt.crop_size, radius=5 if opt.crop_size == 512 else 3)
            if 'tB2_lm' in item:
                idx = torch.tensor(drawn, device=dev)
                item['tB2_lm'] = item['tB2_lm'].index_copy(0, idx, discs[idx])
            else:
                item['tB2_lm'] = discs

        self.shift_second_masks(item, plans)

        size = opt.crop_size
        motion = cal_motion256(torch.cat([item['A_lm_68'], item['A_lm_68']]), torch.cat([item['tB_lm_68'], item['tB2_lm_68']]),
                               device=dev, size=size, triangulate='device')
        check_triangulations(dev)
        item['warp_motion'], item['warp_motion2'] = motion[:n], motion[n:]
        real_a = item['A'].contiguous()
        item['realA_static_warp'] = ops.grid_sample(real_a, item['warp_motion'].contiguous(), align_corners=True)
        item['realA_static_warp2'] = ops.grid_sample(real_a, item['warp_motion2'].contiguous(), align_corners=True)
        return item

    def shift_second_masks(self, item, plans):
        """--max_offset > 3 (umlvd_ifw_dataset.py:324-335, 360-371): the second target's masks move with its offset.  In the
        drawing branch each of B2_mask / B2_maske / B2_maskl is the moved Br mask.  In the photo branch the reference writes
        every moved mask to B2_mask -- the last one enabled stays there -- and leaves B2_maske / B2_maskl unmoved: its own slip,
        kept (B2_mask is written where that key exists).  Works on tensors of any device, on fresh copies."""
        shifted = [i for i, p in enumerate(plans) if p['dxdy'] is not None]
        parts = [suf for _, suf, _ in MASK_PARTS if 'B2_mask' + suf in item]
        if not shifted or not parts:
            return item
        before = {suf: item['B2_mask' + suf] for suf in parts}
        for suf in parts:                                                      # (a key may share its memory with the key it clones)
            item['B2_mask' + suf] = before[suf].clone()
        for i in shifted:
            dx, dy = plans[i]['dxdy']
            for suf in parts:
                moved = transform_mask(before[suf][i], dx, dy)
                if plans[i]['branch'] == 1:
                    item['B2_mask' + suf][i] = moved
                elif 'B2_mask' in item:
                    item['B2_mask'][i] = moved
        return item

    def batches(self, epoch=None):
        """Index lists of one epoch for this rank.  The order is shuffled (unless --serial_batches) by a generator seeded with
        (--shuffle_seed, epoch), so every rank draws the same order whatever its own ``random`` state; it is cut to a multiple
        of world x batch_size where it has one (else of world), and rank r takes order[r::world].  Every rank therefore
        runs the same number of batches, of equal sizes -- each step is a collective -- and the shards are disjoint."""
        epoch = self.epoch if epoch is None else epoch
        if len(self) < self.world:
            raise RuntimeError('umlvd_ifw: %d samples for %d ranks' % (len(self), self.world))
        order = list(range(len(self)))
        if not self.opt.serial_batches:
            random.Random('%d/%d' % (getattr(self.opt, 'shuffle_seed', 0), epoch)).shuffle(order)
        b, w = self.opt.batch_size, self.world
        keep = (len(order) // (w * b)) * (w * b) or (len(order) // w) * w
        order = order[:keep][self.rank::w]
        return [order[i:i + b] for i in range(0, len(order), b)]

    def __iter__(self):
        batches = self.batches()
        self.epoch += 1
        for idx in batches:
            yield self.make_batch([self.plan_sample(i) for i in idx])
