"""The reference's test-time dataset (Module2/data/umlvdfw_test_dataset.py:84-175 UMLVDFWTestDataset) on the same file tree,
with the batch prepared on the device -- the data layer of ``python -m animateportrait_amd.test --model geomcgt_ifw_test``.

Same lists, same three landmark-path rules (:123-128), same random decisions in the same order (``plan_item``), same item;
yielded as one already-batched dict per ``--batch_size`` items (the last one may be short):

  * the photo through ``image_prep`` (umlvd_ifw_dataset.py's transform: one apd_image_prep_u8 launch per group of equal
    source size), or through PIL with ``--data_prep host`` -- same bits;
  * both landmark maps (draw2, op 0 or 1) by one ``apd_landmark_map`` call on the 2B landmark sets;
  * the scipy.griddata grid by ``cal_motion256(triangulate='device')``, the static warp by the grid-sample kernel.

B's image is never opened: the reference gives it A's size (:136) and reads only its landmark txt.
``--draw_op 2`` (a 3-channel polygon picture) is refused: the generator's landmark encoder takes one channel."""
import os
import random

import torch

from . import visuals
from .motion import cal_motion256, check_triangulations
from .umlvd_ifw_dataset import UMLVDIFWDataset, _list_images, crop_params_face, read_landmarks, trans_lm


def landmark_txt(path, side):
    """the three path substitutions of umlvdfw_test_dataset.py:123-128"""
    if side == 'A':
        return path.replace('/Photo/', '/Alm_txt/MTCNN/')[:-4] + '.txt'
    if 'Alm' in path:
        return path.replace('/Alm/MTCNN/', '/Alm_txt/MTCNN/')[:-4] + '.txt'
    return path.replace('/Drawing/', '/Blm_txt/MTCNN/')[:-4] + '.txt'


class UMLVDFWTestDataset:
    """Iterable of batches, tensors on ``cuda:<gpu_ids[0]>``; windows stay on the host, as in umlvd_ifw."""

    @staticmethod
    def modify_commandline_options(parser, is_train):
        parser.add_argument('--list_dir', type=str, default='datasets/list',
                            help='prefix of the list files <list_dir>/<phase>A|B/<dataroot>.txt')
        parser.add_argument('--data_prep', type=str, default='device', choices=['device', 'host'],
                            help='image transform of a batch: device = apd_image_prep_u8 launches, host = PIL on the CPU')
        parser.add_argument('--cache_decoded', action='store_true', help='keep the decoded 8-bit photos in host memory')
        parser.add_argument('--lmark_lookup', type=str, default='faceLmarkLookup.npy',
                            help='the landmark pairs --draw_op 1 joins (the reference reads this file from its working directory)')
        return parser

    def __init__(self, opt):
        self.opt = opt
        self.draw_op = int(getattr(opt, 'draw_op', 0))
        if self.draw_op == 2:
            raise NotImplementedError('umlvdfw_test: --draw_op 2 draws a 3-channel polygon picture, which the generator\'s '
                                      '1-channel landmark encoder cannot take; use --draw_op 0 (discs) or 1 (discs and contours)')
        if self.draw_op not in (0, 1):
            raise NotImplementedError('umlvdfw_test: --draw_op %d is not one of the reference\'s (0, 1, 2)' % self.draw_op)
        if opt.preprocess not in ('resize_and_crop', 'none'):
            raise NotImplementedError('umlvdfw_test: --preprocess %s is not served; the reference tests with resize_and_crop '
                                      '(none is served for photos that already have the crop size)' % opt.preprocess)
        self.segments = visuals.load_lookup(getattr(opt, 'lmark_lookup', 'faceLmarkLookup.npy')) if self.draw_op == 1 else None
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
            raise RuntimeError('umlvdfw_test: no images: neither the lists %s / %s nor %s/%sA|B hold any'
                               % (list_a, list_b, opt.dataroot, opt.phase))
        self.A_size, self.B_size = len(self.A_paths), len(self.B_paths)
        print('A size:', self.A_size)
        print('B size:', self.B_size)
        btoa = opt.direction == 'BtoA'
        self.input_nc = opt.output_nc if btoa else opt.input_nc
        self.output_nc = opt.input_nc if btoa else opt.output_nc
        self.data_prep = getattr(opt, 'data_prep', 'device')
        gpu_ids = getattr(opt, 'gpu_ids', [0]) or [0]
        self.device = torch.device('cuda:%d' % gpu_ids[0])
        self._images = _PhotoPrep(opt, self.input_nc, self.device)

    def __len__(self):
        return max(self.A_size, self.B_size)

    def plan_item(self, index):
        """Every random decision and every landmark of item ``index`` in the reference's order: B's index (random.randint
        unless --serial_batches), get_params2 for A, get_params2 for B, both trans_lm.  Decodes nothing."""
        opt = self.opt
        p = {'index': index}
        p['A_path'] = a_path = self.A_paths[index % self.A_size]
        index_b = index % self.B_size if opt.serial_batches else random.randint(0, self.B_size - 1)
        p['index_B'] = index_b
        p['B_path'] = b_path = self.B_paths[index_b]
        lm_a, lm_b = read_landmarks(landmark_txt(a_path, 'A')), read_landmarks(landmark_txt(b_path, 'B'))
        size = self._images._size(a_path)                 # B's size is A's (:136)
        if opt.preprocess == 'none' and not (size[0] == size[1] == opt.load_size == opt.crop_size):
            # 'none' leaves such a photo as it is, and so does the resize-and-crop this layer runs; any other size it would not
            raise NotImplementedError('umlvdfw_test: --preprocess none with a %d x %d photo (%s) at load %d / crop %d: served '
                                      'only where all four agree' % (size[0], size[1], a_path, opt.load_size, opt.crop_size))
        p['pA'] = crop_params_face(opt, size)
        p['pB'] = crop_params_face(opt, size)
        p['A_lm_68'], p['winA'] = trans_lm(lm_a, p['pA'], opt, size)
        p['tB_lm_68'], p['winB'] = trans_lm(lm_b, p['pB'], opt, size)
        p['image_paths'] = os.path.basename(a_path)[:-4] + '->' + os.path.basename(b_path)[:-4] + '.png'
        return p

    def make_batch(self, plans, mode=None):
        from .. import ops
        opt, dev = self.opt, self.device
        n, size = len(plans), opt.crop_size
        item = {'A': self._images.photos(plans, mode or self.data_prep).to(dev, non_blocking=True)}
        lms = torch.stack([torch.stack([p[k] for p in plans]) for k in ('A_lm_68', 'tB_lm_68')]).to(dev)
        item['A_lm_68'], item['tB_lm_68'] = lms[0], lms[1]
        maps = visuals.landmark_map(lms.reshape(2 * n, lms.shape[2], 2), self.segments, size, size,
                                    radius=5 if size == 512 else 3, thickness=4 if size == 512 else 2, op=self.draw_op)
        item['A_lm'], item['B_lm'] = maps[:n], maps[n:]
        item['tB_lm'] = item['B_lm'].clone()
        item['winB'] = torch.stack([p['winB'] for p in plans])
        item['A_paths'] = [p['A_path'] for p in plans]
        item['B_paths'] = [p['B_path'] for p in plans]
        item['image_paths'] = [p['image_paths'] for p in plans]
        item['warp_motion'] = cal_motion256(item['A_lm_68'], item['tB_lm_68'], device=dev, size=size, triangulate='device')
        check_triangulations(dev)
        item['realA_static_warp'] = ops.grid_sample(item['A'].contiguous(), item['warp_motion'].contiguous(), align_corners=True)
        return item

    def batches(self):
        """one dict per --batch_size items, in index order; the last one may be short"""
        b = max(1, int(self.opt.batch_size))
        for start in range(0, len(self), b):
            yield self.make_batch([self.plan_item(i) for i in range(start, min(start + b, len(self)))])

    def __iter__(self):
        return self.batches()


class _PhotoPrep(UMLVDIFWDataset):
    """the decode pool, size cache and grouped image transform of the training dataset, with the one job the test item has"""

    def __init__(self, opt, input_nc, device):      # (no lists, no clips: only what image_tensors / decode / pool read)
        self.opt = opt
        self.input_nc, self.device = input_nc, device
        self.data_prep = getattr(opt, 'data_prep', 'device')
        self._cache = {} if getattr(opt, 'cache_decoded', False) else None
        self._sizes = {}
        self._pool = None

    def _jobs(self, plans):
        no_flip = self.opt.no_flip
        return [(p['A_path'], True, (p['pA'][0], p['pA'][1], int(p['pA'][2] and not no_flip)), self.input_nc == 1, 'image',
                 [('A', i)]) for i, p in enumerate(plans)]

    def photos(self, plans, mode):
        return self.image_tensors(plans, mode)['A']
