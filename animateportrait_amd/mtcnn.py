"""MTCNN face detection and photo alignment on the device (libapface.so, include/animateportrait_face.h): what the
reference's end-to-end driver does to an arbitrary photo before anything else reads it (align_mtcnn,
main_end2end_module2.py:12-45; MTCNN/detector.py).

    det = Detector('MTCNN/weights')            # the reference's pnet.npy / rnet.npy / onet.npy, or a plain .npz / a directory of them
    boxes, landmarks = det.detect(image_u8)    # (n, 5) float64, (n, 10) float32
    aligned = det.align_photo(image_u8)        # (512, 512, 3) uint8 RGB, or None without a face

Every stage runs on the device and only enqueues: pixels never return to the host, and the one read-back of a detection is
its final result (counts, status, boxes, landmarks).  Launches are sized by the fixed capacities of the header, the true
counts stay in device memory.  A capacity overflow raises: boxes are never dropped silently.

Deviation from the reference: an image in which P-Net finds no candidate at all yields n = 0 here; the reference raises from
np.vstack([]) there."""
import glob
import math
import os

import numpy as np
import torch

from . import _faceapi as F

THRESHOLDS = (0.6, 0.7, 0.8)
NMS_THRESHOLDS = (0.7, 0.7, 0.7)
LEVEL_NMS = 0.5
MIN_FACE_SIZE = 20.0
DEFAULT_WEIGHTS = os.path.join('MTCNN', 'weights')

# named_parameters() of the reference's nets, in order, and the first fully connected layer with the (C, H, W) it flattens
_LAYOUT = {
    'pnet': (['features.conv1', 'features.prelu1', 'features.conv2', 'features.prelu2', 'features.conv3', 'features.prelu3',
              'conv4_1', 'conv4_2'], None, None, F.PNET_PARAMS),
    'rnet': (['features.conv1', 'features.prelu1', 'features.conv2', 'features.prelu2', 'features.conv3', 'features.prelu3',
              'features.conv4', 'features.prelu4', 'conv5_1', 'conv5_2'], 'features.conv4', (64, 3, 3), F.RNET_PARAMS),
    'onet': (['features.conv1', 'features.prelu1', 'features.conv2', 'features.prelu2', 'features.conv3', 'features.prelu3',
              'features.conv4', 'features.prelu4', 'features.conv5', 'features.prelu5', 'conv6_1', 'conv6_2', 'conv6_3'],
             'features.conv5', (128, 3, 3), F.ONET_PARAMS),
}


def _read_raw(path):
    """{net: {parameter name: float32 array}} from either layout"""
    if os.path.isdir(path) and os.path.exists(os.path.join(path, 'pnet.npy')):
        # the reference's own files: a pickled dict in a 0-d object array
        return {net: {k: np.asarray(v, np.float32) for k, v in np.load(os.path.join(path, net + '.npy'), allow_pickle=True)[()].items()}
                for net in _LAYOUT}
    files = sorted(glob.glob(os.path.join(path, '*.npz'))) if os.path.isdir(path) else [path]
    if not files or not all(os.path.exists(f) for f in files):
        raise FileNotFoundError('MTCNN weights: %s holds neither pnet.npy / rnet.npy / onet.npy nor .npz files' % path)
    flat = {}
    for f in files:
        with np.load(f, allow_pickle=False) as z:
            flat.update({k: z[k] for k in z.files})
    raw = {net: {} for net in _LAYOUT}
    pieces = {}
    for key, a in flat.items():
        net, _, name = key.partition('/')
        if net not in raw:
            raise ValueError('MTCNN weights: key %r names no net (pnet/, rnet/, onet/)' % key)
        name, at, part = name.partition('@')           # a tensor split along axis 0: name@0, name@1, ...
        if at:
            pieces.setdefault((net, name), {})[int(part)] = a
        else:
            raw[net][name] = np.asarray(a, np.float32)
    for (net, name), parts in pieces.items():
        raw[net][name] = np.concatenate([parts[k] for k in range(len(parts))], 0).astype(np.float32)
    return raw


def fold_flatten(weight, chw):
    """The reference's Flatten transposes H and W before it flattens: fold that into the next layer's (out, C*W*H) weight, and
    return it as (C*H*W, out) -- input-major, over the plain (c, h, w) order of an NCHW tensor."""
    c, h, w = chw
    out = weight.shape[0]
    return np.ascontiguousarray(weight.reshape(out, c, w, h).transpose(0, 1, 3, 2).reshape(out, c * h * w).T)


def load_weights(path):
    """{net: packed float32 parameters in the order include/animateportrait_face.h states} from the reference's directory of
    pickled .npy files or from plain .npz (one file or a directory of them) with keys pnet/..., rnet/..., onet/..."""
    raw = _read_raw(path)
    packed = {}
    for net, (modules, fc, chw, total) in _LAYOUT.items():
        parts = []
        for m in modules:
            names = [m + '.weight'] + ([m + '.bias'] if 'prelu' not in m else [])
            for n in names:
                if n not in raw[net]:
                    raise KeyError('MTCNN weights: %s lacks %s' % (net, n))
                a = raw[net][n]
                if m == fc and n.endswith('.weight'):
                    a = fold_flatten(a, chw)
                parts.append(np.asarray(a, np.float32).ravel())
        packed[net] = np.concatenate(parts)
        if packed[net].size != total:
            raise ValueError('MTCNN weights: %s has %d parameters, the nets need %d' % (net, packed[net].size, total))
    return packed


def pyramid(width, height, min_face_size=MIN_FACE_SIZE):
    """[(scale, level height, level width)] as detector.py:31-50 and first_stage.py:28 compute them, in Python floats"""
    scales = []
    m = 12 / min_face_size
    min_length = min(height, width) * m
    k = 0
    while min_length > 12:
        scales.append(m * 0.707 ** k)
        min_length *= 0.707
        k += 1
    return [(s, math.ceil(height * s), math.ceil(width * s)) for s in scales]


def align_window(faces):
    """(x11, y11, size1): the square main_end2end_module2.py:22-41 cuts about the largest face, with its int, // and round"""
    best, maxs = None, 0
    for face in np.asarray(faces, np.float64).reshape(-1, 5):
        x1, y1, x2, y2 = (float(v) for v in face[:4])
        w = x2 - x1 + 1
        h = y2 - y1 + 1
        size = int(min([w, h]) * 1.2)
        cx = x1 + w // 2
        cy = y1 + h // 2
        if size > maxs:
            size1 = int(round(size / 0.7))
            best = (int(cx - size1 // 2), int(cy - (size1 * 11) // 20), size1)
            maxs = size
    return best


def _p(t):
    return None if t is None else t.data_ptr()


class _Job:
    """the device buffers of one image's detection, kept until its result is read"""


class Detector:
    def __init__(self, weights=DEFAULT_WEIGHTS, device='cuda', thresholds=THRESHOLDS, nms_thresholds=NMS_THRESHOLDS,
                 min_face_size=MIN_FACE_SIZE):
        self.device = torch.device(device)
        self.lib = F.lib()
        self.thresholds, self.nms_thresholds, self.min_face_size = tuple(thresholds), tuple(nms_thresholds), float(min_face_size)
        self.params = {k: torch.from_numpy(v).to(self.device) for k, v in load_weights(weights).items()}
        self._ws = {}

    # ---- buffers -----------------------------------------------------------------------------------------------------
    def _buf(self, name, shape, dtype):
        """a scratch buffer shared by every detection on this detector (stream order keeps its users apart)"""
        t = self._ws.get(name)
        n = int(np.prod(shape))
        if t is None or t.numel() < n or t.dtype != dtype:
            t = torch.empty(n, dtype=dtype, device=self.device)
            self._ws[name] = t
        return t[:n].view(shape)

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    # ---- stages (tests drive them one by one) ------------------------------------------------------------------------
    def resize_level(self, img, oh, ow):
        H, W = img.shape[:2]
        out = torch.empty((oh, ow, 3), dtype=torch.uint8, device=self.device)
        F.check(self.lib.apf_resize_level(_p(img), H, W, oh, ow, _p(out), self._stream()), 'resize_level')
        return out

    def pnet(self, level, threshold, maps=False):
        """-> (prob, off, cand_idx, cand_score, cand_off, cand_count); prob / off are None unless maps"""
        h, w = level.shape[:2]
        mh, mw = (h - 1) // 2 - 4, (w - 1) // 2 - 4
        prob = torch.empty((mh, mw), dtype=torch.float32, device=self.device) if maps else None
        off = torch.empty((4, mh, mw), dtype=torch.float32, device=self.device) if maps else None
        idx = self._buf('cand_idx', (F.CAP_LEVEL,), torch.int32)
        score = self._buf('cand_score', (F.CAP_LEVEL,), torch.float32)
        coff = self._buf('cand_off', (F.CAP_LEVEL, 4), torch.float32)
        count = torch.zeros(1, dtype=torch.int32, device=self.device)
        F.check(self.lib.apf_pnet(_p(level), h, w, _p(self.params['pnet']), threshold, _p(prob), _p(off), _p(idx), _p(score), _p(coff),
                                  _p(count), self._stream()), 'pnet')
        return prob, off, idx, score, coff, count

    def stage1_level(self, cand, mw, scale, merged, merged_count, status, level_count=None, cand_boxes=None):
        _, _, idx, score, coff, count = cand
        if cand_boxes is None:
            cand_boxes = self._buf('cand_boxes', (F.CAP_LEVEL, 9), torch.float64)
        F.check(self.lib.apf_stage1_level(_p(idx), _p(score), _p(coff), _p(count), mw, scale, LEVEL_NMS, _p(cand_boxes), _p(level_count),
                                          _p(merged), _p(merged_count), _p(status), self._stream()), 'stage1_level')
        return cand_boxes

    def box_stage(self, boxes, n_in, cap_in, cap_out, nms_threshold, mode, late=False, probs=None, offsets=None, landmarks=None,
                  score_threshold=0.0, status=None, trace=False):
        """-> (out (cap_out, 5), out_landmarks or None, n_out, extras); extras = (picks, cal, sq) when trace"""
        out = torch.zeros((cap_out, 5), dtype=torch.float64, device=self.device)
        out_lm = torch.zeros((cap_out, 10), dtype=torch.float32, device=self.device) if late else None
        n_out = torch.zeros(1, dtype=torch.int32, device=self.device)
        picks = cal = sq = None
        if trace:
            picks = torch.full((cap_in,), -1, dtype=torch.int32, device=self.device)
            cal = torch.zeros((cap_in if late else cap_out, 5), dtype=torch.float64, device=self.device)
            sq = None if late else torch.zeros((cap_out, 5), dtype=torch.float64, device=self.device)
        ws = self._buf('box_ws', (int(self.lib.apf_box_stage_ws_bytes(cap_in)),), torch.uint8)
        F.check(self.lib.apf_box_stage(_p(boxes), boxes.shape[1], _p(n_in), cap_in, _p(probs), _p(offsets), _p(landmarks),
                                       score_threshold, nms_threshold, mode, int(late), _p(out), _p(out_lm), _p(n_out), cap_out,
                                       _p(picks), _p(cal), _p(sq), _p(status), _p(ws), self._stream()), 'box_stage')
        return out, out_lm, n_out, (picks, cal, sq)

    def cutouts(self, img, boxes, count, cap, size):
        """(cap, size, size, 3) uint8; clips `boxes` to the image in place, as the reference's get_image_boxes does"""
        H, W = img.shape[:2]
        out = self._buf('cut%d' % size, (cap, size, size, 3), torch.uint8)
        F.check(self.lib.apf_cutouts(_p(img), H, W, _p(boxes), _p(count), cap, size, _p(out), self._stream()), 'cutouts')
        return out

    def net(self, which, cuts, count, cap):
        """R-Net ('r') or O-Net ('o') -> (probs (cap, 2), offsets (cap, 4), landmarks (cap, 10) or None)"""
        net = F.NET_R if which == 'r' else F.NET_O
        probs = torch.zeros((cap, 2), dtype=torch.float32, device=self.device)
        offsets = torch.zeros((cap, 4), dtype=torch.float32, device=self.device)
        lm = torch.zeros((cap, 10), dtype=torch.float32, device=self.device) if which == 'o' else None
        ws = self._buf('net_ws_' + which, (int(self.lib.apf_net_ws_bytes(net, cap)),), torch.uint8)
        F.check(self.lib.apf_net(net, _p(cuts), _p(count), cap, _p(self.params['rnet' if which == 'r' else 'onet']), _p(ws), _p(probs),
                                 _p(offsets), _p(lm), self._stream()), 'net')
        return probs, offsets, lm

    def crop_resize_cubic(self, img, window, out_size=512, fill=255):
        H, W = img.shape[:2]
        x0, y0, size = window
        out = torch.empty((out_size, out_size, 3), dtype=torch.uint8, device=self.device)
        F.check(self.lib.apf_crop_resize_cubic(_p(img), H, W, x0, y0, size, fill, out_size, _p(out), self._stream()), 'crop_resize_cubic')
        return out

    # ---- the detector ------------------------------------------------------------------------------------------------
    def _to_device(self, image):
        img = image if torch.is_tensor(image) else torch.from_numpy(np.ascontiguousarray(image))
        if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
            raise ValueError('MTCNN: the image is (H, W, 3) uint8 RGB, got %s %s' % (tuple(img.shape), img.dtype))
        return img.to(self.device).contiguous()

    def _enqueue(self, image):
        """every stage of one image; nothing is read back"""
        img = self._to_device(image)
        H, W = img.shape[:2]
        job = _Job()
        job.img = img
        job.status = torch.zeros(1, dtype=torch.int32, device=self.device)
        merged = torch.zeros((F.CAP_MERGED, 9), dtype=torch.float64, device=self.device)
        n_merged = torch.zeros(1, dtype=torch.int32, device=self.device)
        for s, lh, lw in pyramid(W, H, self.min_face_size):
            level = self.resize_level(img, lh, lw)
            cand = self.pnet(level, self.thresholds[0])
            self.stage1_level(cand, (lw - 1) // 2 - 4, s, merged, n_merged, job.status)
        thr, nthr = self.thresholds, self.nms_thresholds
        b1, _, n1, _ = self.box_stage(merged, n_merged, F.CAP_MERGED, F.CAP_RNET, nthr[0], F.NMS_UNION, status=job.status)
        cut = self.cutouts(img, b1, n1, F.CAP_RNET, 24)
        probs, offs, _ = self.net('r', cut, n1, F.CAP_RNET)
        b2, _, n2, _ = self.box_stage(b1, n1, F.CAP_RNET, F.CAP_ONET, nthr[1], F.NMS_UNION, probs=probs, offsets=offs,
                                      score_threshold=thr[1], status=job.status)
        job.n_rnet, job.n_onet = n1, n2
        cut = self.cutouts(img, b2, n2, F.CAP_ONET, 48)
        probs, offs, lm = self.net('o', cut, n2, F.CAP_ONET)
        job.boxes, job.landmarks, job.n, _ = self.box_stage(b2, n2, F.CAP_ONET, F.CAP_ONET, nthr[2], F.NMS_MIN, late=True, probs=probs,
                                                            offsets=offs, landmarks=lm, score_threshold=thr[2], status=job.status)
        return job

    @staticmethod
    def _read(jobs):
        """the one read-back: counts and status of every job in one transfer, then the rows that exist"""
        head = torch.stack([torch.cat([j.n, j.status]) for j in jobs]).cpu().numpy()
        out = []
        for j, (n, status) in zip(jobs, head):
            if status:
                raise RuntimeError('MTCNN: a stage met more boxes than its capacity holds (status %d: 1 = candidates of a level, '
                                   '2 = boxes of all levels, 4 = boxes of a later stage; include/animateportrait_face.h)' % status)
            out.append((j.boxes[:n].cpu().numpy(), j.landmarks[:n].cpu().numpy()))
        return out

    def detect(self, image):
        """(H, W, 3) uint8 RGB (numpy or tensor) -> boxes (n, 5) float64 (x1, y1, x2, y2, score), landmarks (n, 10) float32
        (five x, then five y), in the reference's order"""
        return self._read([self._enqueue(image)])[0]

    def detect_batch(self, images):
        """a list of images (sizes may differ): all of them are enqueued before the one read-back"""
        return self._read([self._enqueue(im) for im in images])

    def align_photo(self, image, out_size=512):
        """the white-padded square about the largest face, resized to out_size by OpenCV's 8-bit INTER_CUBIC rule (parity with
        cv2 itself unpinned: tests/cv_resize_reference.py states the rule).  (out_size, out_size, 3) uint8 RGB as a numpy array,
        or None when no face is found."""
        job = self._enqueue(image)
        boxes, _ = self._read([job])[0]
        window = align_window(boxes)
        if window is None:
            return None
        return self.crop_resize_cubic(job.img, window, out_size).cpu().numpy()
