"""The photo's 68 landmarks on the device -- what the reference reads from ``face_alignment.FaceAlignment(LandmarksType._3D,
flip_input=True).get_landmarks(img)`` (main_end2end_module2.py:186-193) and this package otherwise takes as ``--photo_landmarks``.

    python -m animateportrait_amd.landmarks --photo ALIGNED.png --fan_weights FILE --out shape.txt \\
        [--face_box x0,y0,x1,y1] [--channel_order bgr|rgb]

One detection: the crop about the face box and its mirrored copy (apf_fan_crop, one launch), one FAN forward at B = 2 (fan.py),
the flip sum + argmax + quarter-pixel step + inverse transform (apf_fan_decode, one launch).  Only the 68 x 2 result crosses to
the host.  Deviations from the package, all stated in DESIGN.md section 4c-9: the face box comes from this project's MTCNN
detector (mtcnn.Detector) or from the caller, not from the package's SFD network; the depth network is not built -- z is 0, and
module1.adjust_and_norm_input_face overwrites that column anyway; parity with the package, its checkpoint and cv2's resize is
unpinned (the contract is tests/fan_reference.py).
"""
import argparse
import ctypes
import sys

import numpy as np
import torch

from . import _faceapi as F

# the 68-point mirror table (apf_fan_decode holds the same one): jaw i <-> 16 - i, brows, nose, eyes, mouth
PAIR = list(range(F.FAN_POINTS))
for _a, _b in ([(i, 16 - i) for i in range(8)] + [(17 + i, 26 - i) for i in range(5)] + [(31, 35), (32, 34)] +
               [(36, 45), (37, 44), (38, 43), (39, 42), (40, 47), (41, 46)] +
               [(48, 54), (49, 53), (50, 52), (55, 59), (56, 58), (60, 64), (61, 63), (65, 67)]):
    PAIR[_a], PAIR[_b] = _b, _a

ORDERS = {'rgb': F.FAN_RGB, 'bgr': F.FAN_BGR}


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _box4(box):
    b = np.asarray(box, dtype=np.float64).reshape(-1)
    if b.size < 4:
        raise ValueError('a face box is (x0, y0, x1, y1), got %s' % (box,))
    return [float(v) for v in b[:4]]


def fan_crop(image, box, R=256, order='bgr', flip=True):
    """(H, W, 3) uint8 RGB picture on the device + box -> (1 + flip, 3, R, R) fp32 in [0, 1] (apf_fan_crop)"""
    if not (torch.is_tensor(image) and image.is_cuda and image.dtype == torch.uint8 and image.dim() == 3 and image.shape[2] == 3
            and image.is_contiguous()):
        raise TypeError('fan_crop: the picture is a contiguous (H, W, 3) uint8 tensor on the GPU')
    if order not in ORDERS:
        raise ValueError('fan_crop: channel order %r, served: bgr, rgb' % (order,))
    H, W = image.shape[:2]
    out = torch.empty((2 if flip else 1, 3, R, R), dtype=torch.float32, device=image.device)
    F.check(F.lib().apf_fan_crop(_p(image), H, W, *_box4(box), R, int(bool(flip)), ORDERS[order], _p(out), _stream(image.device)),
            'fan_crop')
    return out


def fan_decode(hm, boxes, hm_flipped=None, truncate=True):
    """(B, 68, Hm, Hm) fp32 heat maps on the device (+ those of the mirrored inputs) -> (B, 68, 2) fp32 landmarks in picture
    pixels, on the device (apf_fan_decode); boxes: B face boxes on the host"""
    for t in (hm, hm_flipped):
        if t is not None and not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise TypeError('fan_decode: heat maps are contiguous fp32 tensors on the GPU')
    B, P, Hm, Wm = hm.shape
    if P != F.FAN_POINTS or Hm != Wm or (hm_flipped is not None and hm_flipped.shape != hm.shape):
        raise ValueError('fan_decode: maps of %s (flipped: %s), served: (B, 68, Hm, Hm)'
                         % (tuple(hm.shape), None if hm_flipped is None else tuple(hm_flipped.shape)))
    rows = [_box4(b) for b in boxes]
    if len(rows) != B:
        raise ValueError('fan_decode: %d boxes for %d images' % (len(rows), B))
    host = (ctypes.c_double * (4 * B))(*[v for r in rows for v in r])
    out = torch.empty((B, P, 2), dtype=torch.float32, device=hm.device)
    F.check(F.lib().apf_fan_decode(_p(hm), _p(hm_flipped), B, Hm, ctypes.cast(host, ctypes.c_void_p), int(bool(truncate)), _p(out),
                                   _stream(hm.device)), 'fan_decode')
    return out


class PhotoLandmarks:
    """fan: a prepared fan.FAN (fan.load_fan); detector: an mtcnn.Detector for pictures that come without a box (made on first
    use from ``mtcnn_weights``)."""

    def __init__(self, fan, device='cuda', detector=None, mtcnn_weights=None, resolution=256):
        self.fan, self.device, self.detector, self.mtcnn_weights, self.resolution = fan, torch.device(device), detector, mtcnn_weights, resolution

    def face_box(self, image_u8):
        """the highest-score face of the project's MTCNN detector"""
        from . import mtcnn
        if self.detector is None:
            self.detector = mtcnn.Detector(self.mtcnn_weights or mtcnn.DEFAULT_WEIGHTS, device=self.device)
        boxes, _ = self.detector.detect(image_u8)
        if len(boxes) == 0:
            raise RuntimeError('PhotoLandmarks: no face found in the picture (pass the box)')
        return boxes[int(np.argmax(boxes[:, 4])), :4]

    def detect(self, image_u8, box=None, order='bgr', flip=True, truncate=True):
        """(H, W, 3) uint8 RGB picture (numpy or tensor) -> (68, 3) float32: x, y in picture pixels, z = 0"""
        img = image_u8 if torch.is_tensor(image_u8) else torch.from_numpy(np.ascontiguousarray(image_u8))
        if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
            raise ValueError('PhotoLandmarks: the picture is (H, W, 3) uint8 RGB, got %s %s' % (tuple(img.shape), img.dtype))
        img = img.to(self.device).contiguous()
        if box is None:
            box = self.face_box(img)
        with torch.cuda.device(self.device):
            maps = self.fan(fan_crop(img, box, self.resolution, order, flip))
            pts = fan_decode(maps[:1], [box], maps[1:2] if flip else None, truncate)
        out = np.zeros((F.FAN_POINTS, 3), np.float32)
        out[:, :2] = pts[0].cpu().numpy()
        return out


def parse_box(text):
    try:
        vals = [float(v) for v in text.split(',')]
    except ValueError:
        vals = []
    if len(vals) != 4:
        raise argparse.ArgumentTypeError('a face box is x0,y0,x1,y1 (four numbers), got %r' % text)
    return vals


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--photo', required=True, help='the aligned picture (what --align mtcnn leaves)')
    ap.add_argument('--fan_weights', required=True, help="face_alignment's 3D-FAN checkpoint: a state_dict or a TorchScript archive")
    ap.add_argument('--out', required=True, help='txt, 68 rows "x y z" (z = 0)')
    ap.add_argument('--face_box', type=parse_box, default=None, help='x0,y0,x1,y1; default: the MTCNN detector\'s best face')
    ap.add_argument('--mtcnn_weights', default=None)
    ap.add_argument('--channel_order', choices=('bgr', 'rgb'), default='bgr',
                    help='bgr: the network is fed the picture as the reference feeds it (a cv2.imread array where RGB is expected)')
    ap.add_argument('--gpu', type=int, default=0)
    a = ap.parse_args(argv)
    from PIL import Image
    from . import fan
    device = torch.device('cuda', a.gpu)
    img = np.asarray(Image.open(a.photo).convert('RGB'))
    det = PhotoLandmarks(fan.load_fan(a.fan_weights, device), device, mtcnn_weights=a.mtcnn_weights)
    np.savetxt(a.out, det.detect(img, a.face_box, a.channel_order), fmt='%.6f')
    print('wrote', a.out)
    return 0


if __name__ == '__main__':
    sys.exit(main())
