"""Landmark -> motion grid on the device: ``cal_motion256`` of the reference's data layer
(Module2/data/umlvd_ifw_dataset.py:60-74, umlvdfw_test_dataset.py:67-81), which builds the ``warp_motion`` input of the
generator with ``scipy.interpolate.griddata(destination, source, 256x256 grid, method='linear')`` on the CPU for every
frame (~50 ms -- two orders of magnitude more than the generator needs for the frame).

Same definition here: Delaunay triangulation of the 68 destination landmarks + the reference's 8 border points
(``scipy.spatial.Delaunay``, the triangulation griddata itself builds; 76 points, a fraction of a millisecond on the
host), then ONE kernel launch (``ap_motion_grid``) rasterises the piecewise-linear map for the whole batch and writes
the normalised ``(N, S, S, 2)`` grid where the generator reads it.  SURVEY.md section 8f, row N3.

``triangulate='device'`` (opt-in) triangulates on the device as well (``ap_delaunay``, one workgroup per frame): the
landmarks may then live on the device, nothing is copied to the host, nothing synchronises, and the call -- two kernel
launches between a few torch ops -- can be captured in a graph.  DESIGN.md section 4c states the contract that makes the
device triangulation unique, and the measured times of both paths.
"""
import ctypes

import numpy as np
import torch

from .. import _capi as C

# umlvd_ifw_dataset.py:62 (row, col); the repeated corners are the reference's
EDGES = np.array([[0, 0], [255, 255], [0, 255], [255, 0], [0, 255], [255, 0], [255, 255], [255, 255]], dtype=np.float64)


def triangulate(dest):
    """Delaunay simplices (T, 3) int32 of the (P, 2) destination points, as griddata(linear) builds them."""
    from scipy.spatial import Delaunay
    return np.ascontiguousarray(Delaunay(dest).simplices.astype(np.int32))


_triangulate_host = triangulate      # cal_motion256's ``triangulate`` keyword hides the function's name inside it


_OVERFLOW = {}       # device index -> int32 [1]: min(0, every ap_delaunay count since the last check): sticky, < 0 after an overflow


def _overflow_flag(device):
    key = device.index if device.index is not None else torch.cuda.current_device()
    if key not in _OVERFLOW:
        _OVERFLOW[key] = torch.zeros(1, dtype=torch.int32, device=device)
    return _OVERFLOW[key]


def triangulate_device(pts_dev, tcap=None):
    """Delaunay triangulation of (N, P, 2) float32 device points (row, col) by ``ap_delaunay``, on the current stream and
    without a synchronisation.  Returns ``(tri, count)`` on the device: (N, tcap, 3) int32 rows of ascending point indices in
    lexicographic order, -1 past ``count[n]``; ``count[n] == -1`` (and no row) where a set has more than ``tcap`` triangles
    (default 2 P: a planar triangulation has fewer than 2 P).  An overflow is remembered per device until
    ``check_triangulations`` asks for it.  (The first call on a device allocates that flag, and the first ``cal_motion256``
    of a size uploads the border points: make one call outside a graph capture.)"""
    if not (torch.is_tensor(pts_dev) and pts_dev.is_cuda and pts_dev.dtype == torch.float32 and pts_dev.dim() == 3
            and pts_dev.shape[2] == 2):
        raise ValueError('triangulate_device: expected a (N, P, 2) float32 device tensor')
    pts_dev = pts_dev.contiguous()
    n, p = pts_dev.shape[0], pts_dev.shape[1]
    tcap = 2 * p if tcap is None else int(tcap)
    with torch.cuda.device(pts_dev.device):
        tri = torch.empty((n, tcap, 3), dtype=torch.int32, device=pts_dev.device)
        count = torch.empty((n,), dtype=torch.int32, device=pts_dev.device)
        stream = ctypes.c_void_p(torch.cuda.current_stream(pts_dev.device).cuda_stream)
        C.check(C.lib().ap_delaunay(ctypes.c_void_p(pts_dev.data_ptr()), n, p, tcap, ctypes.c_void_p(tri.data_ptr()),
                                    ctypes.c_void_p(count.data_ptr()), stream), 'delaunay')
        flag = _overflow_flag(pts_dev.device)
        torch.minimum(flag, count.amin().view(1), out=flag)
    return tri, count


def check_triangulations(device=None):
    """Reads and clears the device's overflow flag (one synchronising read): raises if any set triangulated by
    ``triangulate_device`` / ``cal_motion256(triangulate='device')`` since the last check had more triangles than rows."""
    device = torch.device(device if device is not None else 'cuda:0')
    key = device.index if device.index is not None else torch.cuda.current_device()
    flag = _OVERFLOW.get(key)
    if flag is None:
        return
    low = int(flag.item())
    flag.zero_()
    if low < 0:
        raise RuntimeError('animateportrait_amd: ap_delaunay found more triangles than the rows it was given for at least one '
                           'point set since the last check; the motion grids of those sets are invalid')


_EDGES_DEV = {}      # (device, size) -> the border points on the device (uploaded once: later calls copy nothing from the host)


def _edges_on(device, size):
    key = (str(device), size)
    if key not in _EDGES_DEV:
        _EDGES_DEV[key] = torch.tensor(EDGES * ((size - 1) / 255.0), dtype=torch.float32).to(device)
    return _EDGES_DEV[key]


def _cal_motion_device(lm2d0, lm2d, device, size):
    """cal_motion256 with the triangulation on the device: torch ops on ``device`` + ap_delaunay + ap_motion_grid."""
    def dev32(a):
        t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
        return t.to(device=device, dtype=torch.float32)
    a0, a1 = dev32(lm2d0), dev32(lm2d)
    if a0.dim() == 2:
        a0, a1 = a0.unsqueeze(0), a1.unsqueeze(0)
    n = a0.shape[0]
    edges = _edges_on(device, size).unsqueeze(0).expand(n, -1, -1)
    pts = torch.cat([a1.flip(-1), edges], 1).contiguous()                                       # (row, col)
    val = torch.cat([a0.flip(-1), edges], 1).contiguous()
    tri, _ = triangulate_device(pts)
    out = torch.empty((n, size, size, 2), dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        C.check(C.lib().ap_motion_grid(ctypes.c_void_p(pts.data_ptr()), ctypes.c_void_p(val.data_ptr()),
                                       ctypes.c_void_p(tri.data_ptr()), n, pts.shape[1], tri.shape[1], size,
                                       ctypes.c_void_p(out.data_ptr()), stream), 'motion_grid')
    return out


def cal_motion256(lm2d0, lm2d, device=None, size=256, triangulate='host'):
    """lm2d0 / lm2d: source / destination landmarks, (68, 2) or (N, 68, 2), as (x, y) pixels (the txt files).
    Returns the (N, size, size, 2) float32 motion grid on ``device`` (what the reference's dataset yields as
    ``warp_motion``, umlvdfw_test_dataset.py:149-151).
    triangulate: 'host' -- scipy.spatial.Delaunay per frame on the CPU, triangles uploaded; 'device' -- ap_delaunay: the
    landmarks (numpy arrays or tensors on any device; tensors on ``device`` are used in place) never visit the host and the
    call does not synchronise.  Follow a batch of 'device' calls with ``check_triangulations(device)``."""
    if triangulate not in ('host', 'device'):
        raise ValueError("cal_motion256: triangulate must be 'host' or 'device', not %r" % (triangulate,))
    device = torch.device(device if device is not None else 'cuda:0')
    if device.type != 'cuda':
        raise RuntimeError('animateportrait_amd: cal_motion256 rasterises on the MI355X; there is no CPU path')
    if triangulate == 'device':
        return _cal_motion_device(lm2d0, lm2d, device, size)
    # (C-contiguous copies: an expanded / broadcast view would carry its zero strides through every step below and
    # reach the kernel as a non-contiguous device tensor)
    a0 = np.array(lm2d0.cpu() if torch.is_tensor(lm2d0) else lm2d0, dtype=np.float64, order='C')
    a1 = np.array(lm2d.cpu() if torch.is_tensor(lm2d) else lm2d, dtype=np.float64, order='C')
    if a0.ndim == 2:
        a0, a1 = a0[None], a1[None]
    n = a0.shape[0]
    edges = EDGES * ((size - 1) / 255.0)
    dst = np.concatenate([a1[:, :, [1, 0]], np.broadcast_to(edges, (n,) + edges.shape)], 1)     # (row, col)
    src = np.concatenate([a0[:, :, [1, 0]], np.broadcast_to(edges, (n,) + edges.shape)], 1)
    tris = [_triangulate_host(dst[i]) for i in range(n)]
    tmax = max(t.shape[0] for t in tris)
    tri = np.full((n, tmax, 3), -1, dtype=np.int32)
    for i, t in enumerate(tris):
        tri[i, :t.shape[0]] = t
    pts = torch.from_numpy(np.ascontiguousarray(dst, dtype=np.float32)).to(device).contiguous()
    val = torch.from_numpy(np.ascontiguousarray(src, dtype=np.float32)).to(device).contiguous()
    trid = torch.from_numpy(np.ascontiguousarray(tri)).to(device).contiguous()
    out = torch.empty((n, size, size, 2), dtype=torch.float32, device=device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    C.check(C.lib().ap_motion_grid(ctypes.c_void_p(pts.data_ptr()), ctypes.c_void_p(val.data_ptr()),
                                   ctypes.c_void_p(trid.data_ptr()), n, dst.shape[1], tmax, size,
                                   ctypes.c_void_p(out.data_ptr()), stream), 'motion_grid')
    return out
