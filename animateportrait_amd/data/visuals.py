"""Device stages of the test-time item and of test.py's PNG sink (libapdata.so, include/animateportrait_data.h):

  * ``landmark_map``   draw2(op = 0 | 1) of Module2/data/umlvdfw_test_dataset.py:34-52 for a batch (apd_landmark_map),
  * ``landmark_marks`` get_lmvis of Module2/models/geomcgt_ifw_test_model.py:232-251 per sample (apd_landmark_marks),
  * ``frames_to_u8``   tensor2im of Module2/util/util.py:9-29 for a batch (apd_frames_to_u8), into device memory or into a
    pinned host buffer the kernel writes directly,
  * ``save_png_batch`` the sink: one launch per visual, one stream synchronisation, PNG encoding on a thread pool,
  * ``encode_png_batch`` complete PNG files made on the device (apd_png_encode); ``save_png_batch(encoder='device')`` writes
    them, and the pool is left with the write() calls,
  * ``encode_jpeg_batch`` complete baseline JPEG files made on the device (apd_jpeg_encode): the frames of the MJPEG clip
    ``end2end.py --video avi`` writes through util/avi.py,
  * ``landmark_vis``   landmark sets drawn as coloured contours in painter's order (apd_landmark_vis): vis_landmark of
    main_end2end_module2.py:47-68 with ``FACE_CONTOURS``, the frames of ``end2end.py --landmark_video avi`` and the marked photo
    of ``--side_outputs``.

A missing library or a refused call raises; nothing here falls back to the host."""
import concurrent.futures
import ctypes
import os

import numpy as np
import torch

from .. import _dataapi as D

PNG_THREADS = 16          # a constant, not os.cpu_count(): the encoders share the machine with the data pool


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _device_f32(t, what, dims):
    if not (torch.is_tensor(t) and t.is_cuda and t.dim() == dims):
        raise ValueError('%s: expected a %d-d device tensor' % (what, dims))
    return t.detach().float().contiguous()


def load_lookup(path):
    """faceLmarkLookup.npy: the (S, 2) integer table of landmark pairs draw2(op=1) joins, read at run time as the reference
    reads it (umlvdfw_test_dataset.py:33)."""
    if not os.path.exists(path):
        raise FileNotFoundError('--draw_op 1 joins the landmark pairs of %s, which does not exist: copy faceLmarkLookup.npy '
                                'from the reference\'s Module2/ or name it with --lmark_lookup' % path)
    seg = np.load(path)
    if seg.ndim != 2 or seg.shape[1] != 2 or seg.dtype.kind not in 'iu':
        raise ValueError('%s: expected an (S, 2) integer table, found %s %s' % (path, seg.dtype, seg.shape))
    return np.ascontiguousarray(seg.astype(np.int32))


_SEG = {}        # (device, table bytes) -> device copy


def landmark_map(lm, segments, height, width, radius, thickness, op, lo=-1.0, hi=1.0):
    """lm (N, P, 2) device (x, y); segments (S, 2) int host array or None -> (N, 1, height, width) float32 in {lo, hi}."""
    lm = _device_f32(lm, 'landmark_map', 3)
    n, p, _ = lm.shape
    host = np.zeros((0, 2), np.int32) if segments is None or op == 0 else np.ascontiguousarray(np.asarray(segments, dtype=np.int32))
    s = int(host.shape[0])
    dev = None
    if s:
        key = (str(lm.device), host.tobytes())
        if key not in _SEG:
            _SEG[key] = torch.from_numpy(host).to(lm.device)
        dev = _SEG[key]
    out = torch.empty((n, 1, height, width), dtype=torch.float32, device=lm.device)
    with torch.cuda.device(lm.device):
        D.check(D.lib().apd_landmark_map(_p(lm), _p(dev), host.ctypes.data_as(ctypes.c_void_p) if s else None, n, p, s, height, width,
                                         int(radius), int(thickness), int(op), lo, hi, _p(out), _stream(lm.device)), 'landmark_map')
    return out


def landmark_marks(frames, lm, win, hradius=3):
    """frames (N, C, H, W) device, C in {1, 3}; lm (N, P, 2); win (N, 4) [x1, x2, y1, y2] (tensor, array or list) ->
    (N, 3, H, W): every sample carries its own marks."""
    frames = _device_f32(frames, 'landmark_marks', 4)
    n, c, h, w = frames.shape
    lm = _device_f32(lm.to(frames.device), 'landmark_marks', 3)
    win = torch.as_tensor(np.asarray(win.cpu() if torch.is_tensor(win) else win), dtype=torch.int32).reshape(-1, 4)
    if lm.shape[0] != n or win.shape[0] != n:
        raise ValueError('landmark_marks: %d frames, %d landmark sets, %d windows' % (n, lm.shape[0], win.shape[0]))
    win = win.to(frames.device).contiguous()
    out = torch.empty((n, 3, h, w), dtype=torch.float32, device=frames.device)
    with torch.cuda.device(frames.device):
        D.check(D.lib().apd_landmark_marks(_p(frames), _p(lm), _p(win), n, c, lm.shape[1], h, w, int(hradius), _p(out),
                                           _stream(frames.device)), 'landmark_marks')
    return out


def _face_contours():
    """The drawing vis_landmark (main_end2end_module2.py:47-68) makes of a 68-point face, as a table: every curve joins the
    landmarks first .. last + 1 in turn, a closed one then joins first to last + 1; colours are the reference's BGR tuples read
    as RGB, because it writes the picture with cv2.imwrite."""
    curves = (('jaw', 0, 15, False, 0x1990FF), ('brow', 17, 20, False, 0x32CD32), ('brow', 22, 25, False, 0x32CD32),
              ('nose', 27, 34, False, 0x3FE0D0), ('eye', 36, 40, True, 0xFF6347), ('eye', 42, 46, True, 0xFF6347),
              ('mouth', 48, 58, True, 0xEE82EE), ('mouth', 60, 66, True, 0xEE82EE))
    seg, rgb = [], []
    for _, first, last, closed, colour in curves:
        pairs = [(i, i + 1) for i in range(first, last + 1)] + ([(first, last + 1)] if closed else [])
        seg += pairs
        rgb += [colour] * len(pairs)
    return {'segments': np.array(seg, np.int32), 'colours': np.array(rgb, np.uint32), 'disc_rgb': 0xFF0000, 'points': 68}


FACE_CONTOURS = _face_contours()      # 64 segments in draw order, their five colours, the red of the landmark discs


def face_contour_style(height):
    """(thickness, radius) vis_landmark draws with at this frame height: 2 (height // 256) and height // 256"""
    return 2 * (height // 256), height // 256


def landmark_vis(pts, seg, seg_rgb, height, width, radius, thickness, disc_rgb, bg_rgb=0xFFFFFF, bg=None):
    """pts (N, P, 2) integer (x, y), a device tensor or a host array; seg (S, 2) host integer table or None; seg_rgb (S,)
    0xRRGGBB per segment; bg None (the constant bg_rgb) or a device (1 | N, 3, height, width) float tensor -> (N, 3, height,
    width) float32 on the device: the segments drawn in order as cv2.line, then every point as a filled disc of disc_rgb
    (radius -1: none), later marks on top (apd_landmark_vis).  The caller makes the coordinates integers by the rule of the
    call site it mirrors; a floating-point `pts` is refused."""
    if not torch.is_tensor(pts):
        a = np.asarray(pts)
        if a.dtype.kind not in 'iu':
            raise ValueError('landmark_vis: pts must be integers (found %s): truncate or round them as the mirrored call site does' % a.dtype)
        pts = torch.from_numpy(np.ascontiguousarray(a.astype(np.int32))).cuda()
    if pts.is_floating_point() or pts.dtype == torch.bool or not pts.is_cuda or pts.dim() != 3 or pts.shape[2] != 2:
        raise ValueError('landmark_vis: pts must be an (N, P, 2) integer tensor on the device')
    pts = pts.to(torch.int32).contiguous()
    n, p, _ = pts.shape
    host = np.zeros((0, 2), np.int32) if seg is None else np.ascontiguousarray(np.asarray(seg, dtype=np.int32)).reshape(-1, 2)
    s = int(host.shape[0])
    dev = rgb = None
    if s:
        colours = np.ascontiguousarray(np.asarray(seg_rgb, dtype=np.uint32)).reshape(-1)
        if colours.shape[0] != s:
            raise ValueError('landmark_vis: %d segments, %d colours' % (s, colours.shape[0]))
        key = (str(pts.device), host.tobytes(), colours.tobytes())
        if key not in _SEG:
            _SEG[key] = (torch.from_numpy(host).to(pts.device), torch.from_numpy(colours.view(np.int32)).to(pts.device))
        dev, rgb = _SEG[key]
    bg_frames = 1
    if bg is not None:
        bg = _device_f32(bg, 'landmark_vis', 4)
        bg_frames = bg.shape[0]
        if tuple(bg.shape[1:]) != (3, height, width) or bg.device != pts.device:
            raise ValueError('landmark_vis: bg %s, expected (1 | N, 3, %d, %d) on %s' % (tuple(bg.shape), height, width, pts.device))
    out = torch.empty((n, 3, height, width), dtype=torch.float32, device=pts.device)
    with torch.cuda.device(pts.device):
        D.check(D.lib().apd_landmark_vis(_p(pts), _p(dev), host.ctypes.data_as(ctypes.c_void_p) if s else None, _p(rgb), _p(bg), bg_frames,
                                         n, p, s, height, width, int(radius), int(thickness), int(disc_rgb) & 0xFFFFFF,
                                         int(bg_rgb) & 0xFFFFFF, _p(out), _stream(pts.device)), 'landmark_vis')
    return out


_PINNED = {}      # (shape, device, slot) -> pinned uint8 buffer, reused


def pinned_u8(shape, device, slot=0):
    key = (tuple(shape), str(device), slot)
    if key not in _PINNED:
        _PINNED[key] = torch.empty(tuple(shape), dtype=torch.uint8).pin_memory()
    return _PINNED[key]


def frames_to_u8(frames, out=None, slot=0):
    """frames (N, C, H, W) device float32, C in {1, 3} -> (N, H, W, 3) uint8.  ``out``: None = the pinned host buffer of this
    (shape, device, slot), written by the kernel itself (synchronise the stream before reading it); 'device' = a fresh
    device tensor; or a contiguous uint8 tensor of that shape, on the device or pinned."""
    frames = _device_f32(frames, 'frames_to_u8', 4)
    n, c, h, w = frames.shape
    if out is None:
        out = pinned_u8((n, h, w, 3), frames.device, slot)
    elif isinstance(out, str) and out == 'device':
        out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=frames.device)
    if tuple(out.shape) != (n, h, w, 3) or out.dtype != torch.uint8 or not out.is_contiguous():
        raise ValueError('frames_to_u8: out must be a contiguous (%d, %d, %d, 3) uint8 tensor' % (n, h, w))
    if not out.is_cuda and not out.is_pinned():
        raise ValueError('frames_to_u8: a host destination must be pinned')
    with torch.cuda.device(frames.device):
        D.check(D.lib().apd_frames_to_u8(_p(frames), n, c, h, w, _p(out), _stream(frames.device)), 'frames_to_u8')
    return out


_POOL = None


def png_pool():
    global _POOL
    if _POOL is None:
        _POOL = concurrent.futures.ThreadPoolExecutor(max_workers=PNG_THREADS)
    return _POOL


_PNG = {}         # (N, C, H, W, channels, device, slot) -> (pinned file slots, pinned sizes, device workspace), reused


def encode_png_batch(frames, channels=3, slot=0):
    """frames (N, C, H, W) device float32, C in {1, 3} -> (buf (N, apd_png_bound) uint8, sizes (N,) int32), both pinned host
    buffers of this (shape, channels, device, slot) that the kernels write themselves: after the stream has been synchronised,
    frame i's complete PNG file is ``buf[i, :sizes[i]]``.  channels 3: RGB, grey tiled; channels 1: greyscale, C must be 1."""
    frames = _device_f32(frames, 'encode_png_batch', 4)
    n, c, h, w = frames.shape
    lib = D.lib()
    key = (n, c, h, w, int(channels), str(frames.device), slot)
    if key not in _PNG:
        bound, ws = lib.apd_png_bound(h, w, int(channels)), lib.apd_png_workspace_bytes(n, h, w, int(channels))
        if bound < 0 or ws < 0:
            raise RuntimeError('libapdata png_encode refused: %s' % D.last_error())
        _PNG[key] = (torch.empty((n, bound), dtype=torch.uint8).pin_memory(), torch.zeros((n,), dtype=torch.int32).pin_memory(),
                     torch.empty((ws,), dtype=torch.uint8, device=frames.device))
    buf, sizes, ws = _PNG[key]
    with torch.cuda.device(frames.device):
        D.check(lib.apd_png_encode(_p(frames), n, c, h, w, int(channels), _p(buf), buf.shape[1], _p(sizes), _p(ws), ws.numel(),
                                   _stream(frames.device)), 'png_encode')
    return buf, sizes


_JPEG = {}        # (N, C, H, W, channels, device, slot) -> (pinned file slots, pinned sizes, device workspace), reused


def encode_jpeg_batch(frames, channels=3, quality=90, slot=0):
    """frames (N, C, H, W) device float32, C in {1, 3} -> (buf (N, apd_jpeg_bound) uint8, sizes (N,) int32), both pinned host
    buffers of this (shape, channels, device, slot) that the kernels write themselves: after the stream has been synchronised,
    frame i's complete baseline JPEG file is ``buf[i, :sizes[i]]``.  channels 3: Y Cb Cr 4:4:4, grey tiled; channels 1:
    greyscale, C must be 1.  quality 1..100 scales the standard tables as PIL's ``quality`` does."""
    frames = _device_f32(frames, 'encode_jpeg_batch', 4)
    n, c, h, w = frames.shape
    lib = D.lib()
    key = (n, c, h, w, int(channels), str(frames.device), slot)
    if key not in _JPEG:
        bound, ws = lib.apd_jpeg_bound(h, w, int(channels)), lib.apd_jpeg_workspace_bytes(n, h, w, int(channels))
        if bound < 0 or ws < 0:
            raise RuntimeError('libapdata jpeg_encode refused: %s' % D.last_error())
        _JPEG[key] = (torch.empty((n, bound), dtype=torch.uint8).pin_memory(), torch.zeros((n,), dtype=torch.int32).pin_memory(),
                      torch.empty((ws,), dtype=torch.uint8, device=frames.device))
    buf, sizes, ws = _JPEG[key]
    with torch.cuda.device(frames.device):
        D.check(lib.apd_jpeg_encode(_p(frames), n, c, h, w, int(channels), int(quality), _p(buf), buf.shape[1], _p(sizes), _p(ws),
                                    ws.numel(), _stream(frames.device)), 'jpeg_encode')
    return buf, sizes


PNG_ENCODERS = ('host', 'device')


def save_png_batch(visuals, names, encoder='host'):
    """visuals: {label: (N, C, H, W) device tensor}; names: {label: [N paths]}.  ``encoder='host'``: one apd_frames_to_u8 launch
    per visual into its pinned buffer, one synchronisation, then PIL encodes on the pool.  ``encoder='device'``: one
    apd_png_encode call per visual, one synchronisation, then the pool only writes the files.  Returns the number of files
    written."""
    if encoder not in PNG_ENCODERS:
        raise ValueError('save_png_batch: encoder %r, served: %s' % (encoder, ' and '.join(PNG_ENCODERS)))
    if not visuals:
        return 0
    device = next(iter(visuals.values())).device
    if encoder == 'device':
        staged = [(label, encode_png_batch(t, slot=label)) for label, t in visuals.items()]
        torch.cuda.current_stream(device).synchronize()
        files = [(buf.numpy()[i, :size], names[label][i])
                 for label, (buf, sizes) in staged for i, size in enumerate(sizes.tolist())]

        def write(job):
            with open(job[1], 'wb') as f:
                f.write(job[0])
        list(png_pool().map(write, files))
        return len(files)
    from PIL import Image
    staged = [(label, frames_to_u8(t, slot=label)) for label, t in visuals.items()]
    torch.cuda.current_stream(device).synchronize()
    jobs = [(buf.numpy()[i], names[label][i]) for label, buf in staged for i in range(buf.shape[0])]

    def save(job):
        Image.fromarray(job[0]).save(job[1])
    list(png_pool().map(save, jobs))
    return len(jobs)
