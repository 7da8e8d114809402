"""Module1's clip-level landmark post-processing on the device: the numpy / scipy functions of ``landmark_host`` and
``stream.smooth_landmarks`` on CUDA tensors, through the ``apq_*`` post-processing calls of libapseq.so (csrc/seq/seq_post.hip).

Every function takes device tensors and returns device tensors; none copies to the host, synchronises, or falls back: a call
the library refuses raises.  The only uploads are the Savitzky-Golay tap table (once per window and device) and the handful of
blink stamps of ``add_naive_eye``, which are drawn on the host from the caller's generator exactly as the host function does."""
import numpy as np
import torch

from . import _seqapi as Q
from . import ops
from .landmark_host import blink_stamps      # noqa: F401  (part of this module's surface)

_TAPS = {}


def savgol_table(window, order=3):
    """The (window // 2 + 1, window) float64 table apq_savgol reads: rows of the projector on polynomials of ``order`` over
    ``window`` equidistant samples.  Row i < window // 2 is scipy's mode='interp' edge (the fitted polynomial evaluated at sample
    i of the first window; by symmetry also sample window - 1 - i of the last one, read backwards), row window // 2 the interior
    taps.  numpy alone: the orthonormal basis of the Vandermonde columns gives the projector without forming a pseudo-inverse."""
    window = int(window)
    if window % 2 != 1 or window <= order:
        raise ValueError('savgol_table: window %d (odd and above the order %d)' % (window, order))
    h = window // 2
    v = np.vander((np.arange(window, dtype=np.float64) - h) / max(h, 1), order + 1, increasing=True)
    q, _ = np.linalg.qr(v)
    return (q @ q.T)[:h + 1].copy()


def _taps(window, dev):
    key = (int(window), str(dev))
    t = _TAPS.get(key)
    if t is None:
        t = _TAPS[key] = torch.from_numpy(savgol_table(window).astype(np.float32)).to(dev)
    return t


def _dev32(x, what, cols=None):
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32):
        raise TypeError('landmark_post.%s takes a float32 CUDA tensor' % what)
    if cols is not None and (x.dim() != 2 or x.shape[1] != cols):
        raise ValueError('landmark_post.%s takes (T, %d), not %s' % (what, cols, tuple(x.shape)))
    return x.contiguous()


def _savgol_into(x, y, c0, c1, c2, w0, w1):
    t, c = x.shape
    taps0 = _taps(w0, x.device) if c1 > c0 else None
    taps1 = _taps(w1, x.device) if c2 > c1 else None
    Q.check(Q.lib().apq_savgol(ops._ptr(x), ops._ptr(y), ops._ptr(taps0), ops._ptr(taps1), t, c, c0, c1, c2, int(w0), int(w1),
                               ops._stream()), 'savgol')
    return y


def savgol(x, window):
    """``scipy.signal.savgol_filter(x, window, 3, axis=0)`` (mode='interp') on a (T, C) tensor; odd window in 5 .. 31, T >= window."""
    x = _dev32(x, 'savgol')
    if x.dim() != 2:
        raise ValueError('landmark_post.savgol takes (T, C), not %s' % (tuple(x.shape),))
    return _savgol_into(x, torch.empty_like(x), 0, x.shape[1], x.shape[1], window, 0)


def smooth_landmarks(fl):
    """``stream.smooth_landmarks`` on a (T, 68, C) tensor: window 15 on the 48 non-lip points, 5 on the lips -- one launch."""
    fl = _dev32(fl, 'smooth_landmarks')
    t, p, c = fl.shape
    x = fl.view(t, p * c)
    if t < 5:
        return fl.clone()
    c1 = 48 * c if t >= 15 else 0
    y = torch.empty_like(x) if c1 else x.clone()              # (a clip too short for the wide window keeps those columns)
    return _savgol_into(x, y, 0 if c1 else 48 * c, 48 * c, p * c, 15, 5).view(t, p, c)


def calib_baseline(pred, amp_lip_x=2.0, amp_lip_y=2.0, ratio=0.5):
    """``landmark_host.calib_baseline`` on a (T, 204) tensor, 2 <= T <= 512."""
    x = _dev32(pred, 'calib_baseline', Q.LM_C)
    y = torch.empty_like(x)
    Q.check(Q.lib().apq_calib_baseline(ops._ptr(x), ops._ptr(y), x.shape[0], int(x.shape[0] * ratio), float(amp_lip_x),
                                       float(amp_lip_y), ops._stream()), 'calib_baseline')
    return y


def segment_assemble(fl, base=None, fid=None, ratio=0.99, amp=1.0, close=True, lip=True, nose=False, out=None):
    """One apq_segment_assemble launch on a (T, 204) segment, T <= 512: ``close_pose_branch_mouth(fl, ratio) * amp + base + fid``
    (close), ``solve_inverse_lip`` (lip), the nose-top extrapolation (nose); ``out``: a contiguous (T, 204) view to write into."""
    x = _dev32(fl, 'segment_assemble', Q.LM_C)
    if out is None:
        out = torch.empty_like(x)
    elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.shape == x.shape):
        raise ValueError('landmark_post.segment_assemble: out must be a contiguous float32 CUDA tensor of the shape of fl')
    base = None if base is None else _dev32(base, 'segment_assemble', Q.LM_C)
    fid = None if fid is None else _dev32(fid.view(1, -1), 'segment_assemble', Q.LM_C)
    if base is not None and base.shape != x.shape:
        raise ValueError('landmark_post.segment_assemble: base %s, fl %s' % (tuple(base.shape), tuple(x.shape)))
    flags = (Q.SEG_CLOSE if close else 0) | (Q.SEG_LIP if lip else 0) | (Q.SEG_NOSE if nose else 0)
    Q.check(Q.lib().apq_segment_assemble(ops._ptr(x), ops._ptr(base), ops._ptr(fid), ops._ptr(out), x.shape[0], float(ratio),
                                         float(amp), flags, ops._stream()), 'segment_assemble')
    return out


def close_pose_branch_mouth(fl, ratio=0.99):
    """``landmark_host.close_pose_branch_mouth`` on a (T, 204) tensor (out of place)."""
    return segment_assemble(fl, ratio=ratio, close=True, lip=False)


def solve_inverse_lip(fl):
    """``landmark_host.solve_inverse_lip`` on a (T, 204) tensor (out of place)."""
    return segment_assemble(fl, close=False, lip=True)


def rigid_register(fl, std, center=False, no_x_rot=False, register=False, pose=False, out=None):
    """One apq_rigid_register launch on (T, 204) frames against ``std`` (204,), a wave per frame (csrc/seq/seq_register.hip):
    ``module1.stabilise_head`` with ``center`` (centerize_face) and ``no_x_rot`` (the reference's no_y_rotation), or
    ``module1.register_face`` on every frame with ``register`` (which excludes the other two).  ``out``: a contiguous (T, 204)
    tensor to write into, ``fl`` itself for in place.  With ``pose`` also returns the (T, 3, 4) float64 [R | t] that
    ``landmark_host.icp_t_shape`` gives for every frame (after the centring, before any angle is removed)."""
    x = _dev32(fl, 'rigid_register', Q.LM_C)
    sd = _dev32(std.reshape(1, -1) if torch.is_tensor(std) else std, 'rigid_register', Q.LM_C)
    if out is None:
        out = torch.empty_like(x)
    elif not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.shape == x.shape):
        raise ValueError('landmark_post.rigid_register: out must be a contiguous float32 CUDA tensor of the shape of fl')
    ps = torch.empty((x.shape[0], 3, 4), dtype=torch.float64, device=x.device) if pose else None
    flags = (Q.REG_CENTER if center else 0) | (Q.REG_NO_X_ROT if no_x_rot else 0) | (Q.REG_REGISTER if register else 0)
    Q.check(Q.lib().apq_rigid_register(ops._ptr(x), ops._ptr(sd), ops._ptr(out), ops._ptr(ps), x.shape[0], flags, ops._stream()),
            'rigid_register')
    return (out, ps) if pose else out


def image_landmarks(fl, scale=1.0, shift=(0.0, 0.0), transform=True, stamps=None):
    """One apq_image_landmarks launch on (T, 204) -> (T, 204): the pixel transform and, with ``stamps`` (a list of frames),
    ``add_naive_eye`` with its blinks at those frames."""
    x = _dev32(fl, 'image_landmarks', Q.LM_C)
    t = x.shape[0]
    st = None
    if stamps is not None:
        if t < 46:
            raise ValueError('add_naive_eye: %d frames, the first blink (frame 30) reads frame 45' % t)
        st = torch.tensor(list(stamps), dtype=torch.int32, device=x.device)
    y = torch.empty_like(x)
    flags = (Q.IMG_TRANSFORM if transform else 0) | (Q.IMG_EYES if st is not None else 0)
    Q.check(Q.lib().apq_image_landmarks(ops._ptr(x), ops._ptr(y), ops._ptr(st), 0 if st is None else st.numel(), t, float(scale),
                                        float(shift[0]), float(shift[1]), flags, ops._stream()), 'image_landmarks')
    return y


def add_naive_eye(fl, rng=np.random):
    """``landmark_host.add_naive_eye`` on a (T, 68, 3) tensor (out of place); T >= 46, else ValueError before anything is launched."""
    fl = _dev32(fl, 'add_naive_eye')
    if fl.dim() != 3 or fl.shape[1:] != (68, 3):
        raise ValueError('landmark_post.add_naive_eye takes (T, 68, 3), not %s' % (tuple(fl.shape),))
    if fl.shape[0] < 46:
        raise ValueError('add_naive_eye: %d frames, the first blink (frame 30) reads frame 45' % fl.shape[0])
    return image_landmarks(fl.view(-1, Q.LM_C), transform=False, stamps=blink_stamps(fl.shape[0], rng)).view(-1, 68, 3)


def to_image_landmarks(fl, scale=1.0, shift=(0.0, 0.0), eyes=True, smooth=True, rng=np.random):
    """``module1.to_image_landmarks`` on a (T, 204) tensor: two launches.  Returns (T, 68, 3)."""
    fl = _dev32(fl.reshape(-1, Q.LM_C) if torch.is_tensor(fl) else fl, 'to_image_landmarks', Q.LM_C)
    t = fl.shape[0]
    if eyes and t < 46:
        raise ValueError('add_naive_eye: %d frames, the first blink (frame 30) reads frame 45' % t)
    out = image_landmarks(fl, scale, shift, transform=True, stamps=blink_stamps(t, rng) if eyes else None).view(t, 68, 3)
    return smooth_landmarks(out) if smooth else out
