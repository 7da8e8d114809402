"""Module1's clip-level landmark post-processing on the host: the reference's own numpy / scipy statements, function by function,
each with the reference file:line it restates.  ``landmark_post`` holds the same steps on CUDA tensors (libapseq.so); ``savgol``,
``calib_baseline`` and ``segment_assemble`` have its call shapes, so ``module1.predict_landmarks_speaker_aware`` drives either module
with one loop.  numpy in, numpy out; scipy is imported inside the functions that need it."""
import numpy as np

from .stream import smooth_landmarks


def _savgol(x, window, order=3):
    from scipy.signal import savgol_filter
    return savgol_filter(x, window, order, axis=0)


savgol = _savgol                              # ``landmark_post.savgol``'s call shape: savgol(x, window)


def close_pose_branch_mouth(fl, ratio=0.99):
    """train_audio2landmark.py:119-130 on (T, 204): pull the upper / lower lip contours of the pose branch together."""
    fl = fl.reshape((-1, 68, 3))
    index1, index2 = list(range(59, 54, -1)), list(range(67, 64, -1))
    mean_out = 0.5 * fl[:, 49:54] + 0.5 * fl[:, index1]
    fl[:, 49:54] = mean_out * ratio + fl[:, 49:54] * (1 - ratio)
    fl[:, index1] = mean_out * ratio + fl[:, index1] * (1 - ratio)
    mean_in = 0.5 * (fl[:, 61:64] + fl[:, index2])
    fl[:, 61:64] = mean_in * ratio + fl[:, 61:64] * (1 - ratio)
    fl[:, index2] = mean_in * ratio + fl[:, index2] * (1 - ratio)
    return fl.reshape(-1, 204)


def calib_baseline(pred, amp_lip_x=2.0, amp_lip_y=2.0, ratio=0.5):
    """__calib_baseline_pred_fls__ (:235-245): per coordinate, subtract the mean of its K smallest values over the
    segment, then amplify the mouth's x / y."""
    x = np.array(pred, dtype=np.float32, copy=True)
    k = int(x.shape[0] * ratio)
    for c in range(204):
        idx = np.argpartition(x[:, c], k)
        x[:, c] = x[:, c] - np.mean(x[idx[:k], c])
    x[:, 48 * 3::3] *= amp_lip_x
    x[:, 48 * 3 + 1::3] *= amp_lip_y
    return x


def _signed_area(pts):
    """util/geo_math.py:27-39: fan of signed triangles from the first vertex"""
    ab, ac = pts[1:-1] - pts[0], pts[2:] - pts[0]
    return float(0.5 * np.sum(ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]))


def solve_inverse_lip(fl):
    """__solve_inverse_lip2__ (:594-617) on (T, 204), frame by frame (frame j reads the already fixed frame j - 1)."""
    for j in range(fl.shape[0]):
        if _signed_area(fl[j].reshape(68, 3)[60:68, 0:2]) < 0:
            for a, b in ((63, 65), (62, 66), (61, 67)):
                fl[j, b * 3:b * 3 + 3] = 0.5 * (fl[j, a * 3:a * 3 + 3] + fl[j, b * 3:b * 3 + 3])
                fl[j, a * 3:a * 3 + 3] = fl[j, b * 3:b * 3 + 3]
            p = max(j - 1, 0)
            for dst, src in (((55, 59), (64, 68)), ((59, 60), (60, 61)), ((49, 54), (60, 65))):
                d = slice(dst[0] * 3 + 1, dst[1] * 3 + 1, 3)
                s = slice(src[0] * 3 + 1, src[1] * 3 + 1, 3)
                fl[j, d] = fl[j, s] + fl[p, d] - fl[p, s]
    return fl


def segment_assemble(fl, base=None, fid=None, ratio=0.99, amp=1.0, close=True, lip=True, nose=False, out=None):
    """``landmark_post.segment_assemble``'s call shape on a (T, 204) array, out of place, in the float order of
    ``Audio2landmark_model.test``: ``close_pose_branch_mouth(fl, ratio)`` as float32 x float32(amp), + base + fid (close),
    ``solve_inverse_lip`` (lip), the nose top of train_audio2landmark.py:300 (nose); ``out``: (T, 204) rows to write into."""
    x = np.array(fl, copy=True)
    if close:
        x = close_pose_branch_mouth(x, ratio).astype(np.float32) * np.float32(amp)
        if base is not None:
            x = x + base + fid.reshape(1, -1)
    if lip:
        x = solve_inverse_lip(x)
    if nose:
        x[:, 27 * 3:28 * 3] = x[:, 28 * 3:29 * 3] * 2 - x[:, 29 * 3:30 * 3]
    if out is None:
        return x
    out[...] = x
    return out


def blink_stamps(length, rng=np.random):
    """The frames ``add_naive_eye`` blinks at in a clip of ``length`` frames (util/utils.py:373-380): 30, then steps of
    60 + randint(30, 90) while they leave 16 frames behind them.  Draws from ``rng`` what the reference's loop draws."""
    k2 = 15
    stamps, t = [30], 30
    while t < length - 1 - k2:
        t += 60
        t += rng.randint(30, 90)
        if t < length - 1 - k2:
            stamps.append(t)
    return stamps


def add_naive_eye(fl, rng=np.random):
    """util/utils.py:361-393 on (T, 68, C): eyelids slightly closed throughout, plus blinks at random times (the
    reference draws them from numpy's global generator)."""
    pairs = ((37, 41), (38, 40), (43, 47), (44, 46))
    r = 0.95
    for a, b in pairs:
        fa, fb = fl[:, a].copy(), fl[:, b].copy()
        fl[:, a], fl[:, b] = r * fa + (1 - r) * fb, (1 - r) * fa + r * fb
    k1, k2 = 10, 15
    stamps = blink_stamps(fl.shape[0], rng)
    lids = [37, 38, 40, 41, 43, 44, 46, 47]
    for t in stamps:
        for a, b in pairs:
            v = 0.25 * fl[t, a] + 0.75 * fl[t, b]
            fl[t, a], fl[t, b] = v, v.copy()
        for t0 in range(t - k1 + 1, t):
            w = (t - t0) / 1. / k1
            fl[t0, lids] = w * fl[t - k1, lids] + (1 - w) * fl[t, lids]
        for t0 in range(t + 1, t + k2):
            w = (t + k2 - 1 - t0) / 1. / k2
            fl[t0, lids] = w * fl[t, lids] + (1 - w) * fl[t + k2, lids]
    return fl


def to_image_landmarks(fl, scale=1.0, shift=(0.0, 0.0), eyes=True, smooth=True, rng=np.random):
    """main_end2end_module2.py:262-272 on (T, 204): flip / scale / shift x and y into image pixels, ``add_naive_eye``, the two
    clip-level Savitzky-Golay filters.  Returns (T, 68, 3)."""
    fl = np.array(fl, dtype=np.float64).reshape((-1, 68, 3))
    fl[:, :, 0:2] = -fl[:, :, 0:2]
    fl[:, :, 0:2] = fl[:, :, 0:2] / scale - np.asarray(shift, dtype=np.float64)
    if eyes:
        fl = add_naive_eye(fl, rng)
    return smooth_landmarks(fl) if smooth else fl.astype(np.float32)


# ------------------------------------------------------------------------------------------------- rigid registration
T_SHAPE_IDX = (27, 28, 29, 30, 33, 36, 39, 42, 45)      # nose bridge, nose base, the four eye corners: the face's rigid part


def _best_fit_transform(a, b):
    """util/icp.py:5-55: the rigid map (R, t) of the points a (N, 3) onto b (N, 3), Kabsch through LAPACK's SVD; when the fit
    would reflect, the direction of the smallest singular value is mirrored."""
    ca, cb = a.mean(axis=0), b.mean(axis=0)
    u, _, vt = np.linalg.svd((a - ca).T @ (b - cb))
    r = vt.T @ u.T
    if np.linalg.det(r) < 0:
        vt[-1] *= -1
        r = vt.T @ u.T
    return r, cb - r @ ca


def icp_t_shape(frame, std, max_iterations=50, tolerance=1e-4):
    """``icp(frame[T shape], std[T shape])`` of util/icp.py:77-132, whose neighbour search is commented out: the points
    correspond by index.  frame, std: 68 x 3 in any shape.  Returns the (3, 4) float64 [R | t] that maps frame onto std."""
    idx = list(T_SHAPE_IDX)
    a = np.asarray(frame, dtype=np.float64).reshape(68, 3)[idx]
    b = np.asarray(std, dtype=np.float64).reshape(68, 3)[idx]
    src, prev = a.copy(), 0.0
    for _ in range(max_iterations):
        err = np.sum((src - b) ** 2)
        r, t = _best_fit_transform(src, b)
        src = src @ r.T + t
        if abs(prev - err) < tolerance:
            break
        prev = err
    r, t = _best_fit_transform(a, src)
    return np.hstack((r, t[:, None]))


def register_face(frame, anchor):
    """train_content.py:176-183 (``--use_reg_as_std``): the frame's 68 points moved by ``icp_t_shape(frame, anchor)``.
    Rows are float32 in and out, float64 between.  Returns (204,) float32."""
    p = np.asarray(frame, dtype=np.float32).astype(np.float64).reshape(68, 3)
    t34 = icp_t_shape(p, np.asarray(anchor, dtype=np.float32))
    return (p @ t34[:, :3].T + t34[:, 3]).reshape(204).astype(np.float32)


def stabilise_head(fl, std, centerize_face=False, no_y_rotation=False):
    """The two head-stabilisation switches of the reference's test pass (train_audio2landmark.py:312-338) on (T, 204) landmarks,
    in its order: ``centerize_face`` moves every frame's 68-point mean onto that of ``std``; ``no_y_rotation`` registers every
    frame's T shape onto ``std``'s and, with the fitted rotation R = Rz(c) Ry(b) Rx(a) and translation t, maps every point to
    Rz(c) Ry(b) (p - t) + t -- the angle set to zero is the first of scipy's extrinsic 'xyz' triple, whatever the switch's name
    says.  Rows are float32 in and out, float64 between."""
    from scipy.spatial.transform import Rotation
    x = np.asarray(fl, dtype=np.float32).astype(np.float64).reshape(-1, 68, 3)
    sd = np.asarray(std, dtype=np.float32).astype(np.float64).reshape(68, 3)
    if centerize_face:
        x = x - x.mean(axis=1, keepdims=True) + sd.mean(axis=0)
    if no_y_rotation:
        for i in range(x.shape[0]):
            t34 = icp_t_shape(x[i], sd)
            t = t34[:, 3]
            _, b, c = Rotation.from_matrix(t34[:, :3]).as_euler('xyz')
            x[i] = (x[i] - t) @ Rotation.from_euler('xyz', [0.0, b, c]).as_matrix().T + t
    return x.reshape(-1, 204).astype(np.float32)
