"""The float64 statement of the rigid landmark registration (Module1/util/icp.py and its uses in train_content.py:176-183 and
train_audio2landmark.py:312-338), in numpy only.  apq_rigid_register (csrc/seq/seq_register.hip) and the numpy twins of
``animateportrait_amd.landmark_host`` are pinned to it; tests/golden/register.npz pins it to the reference's own functions.

Arithmetic contract: rows are float32 in and out, everything between is float64, one rounding to float32 at the end.

Two 3x3 SVDs stand side by side: LAPACK's (``svd='lapack'``, what the reference calls) and a one-sided Jacobi iteration
(``svd='jacobi'``, what the kernel runs).  Their spread over a test's inputs sets the bar for the kernel's ``pose``."""
import numpy as np

T_SHAPE_IDX = (27, 28, 29, 30, 33, 36, 39, 42, 45)
MAX_ROUNDS = 50
TOLERANCE = 1e-4
FLAG_CENTER, FLAG_NO_X_ROT, FLAG_REGISTER = 1, 2, 4


def svd3_jacobi(h, max_sweeps=30):
    """U, S, Vt of a 3x3 matrix with S descending, as numpy.linalg.svd returns them: one-sided Jacobi (columns of G = H V are
    turned pairwise until they are orthogonal; their lengths are S, their directions U).  The third left vector is the cross
    product of the first two, signed so that S[2] >= 0: a vanishing third column has no direction of its own."""
    g = np.array(h, dtype=np.float64)
    v = np.eye(3)
    eps = np.finfo(np.float64).eps
    for _ in range(max_sweeps):
        turned = False
        for p, q in ((0, 1), (0, 2), (1, 2)):
            alpha, beta, gamma = g[:, p] @ g[:, p], g[:, q] @ g[:, q], g[:, p] @ g[:, q]
            if not abs(gamma) > eps * np.sqrt(alpha * beta):
                continue
            zeta = (beta - alpha) / (2.0 * gamma)
            t = np.copysign(1.0, zeta) / (abs(zeta) + np.sqrt(1.0 + zeta * zeta))
            c = 1.0 / np.sqrt(1.0 + t * t)
            s = c * t
            rot = np.array([[c, s], [-s, c]])
            g[:, [p, q]] = g[:, [p, q]] @ rot
            v[:, [p, q]] = v[:, [p, q]] @ rot
            turned = True
        if not turned:
            break
    s2 = np.sum(g * g, axis=0)
    order = np.argsort(-s2, kind='stable')
    g, v, sv = g[:, order], v[:, order], np.sqrt(s2[order])
    with np.errstate(divide='ignore', invalid='ignore'):
        u = np.empty((3, 3))
        u[:, 0], u[:, 1] = g[:, 0] / sv[0], g[:, 1] / sv[1]
    u[:, 2] = np.cross(u[:, 0], u[:, 1])
    if u[:, 2] @ g[:, 2] < 0:
        u[:, 2] = -u[:, 2]
    return u, sv, v.T.copy()


def best_fit_transform(a, b, svd='lapack'):
    """icp.py:5-55 on (N, 3) points: (R, t, S) of the rigid map of a onto b; S the singular values of the covariance."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    ca, cb = np.mean(a, axis=0), np.mean(b, axis=0)
    h = np.dot((a - ca).T, b - cb)
    u, s, vt = np.linalg.svd(h) if svd == 'lapack' else svd3_jacobi(h)
    r = np.dot(vt.T, u.T)
    if np.linalg.det(r) < 0:
        vt[2, :] *= -1                      # the direction of the smallest singular value
        r = np.dot(vt.T, u.T)
    t = cb - np.dot(r, ca)
    return r, t, s


def icp(a, b, svd='lapack'):
    """icp.py:77-132 on (9, 3) points, correspondences by index: (T (3, 4) = [R | t], rounds run, S of the first round's
    covariance)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    src = a.copy()
    prev, s0, rounds = 0.0, None, 0
    for _ in range(MAX_ROUNDS):
        err = np.sum((src - b) ** 2)
        r, t, s = best_fit_transform(src, b, svd)
        if s0 is None:
            s0 = s
        src = np.dot(src, r.T) + t
        rounds += 1
        if np.abs(prev - err) < TOLERANCE:
            break
        prev = err
    r, t, _ = best_fit_transform(a, src, svd)
    return np.hstack((r, t.reshape(3, 1))), rounds, s0


def euler_bc(r):
    """Angles b, c of R = Rz(c) Ry(b) Rx(a) (scipy's as_euler('xyz')[1:]), away from gimbal lock."""
    return np.arctan2(-r[2, 0], np.sqrt(r[0, 0] ** 2 + r[1, 0] ** 2)), np.arctan2(r[1, 0], r[0, 0])


def rot_zy(b, c):
    cb, sb, cc, sc = np.cos(b), np.sin(b), np.cos(c), np.sin(c)
    return np.array([[cc * cb, -sc, cc * sb], [sc * cb, cc, sc * sb], [-sb, 0.0, cb]])


def rigid_register64(fl, std, flags, svd='lapack'):
    """The statement before its rounding: fl (T, 204) and std (204,) as float32 -> out (T, 204) float64, pose (T, 12) float64,
    and per frame (rounds, S[1] / S[0] of the first covariance, |b| in degrees)."""
    fl32, std32 = np.asarray(fl, dtype=np.float32).reshape(-1, 68, 3), np.asarray(std, dtype=np.float32).reshape(68, 3)
    x, sd = fl32.astype(np.float64), std32.astype(np.float64)
    if flags & ~7 or (flags & FLAG_REGISTER and flags & (FLAG_CENTER | FLAG_NO_X_ROT)):
        raise ValueError('flags = %d' % flags)
    idx = list(T_SHAPE_IDX)
    if flags & FLAG_CENTER:
        x = x - np.mean(x, axis=1, keepdims=True) + np.mean(sd.reshape(1, 68, 3), axis=1, keepdims=True)
    pose, info = np.empty((x.shape[0], 12)), np.empty((x.shape[0], 3))
    out = x.copy()
    for i in range(x.shape[0]):
        t34, rounds, s = icp(x[i, idx], sd[idx], svd)
        pose[i] = t34.reshape(12)
        r, t = t34[:, :3], t34[:, 3]
        b, c = euler_bc(r)
        with np.errstate(divide='ignore', invalid='ignore'):
            info[i] = rounds, s[1] / s[0], np.degrees(abs(b))
        if flags & FLAG_REGISTER:
            out[i] = np.dot(t34, np.hstack((x[i], np.ones((68, 1)))).T).T
        elif flags & FLAG_NO_X_ROT:
            t2 = np.hstack((rot_zy(b, c), t.reshape(3, 1)))
            out[i] = np.dot(t2, np.hstack((x[i] - t, np.ones((68, 1)))).T).T
    return out.reshape(-1, 204), pose, info


def rigid_register(fl, std, flags, svd='lapack'):
    """(out float32 (T, 204), pose float64 (T, 12)) of the statement."""
    out, pose, _ = rigid_register64(fl, std, flags, svd)
    return out.astype(np.float32), pose


# ------------------------------------------------------------------------------------------------------- seeded test inputs
def rot_xyz(a, b, c):
    """Rz(c) Ry(b) Rx(a)"""
    ca, sa = np.cos(a), np.sin(a)
    return rot_zy(b, c) @ np.array([[1.0, 0.0, 0.0], [0.0, ca, -sa], [0.0, sa, ca]])


def seeded_frames(std, n, seed, noise=0.01):
    """n regular frames as float32 (n, 204): ``std`` turned by up to 40 degrees about x and z and 60 about y, scaled by
    0.8 .. 1.25, moved by up to 0.5 per axis, with normal noise of ``noise`` on every coordinate."""
    rng = np.random.RandomState(seed)
    sd = np.asarray(std, dtype=np.float64).reshape(68, 3)
    out = np.empty((n, 68, 3))
    for i in range(n):
        a, c = np.radians(rng.uniform(-40, 40, 2))
        b = np.radians(rng.uniform(-60, 60))
        s = np.exp(rng.uniform(np.log(0.8), np.log(1.25)))
        out[i] = s * sd @ rot_xyz(a, b, c).T + rng.uniform(-0.5, 0.5, 3) + rng.normal(0.0, noise, (68, 3))
    return out.reshape(n, 204).astype(np.float32)


def mirrored(frames):
    """x negated: the best fit of such a frame onto a face is a reflection, so best_fit_transform takes its det < 0 branch"""
    out = np.array(frames, dtype=np.float32, copy=True).reshape(-1, 68, 3)
    out[:, :, 0] = -out[:, :, 0]
    return out.reshape(-1, 204)
