#!/usr/bin/env python3
"""Golden for the rigid landmark registration (tests/golden/register.npz): the reference's own ``icp`` (Module1/util/icp.py,
imported, with scikit-learn for its import line) on seeded frames, and around it the three uses the reference makes of it,
spelled with today's scipy names (``from_matrix`` / ``as_matrix`` for the removed ``from_dcm`` / ``as_dcm``):

* flags 0: the frames as they are, ``pose`` = icp(frame[T shape], std[T shape]);
* flags 1 (centerize_face), 2 (no_y_rotation), 3 (both): the steps of the test pass, train_audio2landmark.py:312-338, in float64;
* flags 4 (use_reg_as_std): train_content.py:176-183, every frame moved by its own T.

Inputs: ``std`` = STD_FACE_LANDMARKS.txt rounded to float32 (also copied to tests/golden/STD_FACE_LANDMARKS.txt, as data), 24
regular frames of ``register_reference.seeded_frames(std, 24, 20)``, then std itself, a mirrored regular frame and a regular frame
scaled by 1.5.  Float32 rows in, float64 between, float32 ``out_<flags>`` and float64 ``pose_<flags>`` out.

Run with the reference checkout at hand:  python tests/golden/make_register_golden.py REFERENCE_ROOT  (or AP_REFERENCE_ROOT)"""
import os
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

SEED, N_REGULAR = 20, 24


def main():
    from scipy.spatial.transform import Rotation
    import register_reference as rr
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('AP_REFERENCE_ROOT')
    if not ref:
        raise SystemExit(__doc__)
    sys.path.insert(0, os.path.join(ref, 'Module1'))
    from util.icp import icp
    std_txt = os.path.join(ref, 'Module1', 'src', 'dataset', 'utils', 'STD_FACE_LANDMARKS.txt')
    shutil.copyfile(std_txt, os.path.join(HERE, 'STD_FACE_LANDMARKS.txt'))
    std = np.loadtxt(std_txt).reshape(204).astype(np.float32)
    regular = rr.seeded_frames(std, N_REGULAR, SEED)
    frames = np.concatenate([regular, std.reshape(1, 204), rr.mirrored(regular[3:4]), regular[5:6] * np.float32(1.5)]).astype(np.float32)
    idx = list(rr.T_SHAPE_IDX)
    sd = std.astype(np.float64).reshape(68, 3)
    out = {'std': std, 'frames': frames}
    for flags in (0, 1, 2, 3, 4):
        x = frames.astype(np.float64).reshape(-1, 68, 3)
        pose = np.empty((x.shape[0], 12))
        if flags & 1:
            x = x - np.mean(x, axis=1, keepdims=True) + np.mean(sd.reshape(1, 68, 3), axis=1, keepdims=True)
        t_shapes = x[:, idx, :]
        for i in range(x.shape[0]):
            T, _, _ = icp(t_shapes[i], sd[idx])
            pose[i] = T[:3].reshape(12)
            if flags & 2:
                angles = Rotation.from_matrix(T[:3, :3]).as_euler('xyz')
                kept = Rotation.from_euler('xyz', [0.0, angles[1], angles[2]]).as_matrix()
                moved = np.hstack((x[i] - T[:3, 3], np.ones((68, 1))))
                x[i] = np.dot(np.hstack((kept, T[:3, 3:4])), moved.T).T
            elif flags & 4:
                x[i] = np.dot(T, np.hstack((x[i], np.ones((68, 1)))).T).T[:, 0:3]
        out['out_%d' % flags] = x.reshape(-1, 204).astype(np.float32)
        out['pose_%d' % flags] = pose
    path = os.path.join(HERE, 'register.npz')
    np.savez_compressed(path, **out)
    print('register.npz %.1f KB' % (os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
