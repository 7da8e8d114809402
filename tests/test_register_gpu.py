"""GPU (-m gpu): apq_rigid_register (csrc/seq/seq_register.hip) through the C ABI against its float64 statement
(tests/register_reference.py), then the clip driver with both head-stabilisation switches on the device against the numpy path.

Inputs: one pool of 625 seeded frames (register_reference.seeded_frames: the standard face turned by up to 40 / 60 / 40 degrees,
scaled by 0.8 .. 1.25, moved by up to 0.5, noise 0.01) whose first three are special -- the standard face itself, a mirrored
frame (its fit takes the det < 0 branch), a frame scaled by 1.5 -- and whose every prefix is a test size.  The statement is
computed once per flag combination for the whole pool: a frame's result depends on nothing but the frame.

Tolerances.  ``out``: the float32 rounding of the statement, to 1 float32 ulp of the frame's largest |coordinate| (the fp64
error is orders below half an ulp: only a rounding tie can differ).  ``pose``: 16 x the spread between the statement's two
float64 SVDs (LAPACK, Jacobi) over the pool, at least 1e-12; the test prints the spread, the bar and the kernel's error.
Measured on an MI355X: spread 6.5e-15, bar 1e-12 (the floor), kernel against the LAPACK statement 6.8e-15 at worst; out 0 ulp
off in all 5 x 625 x 204 values; clip driver 1.2e-7 against a bar of 1.2e-5.  End to end: the bar of tests/test_module1_post_gpu.py, 2e-5 max|ref| + 1e-6."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import register_reference as rr                                                     # noqa: E402

pytestmark = pytest.mark.gpu

POOL_T, SEED = 625, 31
SIZES = (1, 2, 63, 64, 65, 130)
LEGAL_FLAGS = (0, 1, 2, 3, 4)


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def pool():
    """std (204,), frames (625, 204), and per flag combination the statement's (out float32, pose, info); spread and bar"""
    std = np.loadtxt(os.path.join(GOLDEN, 'STD_FACE_LANDMARKS.txt')).reshape(204).astype(np.float32)
    frames = rr.seeded_frames(std, POOL_T, SEED)
    frames[0] = std
    frames[1] = rr.mirrored(frames[7:8])[0]
    frames[2] = frames[9] * np.float32(1.5)
    ref = {}
    for flags in LEGAL_FLAGS:
        out, pose, info = rr.rigid_register64(frames, std, flags)
        ref[flags] = (out.astype(np.float32), pose, info)
    spread = 0.0
    for flags in (0, 1):                                       # the two inputs icp sees: the frames, and the frames centred
        _, pose_j, _ = rr.rigid_register64(frames, std, flags, svd='jacobi')
        spread = max(spread, float(np.abs(pose_j - ref[flags][1]).max()))
    bar = max(16.0 * spread, 1e-12)
    print('pose: spread between the two float64 SVDs %.3e, bar %.3e' % (spread, bar))
    return {'std': std, 'frames': frames, 'ref': ref, 'spread': spread, 'bar': bar}


def _launch(dev, frames, std, flags, want_pose=True, in_place=False, guard=64):
    """One apq_rigid_register call on guarded buffers: NaN behind out and pose.  Returns (out, pose or None) as numpy, after
    checking the guards."""
    from animateportrait_amd import _seqapi as Q, ops
    T = frames.shape[0]
    n = T * 204
    xin = torch.from_numpy(np.ascontiguousarray(frames)).to(dev).view(-1)
    sd = torch.from_numpy(np.ascontiguousarray(std)).to(dev)
    ob = torch.full((n + guard,), float('nan'), device=dev)
    if in_place:
        ob[:n] = xin
        xin = ob[:n]
    pb = torch.full((T * 12 + guard,), float('nan'), dtype=torch.float64, device=dev) if want_pose else None
    rc = Q.lib().apq_rigid_register(ops._ptr(xin), ops._ptr(sd), ops._ptr(ob), ops._ptr(pb), T, flags, ops._stream())
    Q.check(rc, 'rigid_register')
    torch.cuda.synchronize()
    assert bool(torch.isnan(ob[n:]).all()), 'out: the guard behind the rows was written'
    if want_pose:
        assert bool(torch.isnan(pb[T * 12:]).all()), 'pose: the guard behind the rows was written'
    return ob[:n].view(T, 204).cpu().numpy(), (pb[:T * 12].view(T, 12).cpu().numpy() if want_pose else None)


def _ulps(got, ref):
    """per frame: max |got - ref| in float32 ulps of the frame's largest |coordinate|"""
    ulp = np.spacing(np.abs(ref).max(axis=1)).astype(np.float64)
    return np.abs(got.astype(np.float64) - ref.astype(np.float64)).max(axis=1) / ulp


def _check(what, got, pose, pool, flags, rows):
    ref_out, ref_pose, _ = pool['ref'][flags]
    u = _ulps(got, ref_out[rows])
    line = '%s flags %d: out %.2f ulp at worst' % (what, flags, float(u.max()))
    if pose is not None:
        perr = float(np.abs(pose - ref_pose[rows]).max())
        line += ', pose err %.3e (bar %.3e)' % (perr, pool['bar'])
    print(line)
    assert float(u.max()) <= 1.0
    if pose is not None:
        assert perr <= pool['bar']


def test_symbols_are_bound_and_exported():
    from animateportrait_amd import _seqapi as Q
    for name in ('apq_rigid_register', 'apq_rigid_register_ok'):
        assert name in Q.SIGNATURES and hasattr(Q.lib(), name)
    assert Q.lib().apq_abi_version() == 1


def test_regular_inputs_are_well_conditioned(pool):
    """a condition on the inputs, met by the statement alone: S[1] > 1e-3 S[0] and |b| < 80 degrees for every frame used"""
    for flags in LEGAL_FLAGS:
        info = pool['ref'][flags][2]
        assert (info[:, 1] > 1e-3).all() and (info[:, 2] < 80.0).all()
    info = pool['ref'][0][2]
    assert info[0, 0] == 1 and (info[3:, 0] > 2).any()          # the standard face stops at once; regular frames need three rounds
    a = pool['frames'][1].astype(np.float64).reshape(68, 3)[list(rr.T_SHAPE_IDX)]
    b = pool['std'].astype(np.float64).reshape(68, 3)[list(rr.T_SHAPE_IDX)]
    u, _, vt = np.linalg.svd((a - a.mean(0)).T @ (b - b.mean(0)))
    assert np.linalg.det(vt.T @ u.T) < 0                        # the mirrored frame takes the reflection branch


@pytest.mark.parametrize('T', SIZES)
def test_sizes_against_the_statement(dev, pool, T):
    for flags in (3, 4):
        got, pose = _launch(dev, pool['frames'][:T], pool['std'], flags)
        _check('T = %d' % T, got, pose, pool, flags, slice(0, T))


def test_example_clip_length_and_position_in_the_clip(dev, pool):
    got, pose = _launch(dev, pool['frames'], pool['std'], 3)
    _check('T = 625', got, pose, pool, 3, slice(0, POOL_T))
    # a frame's result depends on neither T nor its row: the prefix run alone gives the same bits
    g130, p130 = _launch(dev, pool['frames'][:130], pool['std'], 3)
    assert np.array_equal(g130, got[:130]) and np.array_equal(p130, pose[:130])


def test_special_frames(dev, pool):
    got, pose = _launch(dev, pool['frames'][:3], pool['std'], 0)
    _check('specials', got, pose, pool, 0, slice(0, 3))
    assert np.array_equal(got, pool['frames'][:3])              # flags 0 copies the rows
    r_std = pose[0].reshape(3, 4)
    err = float(np.abs(r_std - np.hstack((np.eye(3), np.zeros((3, 1))))).max())
    print('the standard face onto itself: |[R | t] - [I | 0]| %.3e' % err)
    assert err <= pool['bar']
    r_mir = pose[1].reshape(3, 4)[:, :3]
    assert abs(np.linalg.det(r_mir) - 1.0) < 1e-12              # a rotation, although the best orthogonal fit is a reflection


@pytest.mark.parametrize('flags', LEGAL_FLAGS)
def test_flag_combinations_pose_and_in_place(dev, pool, flags):
    T = 65
    outs = []
    for want_pose in (True, False):
        for in_place in (False, True):
            got, pose = _launch(dev, pool['frames'][:T], pool['std'], flags, want_pose, in_place)
            _check('pose %d in place %d' % (want_pose, in_place), got, pose, pool, flags, slice(0, T))
            outs.append(got)
    for o in outs[1:]:
        assert np.array_equal(o, outs[0])


def test_position_independence(dev, pool):
    """one frame's rows are bit-equal at every position of a 130-frame clip, among copies of itself and among other frames"""
    frame = pool['frames'][11]
    alone, pose_alone = _launch(dev, frame.reshape(1, 204), pool['std'], 3)
    got, pose = _launch(dev, np.tile(frame, (130, 1)), pool['std'], 3)
    assert (got == alone).all() and (pose == pose_alone).all()
    for k in (0, 63, 64, 129):
        clip = pool['frames'][200:330].copy()
        clip[k] = frame
        got, pose = _launch(dev, clip, pool['std'], 3)
        assert np.array_equal(got[k], alone[0]) and np.array_equal(pose[k], pose_alone[0])


def test_hostile_frames_stay_in_their_rows(dev, pool):
    """a NaN frame, an all-equal frame and a frame at gimbal lock between regular frames: the kernel returns, the regular
    neighbours have the bits they have when run alone, and the guards behind out and pose stay (checked by _launch)"""
    std = pool['std']
    reg = pool['frames'][20:24]
    nan = np.full(204, np.nan, dtype=np.float32)
    equal = np.full(204, 0.25, dtype=np.float32)
    lock = (std.astype(np.float64).reshape(68, 3) @ rr.rot_xyz(0.0, np.pi / 2, 0.0)).reshape(204).astype(np.float32)
    clip = np.stack([reg[0], nan, reg[1], equal, reg[2], lock, reg[3]])
    for flags in LEGAL_FLAGS:
        got, pose = _launch(dev, clip, std, flags)
        alone, pose_alone = _launch(dev, reg, std, flags)
        assert np.array_equal(got[0::2], alone) and np.array_equal(pose[0::2], pose_alone)
        _check('hostile neighbours', got[0::2], pose[0::2], pool, flags, slice(20, 24))


def test_python_surface_on_device(dev, pool):
    from animateportrait_amd import landmark_post as lp, module1 as m1
    fl = torch.from_numpy(pool['frames'][:65]).to(dev)
    std = torch.from_numpy(pool['std']).to(dev)
    out, pose = lp.rigid_register(fl, std, center=True, no_x_rot=True, pose=True)
    assert out.shape == (65, 204) and pose.shape == (65, 3, 4) and pose.dtype == torch.float64
    _check('landmark_post.rigid_register', out.cpu().numpy(), pose.view(65, 12).cpu().numpy(), pool, 3, slice(0, 65))
    got = m1.stabilise_head(fl, std, centerize_face=True, no_y_rotation=True)
    assert torch.is_tensor(got) and got.is_cuda and torch.equal(got, out)
    assert m1.stabilise_head(fl, std) is fl
    reg = m1.register_face(fl[5], std)
    _check('module1.register_face', reg.view(1, 204).cpu().numpy(), None, pool, 4, slice(5, 6))
    with pytest.raises(RuntimeError, match='excludes'):
        lp.rigid_register(fl, std, center=True, register=True)


def test_clip_driver_with_both_switches_on_device(dev, golden):
    """predict_landmarks_speaker_aware with seeded networks: 'device' post backend and both switches against the numpy path"""
    from animateportrait_amd import module1 as m1
    from test_module1_gpu import _nets
    gd = golden('module1.npz')
    netc, netg = _nets(gd, dev)
    gp = torch.Generator().manual_seed(5)
    au = torch.randn(40, 18, 80, generator=gp)
    spk = torch.randn(256, generator=gp)
    fid = gd['fid'].view(-1)
    host = m1.predict_landmarks_speaker_aware(netg, netc, au, spk, fid, centerize_face=True, no_y_rotation=True)
    plain = m1.predict_landmarks_speaker_aware(netg, netc, au, spk, fid)
    prev = m1.set_post_backend('device')
    try:
        got = m1.predict_landmarks_speaker_aware(netg, netc, au, spk, fid, centerize_face=True, no_y_rotation=True)
    finally:
        m1.set_post_backend(prev)
    assert isinstance(host, np.ndarray) and host.dtype == np.float32 and torch.is_tensor(got) and got.is_cuda
    assert got.shape == host.shape == (40, 204)
    bar = 2e-5 * float(np.abs(host).max()) + 1e-6
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - host).max())
    moved = float(np.abs(host - plain).max())
    print('clip driver, device vs numpy with both switches: linf %.3e (bar %.3e); the switches moved the clip by %.3e' % (err, bar, moved))
    assert moved > 100 * bar                                    # the switches did something
    assert err <= bar
