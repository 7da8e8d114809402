"""CPU (-m "not gpu"): the rigid landmark registration -- its float64 statement (tests/register_reference.py) against the golden
the reference's own icp made (tests/golden/register.npz), the numpy twins of landmark_host (through module1) against the statement, every refusal of
apq_rigid_register_ok by name, ``module1_train --use_reg_as_std --std_face`` on a tiny dump, and the clip driver with both
head-stabilisation switches off."""
import argparse
import ctypes
import os
import pickle
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, GOLDEN

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, GOLDEN)
import register_reference as rr                                                     # noqa: E402

A = 0x10000000       # a stand-in address, aligned to everything the kernel asks for
ROWS = 204 * 4       # bytes of a frame
STD_TXT = os.path.join(GOLDEN, 'STD_FACE_LANDMARKS.txt')
NAMES = ('apq_rigid_register_ok', 'apq_rigid_register')


@pytest.fixture(scope='module')
def gold():
    z = np.load(os.path.join(GOLDEN, 'register.npz'))
    return {k: z[k] for k in z.files}


# ------------------------------------------------------------------------------------------------- statement and twins
def test_standard_face_fixture_is_the_goldens(gold):
    std = np.loadtxt(STD_TXT)
    assert std.shape == (68, 3) and np.array_equal(std.reshape(204).astype(np.float32), gold['std'])


@pytest.mark.parametrize('svd', ['lapack', 'jacobi'])
@pytest.mark.parametrize('flags', [0, 1, 2, 3, 4])
def test_statement_equals_the_references_own_icp(gold, flags, svd):
    out, pose = rr.rigid_register(gold['frames'], gold['std'], flags, svd)
    err = float(np.abs(pose - gold['pose_%d' % flags]).max())
    print('flags %d, %s: pose err %.3e' % (flags, svd, err))
    assert err <= 1e-12
    assert out.dtype == np.float32 and np.array_equal(out, gold['out_%d' % flags])


def test_statement_refuses_contradictory_flags(gold):
    for flags in (5, 6, 7, 8):
        with pytest.raises(ValueError):
            rr.rigid_register(gold['frames'][:1], gold['std'], flags)


def test_jacobi_svd_orders_and_signs_like_lapack():
    rng = np.random.RandomState(3)
    for k in range(40):
        h = rng.randn(3, 3) * (10.0 ** rng.uniform(-3, 3))
        if k % 4 == 0:
            h[:, 2] = h[:, 0] * 0.5 - h[:, 1]                    # rank 2: the third direction comes from the other two
        u, s, vt = rr.svd3_jacobi(h)
        s_ref = np.linalg.svd(h, compute_uv=False)
        assert s[0] >= s[1] >= s[2] >= 0 and np.abs(s - s_ref).max() <= 1e-13 * s_ref[0]
        assert np.abs(u @ np.diag(s) @ vt - h).max() <= 1e-13 * s_ref[0]
        assert np.abs(u.T @ u - np.eye(3)).max() <= 1e-13 and np.abs(vt @ vt.T - np.eye(3)).max() <= 1e-13


def test_numpy_twins_equal_the_statement(gold):
    from animateportrait_amd import landmark_host as lh, module1 as m1
    fl, std = gold['frames'], gold['std']
    assert lh.T_SHAPE_IDX == rr.T_SHAPE_IDX
    for centre, rot, flags in ((True, False, 1), (False, True, 2), (True, True, 3)):
        got = m1.stabilise_head(fl, std, centerize_face=centre, no_y_rotation=rot)
        assert got.dtype == np.float32 and got.shape == fl.shape and np.array_equal(got, rr.rigid_register(fl, std, flags)[0])
    assert m1.stabilise_head(fl, std) is fl                      # both off: nothing runs
    ref_out, ref_pose = rr.rigid_register(fl, std, 4)
    for i in range(fl.shape[0]):
        assert np.abs(lh.icp_t_shape(fl[i], std) - ref_pose[i].reshape(3, 4)).max() <= 1e-12
        got = m1.register_face(fl[i], std)
        assert got.dtype == np.float32 and np.array_equal(got, ref_out[i])
    # a torch tensor on the CPU is served like an array
    got = m1.stabilise_head(torch.from_numpy(fl), torch.from_numpy(std), True, True)
    assert isinstance(got, np.ndarray) and np.array_equal(got, rr.rigid_register(fl, std, 3)[0])


# ------------------------------------------------------------------------------------------------------------- the C ABI
def test_symbols_in_header_binding_and_library_with_equal_signatures():
    from animateportrait_amd import _seqapi
    hdr = open(os.path.join(ROOT, 'include', 'animateportrait_seq.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    ctype = {'int32_t': ctypes.c_int32, 'int': ctypes.c_int, 'void*': ctypes.c_void_p, 'float*': ctypes.c_void_p,
             'const float*': ctypes.c_void_p, 'double*': ctypes.c_void_p, 'const double*': ctypes.c_void_p}
    lib = _seqapi.lib()
    for name in NAMES:
        m = re.search(r'(\w+)\s+%s\s*\(([^)]*)\)\s*;' % name, code)
        assert m, name
        args = [re.sub(r'\s*\w+$', '', a.strip()) for a in m.group(2).split(',')]
        res, argtypes = _seqapi.SIGNATURES[name]
        assert res is ctype[m.group(1)] and argtypes == [ctype[a] for a in args] and hasattr(lib, name), name
    assert _seqapi.SIGNATURES[NAMES[1]][1] == _seqapi.SIGNATURES[NAMES[0]][1] + [ctypes.c_void_p]
    assert int(re.search(r'#define\s+APQ_ABI_VERSION\s+(\d+)', hdr).group(1)) == 1 == lib.apq_abi_version()
    for macro, value in (('APQ_REG_CENTER', _seqapi.REG_CENTER), ('APQ_REG_NO_X_ROT', _seqapi.REG_NO_X_ROT),
                         ('APQ_REG_REGISTER', _seqapi.REG_REGISTER), ('APQ_REG_MAX_ROUNDS', _seqapi.REG_MAX_ROUNDS)):
        assert int(re.search(r'#define\s+%s\s+(\d+)' % macro, hdr).group(1)) == value


def _ok(inp=A, std=A - 4096, out=A + 0x1000000, pose=A + 0x2000000, T=130, flags=3):
    from animateportrait_amd import _seqapi
    return _seqapi.lib().apq_rigid_register_ok(inp, std, out, pose, T, flags)


@pytest.mark.parametrize('kw', [dict(), dict(T=1), dict(T=65536, pose=None, out=A), dict(flags=0), dict(flags=1), dict(flags=2),
                                dict(flags=4), dict(pose=None), dict(out=A), dict(out=A + 130 * ROWS), dict(out=A - 130 * ROWS, std=8)])
def test_ok_twin_serves(kw):
    from animateportrait_amd import _seqapi
    assert _ok(**kw) == 1, _seqapi.last_error()


@pytest.mark.parametrize('kw,reason', [
    (dict(inp=None), 'null in'), (dict(std=None), 'null std'), (dict(out=None), 'null out'),
    (dict(T=0), 'T = 0'), (dict(T=-1), 'T = -1'), (dict(T=65537), 'T = 65537'),
    (dict(flags=8), 'unknown flags = 8'), (dict(flags=16 | 3), 'unknown flags = 19'), (dict(flags=-1), 'unknown flags'),
    (dict(flags=5), 'excludes'), (dict(flags=6), 'excludes'), (dict(flags=7), 'excludes'),
    (dict(inp=A + 2), 'in is not 4-byte'), (dict(std=A - 4095), 'std is not 4-byte'), (dict(out=A + 0x1000001), 'out is not 4-byte'),
    (dict(pose=A + 0x2000004), 'pose is not 8-byte'),
    (dict(out=A + ROWS), 'out overlaps in'), (dict(out=A - 4), 'out overlaps in'), (dict(out=A + 130 * ROWS - 4), 'out overlaps in'),
    (dict(std=A + 0x1000000 + 8), 'out overlaps std'), (dict(pose=A + 0x1000000 + 8), 'pose overlaps out'),
    (dict(pose=A + 8), 'pose overlaps in'), (dict(pose=A - 4096, T=1), 'pose overlaps std'),
])
def test_ok_twin_refuses_and_names_the_reason(kw, reason):
    from animateportrait_amd import _seqapi
    assert _ok() == 1
    assert _ok(**kw) == 0
    assert 'rigid_register' in _seqapi.last_error() and reason in _seqapi.last_error(), _seqapi.last_error()


def test_launching_call_refuses_without_launching():
    from animateportrait_amd import _seqapi
    lib = _seqapi.lib()
    assert lib.apq_rigid_register(A, A - 4096, A + ROWS, None, 130, 3, None) == _seqapi.ERR_INVALID
    assert lib.apq_rigid_register(A, A - 4096, A, None, 65537, 3, None) == _seqapi.ERR_UNSUPPORTED
    assert lib.apq_rigid_register(A, A - 4096, A, None, 130, 5, None) == _seqapi.ERR_INVALID


def test_device_entry_point_takes_cuda_tensors_only(gold):
    from animateportrait_amd import landmark_post as lp
    with pytest.raises(TypeError, match='CUDA'):
        lp.rigid_register(torch.from_numpy(gold['frames']), torch.from_numpy(gold['std']), center=True)


# ------------------------------------------------------------------------------------------------------------ the trainer
def _write_dump(dump_dir, frames, n_frames=60):
    """a dump in the layout main_end2end_module2.py:230-251 writes, one clip per status: the golden's frames in turn, the lips
    of frame 20 closed so that the identity frame (picked among every tenth frame) is known"""
    rng = np.random.RandomState(0)
    os.makedirs(dump_dir, exist_ok=True)
    fl = np.stack([frames[k % 24] for k in range(n_frames)]).astype(np.float64)
    pts = fl[20].reshape(68, 3)
    pts[60:68, 1] = pts[60, 1]                                                       # inner lip on one line in x, y: no area
    info = (0, 'clip0.wav', np.zeros(256))
    for status in ('train', 'test'):
        for kind, data in (('au', [(rng.randn(n_frames, 80), info)]), ('fl', [(fl, info)])):
            with open(os.path.join(dump_dir, 'autovc_retrain_mel_%s_%s.pickle' % (status, kind)), 'wb') as fp:
                pickle.dump(data, fp)
    return fl[20].astype(np.float32)


def test_trainer_registers_the_identity_frame(gold, tmp_path, monkeypatch):
    from animateportrait_amd import module1_train as mt
    d, ck = str(tmp_path / 'dump'), str(tmp_path / 'ckpt')
    picked = _write_dump(d, gold['frames'])
    want = rr.rigid_register(picked.reshape(1, 204), gold['std'], 4)[0]
    # (the frame differs from the golden's frame 20 only in its inner lip, which the T shape does not contain: the same T)
    assert np.abs(rr.rigid_register64(picked.reshape(1, 204), gold['std'], 4)[1] - gold['pose_4'][20]).max() <= 1e-12
    seen = []
    inner = mt.ContentTrainer.train_content

    def spy(self, fls, aus, face_id, is_training=True):
        seen.append(face_id.detach().cpu().numpy().copy())
        return inner(self, fls, aus, face_id, is_training)
    monkeypatch.setattr(mt.ContentTrainer, 'train_content', spy)
    argv = ['--dump_dir', d, '--ckpt_dir', ck, '--nepoch', '1', '--device', 'cpu', '--seed', '2']
    assert mt.main(argv + ['--use_reg_as_std', '--std_face', STD_TXT]) == 0
    assert len(seen) == 2 and os.path.exists(os.path.join(ck, 'ckpt_last_epoch.pth'))         # one training, one eval segment
    for face_id in seen:
        assert face_id.dtype == np.float32 and np.array_equal(face_id, want)
    # without the flag the identity frame is the picked frame itself, as before
    del seen[:]
    assert mt.main(argv) == 0
    for face_id in seen:
        assert np.array_equal(face_id, picked.reshape(1, 204))
    # one golden frame through the trainer's own method
    tr = mt.ContentTrainer(mt.make_parser().parse_args(argv + ['--use_reg_as_std', '--std_face', STD_TXT]), device='cpu')
    got = tr.registered_face_id(torch.from_numpy(gold['frames'][3:4]))
    assert np.array_equal(got.numpy(), gold['out_4'][3:4])


def test_flag_alone_is_still_refused(tmp_path):
    from animateportrait_amd import module1_train as mt
    with pytest.raises(SystemExit, match='use_reg_as_std'):
        mt.main(['--dump_dir', str(tmp_path), '--ckpt_dir', str(tmp_path), '--nepoch', '1', '--use_reg_as_std'])
    with pytest.raises(NotImplementedError, match='use_reg_as_std'):
        mt.ContentTrainer(argparse.Namespace(use_reg_as_std=True))
    with pytest.raises(NotImplementedError, match='std_face'):
        mt.ContentTrainer(argparse.Namespace(use_reg_as_std=True, std_face=None))
    bad = tmp_path / 'short.txt'
    bad.write_text('1 2 3\n')
    with pytest.raises(ValueError, match='68 x 3'):
        mt.load_std_face(str(bad))


# -------------------------------------------------------------------------------------------------------- the clip driver
def test_clip_driver_with_the_switches_off_is_unchanged(golden, monkeypatch):
    from animateportrait_amd import landmark_host as lh, module1 as m1
    from test_stream_cpu import _seeded
    gd = golden('module1.npz')
    netc = _seeded(m1.Audio2LandmarkContent(use_prior_net=True, drop_out=0.5), gd, 'c_', 78)
    netg = _seeded(m1.Audio2LandmarkPos(drop_out=0.5), gd, 'g_', 79)
    gp = torch.Generator().manual_seed(5)
    au, spk, fid = torch.randn(40, 18, 80, generator=gp), torch.randn(256, generator=gp), gd['fid'].view(-1)
    on = m1.predict_landmarks_speaker_aware(netg, netc, au, spk, fid, centerize_face=True, no_y_rotation=True)
    # with both switches off nothing of the registration runs: the twins may not even be reached past their first line
    monkeypatch.setattr(lh, 'icp_t_shape', lambda *a, **k: pytest.fail('icp ran with the switches off'))
    plain = m1.predict_landmarks_speaker_aware(netg, netc, au, spk, fid)
    off = m1.predict_landmarks_speaker_aware(netg, netc, au, spk, fid, centerize_face=False, no_y_rotation=False)
    assert plain.dtype == off.dtype == np.float32 and plain.shape == (40, 204) and np.array_equal(plain, off)
    # ... and the switches are the statement applied to that output
    assert np.array_equal(on, rr.rigid_register(plain, fid.numpy(), 3)[0])
    assert np.abs(on - plain).max() > 1e-3


def test_end2end_parser_carries_the_references_names():
    from animateportrait_amd import end2end
    ap = end2end.make_parser()
    a = ap.parse_args(['--photo', 'p.png', '--out', 'o'])
    assert a.centerize_face is False and a.no_y_rotation is False
    a = ap.parse_args(['--photo', 'p.png', '--out', 'o', '--centerize_face', '--no_y_rotation'])
    assert a.centerize_face is True and a.no_y_rotation is True
    text = ap.format_help()
    assert 'about the x axis' in re.sub(r'\s+', ' ', text)
