"""CPU (-m "not gpu"): Module1's clip driver after its host statements moved to landmark_host -- the one segment loop of
``predict_landmarks_speaker_aware`` against the composition it replaced, spelt out here from landmark_host's primitives; the named
refusal of a clip without a segment; the four backend switches through their one helper; who imports whom; and the host
``segment_assemble`` against the three functions it is made of.  Every comparison is ``np.array_equal``."""
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

SWITCHES = [   # (the X of set_X_backend / get_X_backend, its variable, its tuple in module1, what its messages call it)
    ('lstm', 'APAMD_MODULE1_LSTM', 'LSTM_BACKENDS', 'LSTM'),
    ('lstm_train', 'APAMD_MODULE1_LSTM_TRAIN', 'LSTM_BACKENDS', 'LSTM'),
    ('encoder', 'APAMD_MODULE1_ENCODER', 'ENCODER_BACKENDS', 'encoder'),
    ('post', 'APAMD_MODULE1_POST', 'POST_BACKENDS', 'post-processing'),
]


def _clip(T):
    g = torch.Generator().manual_seed(100 + T)
    return torch.randn(T, 18, 80, generator=g), torch.randn(256, generator=g), torch.randn(204, generator=g) * 0.1


def _parent_host_loop(lh, net_g, net_c, au, spk, fid, segment, amp_pos=0.5, amp_lip_x=2.0, amp_lip_y=2.0, smooth_win=31, ratio=0.99):
    """The host loop as it stood before the two loops became one, statement for statement."""
    emb = spk.view(1, -1).expand(au.shape[0], -1)
    fid = fid.view(1, 204)
    out = []
    with torch.no_grad():
        for j in range(0, au.shape[0], segment):
            a, e = au[j:j + segment], emb[j:j + segment]
            if a.shape[0] < 10:
                continue
            z = torch.zeros(a.shape[0], 128)
            dis = net_g(a, e * 3.0, fid.repeat(a.shape[0], 1), None, z)[0].cpu().numpy()
            dis = lh._savgol(dis, int(min(dis.shape[0] - 1, smooth_win) // 2 * 2 + 1))
            dis = lh.close_pose_branch_mouth(dis, ratio).astype(np.float32) * np.float32(amp_pos)
            base = net_c(a[:, 0:18, :], fid)[0].cpu().numpy()
            seg = dis + lh.calib_baseline(base, amp_lip_x, amp_lip_y) + fid.cpu().numpy()
            out.append(lh.solve_inverse_lip(seg))
    fl = np.concatenate(out)
    fl[:, 27 * 3:28 * 3] = fl[:, 28 * 3:29 * 3] * 2 - fl[:, 29 * 3:30 * 3]
    return lh._savgol(fl, 5)


@pytest.fixture(scope='module')
def nets():
    from test_seq_lstm_cpu import _seeded_nets
    return _seeded_nets()


@pytest.mark.parametrize('T,segment,kept', [(40, 16, 32), (44, 16, 44), (12, 512, 12)])
def test_host_driver_equals_the_parents_composition(nets, T, segment, kept):
    """(40, 16): segments 16, 16 and a dropped 8; (44, 16): 16, 16 and a kept 12; (12, 512): one short segment.  The
    Savitzky-Golay windows are 15, 15 (, 11) and 11."""
    from animateportrait_amd import landmark_host as lh, module1 as m1
    netc, netg = nets
    au, spk, fid = _clip(T)
    assert m1.get_post_backend() == 'host'
    got = m1.predict_landmarks_speaker_aware(netg, netc, au, spk, fid, segment=segment)
    want = _parent_host_loop(lh, netg, netc, au, spk, fid, segment)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (kept, 204)
    assert want.dtype == np.float32 and np.array_equal(got, want)


def test_a_clip_without_a_segment_is_refused_by_name(nets):
    from animateportrait_amd import module1 as m1
    netc, netg = nets
    au, spk, fid = _clip(9)
    with pytest.raises(ValueError, match='predict_landmarks_speaker_aware: no segment of at least 10 windows'):
        m1.predict_landmarks_speaker_aware(netg, netc, au, spk, fid)


_SWITCH_PROBE = '''
import importlib, json, os, sys
name, var, values = sys.argv[1], sys.argv[2], json.loads(sys.argv[3])
res = {}
for v in values:
    os.environ.pop(var, None)
    if v is not None:
        os.environ[var] = v
    sys.modules.pop('animateportrait_amd.module1', None)
    try:
        m1 = importlib.import_module('animateportrait_amd.module1')
        res[str(v)] = getattr(m1, 'get_%s_backend' % name)()
    except ValueError as e:
        res[str(v)] = 'ValueError: %s' % e
print(json.dumps(res))
'''


@pytest.mark.parametrize('name,var,tup,what', SWITCHES)
def test_switch(name, var, tup, what):
    from animateportrait_amd import module1 as m1
    choices = getattr(m1, tup)
    get, set_ = getattr(m1, 'get_%s_backend' % name), getattr(m1, 'set_%s_backend' % name)
    # the variable, read when the module is imported: absent, each choice, an unknown name (one interpreter, a fresh import each)
    env = {k: v for k, v in os.environ.items() if not k.startswith('APAMD_MODULE1_')}
    got = subprocess.run([sys.executable, '-c', _SWITCH_PROBE, name, var, json.dumps([None] + list(choices) + ['nope'])], cwd=ROOT,
                         env=env, capture_output=True, text=True, timeout=240)
    assert got.returncode == 0, got.stderr
    res = json.loads(got.stdout.strip().split('\n')[-1])
    assert res['None'] == choices[0] and all(res[c] == c for c in choices)
    assert res['nope'] == "ValueError: Module1 %s backend 'nope' (known: %s)" % (what, ', '.join(choices))
    # set_* returns the previous value; a refused set_* leaves the value and names the known ones
    before = get()
    others = {n: getattr(m1, 'get_%s_backend' % n)() for n, _, _, _ in SWITCHES if n != name}
    try:
        for prev, new in zip((before,) + tuple(choices), tuple(choices) + (choices[0],)):
            assert set_(new) == prev and get() == new
            with pytest.raises(ValueError, match=r"Module1 %s backend 'nope' \(known: %s\)" % (what, ', '.join(choices))):
                set_('nope')
            assert get() == new
            assert {n: getattr(m1, 'get_%s_backend' % n)() for n in others} == others        # the other three stay
    finally:
        set_(before)
    assert get() == before


def test_module1_holds_no_second_home_for_the_moved_names():
    from animateportrait_amd import landmark_host as lh, module1 as m1
    for name in ('_savgol', 'close_pose_branch_mouth', 'calib_baseline', '_signed_area', 'solve_inverse_lip', 'blink_stamps',
                 'add_naive_eye', 'T_SHAPE_IDX', '_best_fit_transform', 'icp_t_shape'):
        assert hasattr(lh, name) and not hasattr(m1, name), name


def test_import_graph():
    code = ('import json, sys; import animateportrait_amd.%s; '
            'print(json.dumps(sorted(m for m in sys.modules if m == "animateportrait_amd.module1" or m.split(".")[0] == "scipy")[:3]))')
    for mod, allowed in (('landmark_post', ()), ('landmark_host', ('scipy',))):
        got = subprocess.run([sys.executable, '-c', code % mod], cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert got.returncode == 0, got.stderr
        seen = json.loads(got.stdout.strip().split('\n')[-1])
        assert [m for m in seen if m.split('.')[0] not in allowed] == [], (mod, seen)


@pytest.mark.parametrize('T', [2, 17])
@pytest.mark.parametrize('close,lip,nose', list(itertools.product((False, True), repeat=3)))
def test_host_segment_assemble_is_its_three_functions(T, close, lip, nose):
    from animateportrait_amd import landmark_host as lh
    from segment_inputs import segment_inputs as _segment_inputs
    dis, base, fid = _segment_inputs(T, [1] if T == 2 else [0, 5, 6, 16])
    if not close:
        dis = (dis + base + fid).astype(np.float32)              # the steps alone act on an assembled segment
    ratio, amp = 0.9, 0.5
    want = dis.copy()
    if close:
        want = lh.close_pose_branch_mouth(want, ratio).astype(np.float32) * np.float32(amp) + base + fid
    before_lip = want.copy()
    if lip:
        want = lh.solve_inverse_lip(want)
        assert not np.array_equal(want, before_lip)              # some frame was inverted: the step did something
    if nose:
        want[:, 81:84] = want[:, 84:87] * 2 - want[:, 87:90]
    keep = dis.copy()
    got = lh.segment_assemble(dis, base if close else None, fid if close else None, ratio, amp, close=close, lip=lip, nose=nose)
    assert got.dtype == np.float32 and np.array_equal(got, want) and np.array_equal(dis, keep)        # out of place
    rows = np.full((T + 2, 204), 7.0, dtype=np.float32)
    out = lh.segment_assemble(dis, base if close else None, fid if close else None, ratio, amp, close=close, lip=lip, nose=nose,
                              out=rows[1:T + 1])
    assert np.array_equal(rows[1:T + 1], want) and np.array_equal(out, want) and (rows[[0, -1]] == 7.0).all()
