"""GPU (-m gpu): Module1's clip-level landmark post-processing on the device (landmark_post.py over the apq_* calls of
libapseq.so, csrc/seq/seq_post.hip) against the host functions it restates -- scipy's savgol_filter, landmark_host.calib_baseline,
close_pose_branch_mouth / solve_inverse_lip, add_naive_eye, stream.smooth_landmarks -- then the whole stage against the
reference-made golden (tests/golden/module1.npz) and the frame loop fed the device sequence.

Bar wherever a float64 reference exists: 2e-5 max|ref| + 1e-6, the form and size test_module1_gpu.py uses for this stage.  Every
case prints the L-inf it measured."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
from segment_inputs import segment_inputs as _segment_inputs           # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 777.0


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


def _bar(ref):
    return 2e-5 * float(np.abs(ref).max()) + 1e-6


def _report(what, got, ref):
    err = float(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64)).max())
    print('%s: linf %.3e (bar %.3e, max|ref| %.3e)' % (what, err, _bar(ref), float(np.abs(ref).max())))
    return err


def _guarded(x_np, dev):
    """x on the device with NaN right behind it, and an output buffer of sentinels with room behind it as well"""
    n = x_np.size
    xb = torch.full((n + 256,), float('nan'), device=dev)
    xb[:n] = torch.from_numpy(x_np.reshape(-1)).to(dev)
    yb = torch.full((n + 256,), SENTINEL, device=dev)
    return xb, xb[:n].view(x_np.shape), yb, yb[:n].view(x_np.shape)


# ------------------------------------------------------------------------------------------------------------ Savitzky-Golay
@pytest.mark.parametrize('T,C,W', [(5, 3, 5), (9, 204, 9), (10, 204, 9), (31, 7, 31), (113, 204, 31), (512, 204, 31)])
def test_savgol_matches_scipy(dev, T, C, W):
    from scipy.signal import savgol_filter
    from animateportrait_amd import landmark_post as lp
    x = (np.random.RandomState(T + W).randn(T, C) * 3 + 1).astype(np.float32)
    ref = savgol_filter(x.astype(np.float64), W, 3, axis=0)
    xb, xv, yb, yv = _guarded(x, dev)
    lp._savgol_into(xv, yv, 0, C, C, W, 0)
    assert _report('savgol T %d C %d W %d' % (T, C, W), yv.cpu().numpy(), ref) <= _bar(ref)
    # nothing behind y was written, and the NaN behind x was not read into any output
    assert bool((yb[T * C:] == SENTINEL).all()) and bool(torch.isfinite(yv).all())
    assert bool(torch.isnan(xb[T * C:]).all()) and np.array_equal(xv.cpu().numpy(), x)
    # the public function is the same launch
    assert torch.equal(lp.savgol(xv, W), yv)


def test_savgol_column_split_is_the_clip_smoothing(dev):
    """(625, 204) with window 15 on the columns [0, 144) and 5 on the rest: range by range (the columns outside a call's range
    stay untouched), then as the one call smooth_landmarks makes, against stream.smooth_landmarks (float64 inside)."""
    from scipy.signal import savgol_filter
    from animateportrait_amd import landmark_post as lp, stream
    T, C = 625, 204
    x = (np.random.RandomState(625).randn(T, C) * 40 + 128).astype(np.float32)
    x64 = x.astype(np.float64)
    ref = np.concatenate([savgol_filter(x64[:, :144], 15, 3, axis=0), savgol_filter(x64[:, 144:], 5, 3, axis=0)], 1)
    xb, xv, yb, yv = _guarded(x, dev)
    lp._savgol_into(xv, yv, 0, 144, 144, 15, 0)
    assert bool((yv[:, 144:] == SENTINEL).all()) and bool((yb[T * C:] == SENTINEL).all())
    assert _report('savgol split, wide range alone', yv[:, :144].cpu().numpy(), ref[:, :144]) <= _bar(ref)
    yb.fill_(SENTINEL)
    lp._savgol_into(xv, yv, 144, 144, 204, 0, 5)
    assert bool((yv[:, :144] == SENTINEL).all()) and bool((yb[T * C:] == SENTINEL).all())
    assert _report('savgol split, lip range alone', yv[:, 144:].cpu().numpy(), ref[:, 144:]) <= _bar(ref)
    yb.fill_(SENTINEL)
    lp._savgol_into(xv, yv, 3, 144, 201, 15, 5)                 # an inner range: a point on either side stays as it was
    got = yv.cpu().numpy()
    assert (got[:, :3] == SENTINEL).all() and (got[:, 201:] == SENTINEL).all() and bool((yb[T * C:] == SENTINEL).all())
    assert np.abs(got[:, 3:201] - ref[:, 3:201]).max() <= _bar(ref)
    yb.fill_(SENTINEL)
    lp._savgol_into(xv, yv, 0, 144, 204, 15, 5)
    assert _report('savgol split, one call', yv.cpu().numpy(), ref) <= _bar(ref)
    assert bool((yb[T * C:] == SENTINEL).all())
    host = stream.smooth_landmarks(x.reshape(T, 68, 3))
    out = lp.smooth_landmarks(xv.view(T, 68, 3))
    assert out.is_cuda and out.shape == (T, 68, 3) and torch.equal(out.view(T, C), yv)
    assert _report('smooth_landmarks', out.cpu().numpy(), host) <= _bar(host)
    # a clip too short for the wide window keeps those columns, as on the host
    short = lp.smooth_landmarks(xv[:9].view(9, 68, 3))
    host9 = stream.smooth_landmarks(x[:9].reshape(9, 68, 3))
    assert np.array_equal(short.cpu().numpy()[:, :48], x[:9].reshape(9, 68, 3)[:, :48])
    assert _report('smooth_landmarks, 9 frames', short.cpu().numpy(), host9) <= _bar(host9)


# ------------------------------------------------------------------------------------------------------------ calib_baseline
def _calib_ref64(x, ratio, ax=2.0, ay=2.0):
    x = np.asarray(x, dtype=np.float64)
    k = int(x.shape[0] * ratio)
    y = x - np.sort(x, axis=0)[:k].mean(0, keepdims=True)
    y[:, 144::3] *= ax
    y[:, 145::3] *= ay
    return y


@pytest.mark.parametrize('T', [10, 11, 113, 512])
@pytest.mark.parametrize('ratio', [0.5, 0.25])
@pytest.mark.parametrize('negative', [False, True])
def test_calib_baseline_matches_host(dev, T, ratio, negative):
    """Against the float64 statement of the operation (bar) and the host function itself (fp32 inside: the same bar around
    it).  Column 3 is constant, column 7 and the mouth column 148 hold every value twice (ties across the k boundary)."""
    from animateportrait_amd import landmark_host as lh, landmark_post as lp
    rs = np.random.RandomState(T)
    x = rs.randn(T, 204).astype(np.float32)
    x[:, 3] = 1.25
    for c in (7, 148):
        x[:, c] = rs.permutation(np.repeat(rs.randn((T + 1) // 2), 2)[:T]).astype(np.float32)
    if negative:
        x = -np.abs(x) - 0.5
    ref = _calib_ref64(x, ratio, 2.0, 1.5)
    host = lh.calib_baseline(x.astype(np.float64), 2.0, 1.5, ratio)
    xb, xv, yb, yv = _guarded(x, dev)
    from animateportrait_amd import _seqapi as Q, ops
    Q.check(Q.lib().apq_calib_baseline(ops._ptr(xv), ops._ptr(yv), T, int(T * ratio), 2.0, 1.5, ops._stream()), 'calib_baseline')
    got = yv.cpu().numpy()
    assert _report('calib_baseline T %d ratio %.2f%s' % (T, ratio, ' negative' if negative else ''), got, ref) <= _bar(ref)
    assert np.abs(got.astype(np.float64) - host).max() <= _bar(ref)
    assert bool((yb[T * 204:] == SENTINEL).all()) and np.isfinite(got).all()
    assert torch.equal(lp.calib_baseline(xv, 2.0, 1.5, ratio), yv)
    if not negative:
        assert np.abs(got[:, 3]).max() <= 1e-6                  # the constant column becomes zero


# ---------------------------------------------------------------------------------------------------------- segment assembly
@pytest.mark.parametrize('T', [10, 113, 512])
@pytest.mark.parametrize('which', ['first', 'second', 'last', 'run', 'none'])
def test_segment_assemble_matches_host(dev, T, which):
    """close_pose_branch_mouth x amp + base + fid, then solve_inverse_lip, in one launch against the host statements on the same
    fp32 inputs.  Observed on the MI355X: all fifteen cases are bit equal to the host (L-inf 0): the kernel keeps numpy's fp32
    operation order and is built without multiply-add contraction.  The assertion is the bar all the same."""
    from animateportrait_amd import landmark_host as lh, landmark_post as lp
    inverted = {'first': [0], 'second': [1], 'last': [T - 1], 'run': [5, 6, 7], 'none': []}[which]
    dis, base, fid = _segment_inputs(T, inverted)
    ratio, amp = 0.99, 0.5
    seg = lh.close_pose_branch_mouth(dis.copy(), ratio).astype(np.float32) * np.float32(amp) + base + fid
    assert seg.dtype == np.float32
    areas = np.array([lh._signed_area(seg[j].reshape(68, 3)[60:68, 0:2]) for j in range(T)])
    # the condition of the comparison: no frame's branch can flip on rounding, and the inverted frames are the intended ones
    assert np.abs(areas).min() >= 1e-4 and sorted(np.nonzero(areas < 0)[0].tolist()) == inverted
    ref = lh.solve_inverse_lip(seg.copy())
    assert (len(inverted) > 0) == (not np.array_equal(ref, seg))
    d, b, f = (torch.from_numpy(a).to(dev) for a in (dis, base, fid))
    got = lp.segment_assemble(d, b, f, ratio, amp, close=True, lip=True, nose=False).cpu().numpy()
    err = _report('segment T %d inverted %s (bit equal: %s)' % (T, which, np.array_equal(got, ref)), got, ref)
    assert err <= _bar(ref)
    # the nose-top flag changes point 27 alone
    nose = lp.segment_assemble(d, b, f, ratio, amp, close=True, lip=True, nose=True).cpu().numpy()
    want = ref.copy()
    want[:, 81:84] = ref[:, 84:87] * 2 - ref[:, 87:90]
    assert np.abs(nose - want).max() <= _bar(ref)
    assert np.array_equal(np.delete(nose, [81, 82, 83], 1), np.delete(got, [81, 82, 83], 1))


def test_segment_steps_alone_match_host(dev):
    from animateportrait_amd import landmark_host as lh, landmark_post as lp
    dis, base, fid = _segment_inputs(113, [4, 5, 40])
    seg = (dis + base + fid).astype(np.float32)
    t = torch.from_numpy(seg).to(dev)
    keep = t.clone()
    ref = lh.close_pose_branch_mouth(seg.copy(), 0.9)
    assert _report('close_pose_branch_mouth', lp.close_pose_branch_mouth(t, 0.9).cpu().numpy(), ref) <= _bar(ref)
    ref = lh.solve_inverse_lip(seg.copy())
    assert not np.array_equal(ref, seg)
    assert _report('solve_inverse_lip', lp.solve_inverse_lip(t).cpu().numpy(), ref) <= _bar(ref)
    assert torch.equal(t, keep)                                  # out of place


# ------------------------------------------------------------------------------------------------------------------- eyes
@pytest.mark.parametrize('T', [46, 200])
def test_add_naive_eye_matches_host(dev, T):
    """T = 46: the single blink at frame 30, whose ramp reaches the last frame; T = 200: two blinks with RandomState(0)."""
    from animateportrait_amd import landmark_host as lh, landmark_post as lp
    x = (np.random.RandomState(T).randn(T, 68, 3) * 30 + 128).astype(np.float32)
    ref = lh.add_naive_eye(x.astype(np.float64), np.random.RandomState(0))
    assert len(lh.blink_stamps(T, np.random.RandomState(0))) == (1 if T == 46 else 2)
    t = torch.from_numpy(x).to(dev)
    got = lp.add_naive_eye(t, np.random.RandomState(0))
    assert got.is_cuda and got.shape == (T, 68, 3) and np.array_equal(t.cpu().numpy(), x)
    assert _report('add_naive_eye T %d' % T, got.cpu().numpy(), ref) <= _bar(ref)
    lids = [37, 38, 40, 41, 43, 44, 46, 47]
    assert np.array_equal(np.delete(got.cpu().numpy(), lids, 1), np.delete(x, lids, 1))


def test_add_naive_eye_refuses_45_frames_before_launching(dev, monkeypatch):
    from animateportrait_amd import landmark_post as lp, module1 as m1

    def no_library():
        raise AssertionError('the library was reached')
    t = torch.zeros(45, 68, 3, device=dev)
    flat = torch.zeros(45, 204, device=dev)
    monkeypatch.setattr(lp.Q, 'lib', no_library)
    rng = np.random.RandomState(0)
    state = rng.get_state()[1].copy()
    with pytest.raises(ValueError, match='45 frames'):
        lp.add_naive_eye(t, rng)
    with pytest.raises(ValueError, match='45 frames'):
        lp.to_image_landmarks(flat, rng=rng)
    with pytest.raises(ValueError, match='45 frames'):
        m1.to_image_landmarks(flat, rng=rng)
    assert np.array_equal(rng.get_state()[1], state)             # and nothing was drawn


# ------------------------------------------------------------------------------------------------------------ the whole stage
@pytest.fixture(scope='module')
def stage(dev, golden):
    """The golden's 600-window loop through both backends, once: host first with the switch untouched, then device, then host
    again."""
    from animateportrait_amd import module1 as m1
    from test_module1_gpu import _nets
    gd = golden('module1.npz')
    netc, netg = _nets(gd, dev)
    gp = torch.Generator().manual_seed(int(gd['p_seed']))
    au = torch.randn(int(gd['p_T']), 18, 80, generator=gp)
    spk = torch.randn(256, generator=gp)
    fid = gd['fid'].view(-1)

    def run():
        fl = m1.predict_landmarks_speaker_aware(netg, netc, au, spk, fid)
        return fl, m1.to_image_landmarks(fl, scale=0.01, shift=(-128.0, -120.0), rng=np.random.RandomState(0))
    assert m1.get_post_backend() == 'host'
    res = {'untouched': run()}
    prev = m1.set_post_backend('device')
    try:
        res['device'] = run()
    finally:
        m1.set_post_backend(prev)
    assert m1.get_post_backend() == 'host'
    res['host'] = run()
    res['p_sub'] = gd['p_sub'].numpy()
    return res


def test_stage_on_device_matches_reference_golden(stage):
    fl, img = stage['device']
    assert torch.is_tensor(fl) and fl.is_cuda and fl.dtype == torch.float32 and fl.shape == (600, 204)
    assert torch.is_tensor(img) and img.is_cuda and img.dtype == torch.float32 and img.shape == (600, 68, 3)
    ref = stage['p_sub']
    err = float(np.abs(fl.cpu().numpy()[::16] - ref).max())
    print('stage vs golden: linf %.3e (bar %.3e)' % (err, 1e-4 * np.abs(ref).max()))
    assert err < 1e-4 * np.abs(ref).max()
    host_fl, host_img = stage['host']
    _report('stage, device vs host landmarks', fl.cpu().numpy(), host_fl)
    assert _report('to_image_landmarks, device on device vs host on host', img.cpu().numpy(), host_img) <= _bar(host_img)


def test_stage_host_backend_is_unchanged(stage):
    for a, b in zip(stage['untouched'], stage['host']):
        assert isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == np.float32 and np.array_equal(a, b)
    assert stage['host'][0].shape == (600, 204) and stage['host'][1].shape == (600, 68, 3)
    ref = stage['p_sub']
    assert np.abs(stage['host'][0][::16] - ref).max() < 1e-4 * np.abs(ref).max()


def test_predict_landmarks_content_branch_on_device(dev, golden):
    from animateportrait_amd import module1 as m1
    from test_module1_gpu import _nets
    gd = golden('module1.npz')
    netc, _ = _nets(gd, dev)
    au = torch.randn(40, 18, 80, generator=torch.Generator().manual_seed(2))
    host = m1.predict_landmarks(netc, au, gd['fid'].view(-1), scale=0.01, shift=(-128.0, -120.0))
    prev = m1.set_post_backend('device')
    try:
        got = m1.predict_landmarks(netc, au, gd['fid'].view(-1), scale=0.01, shift=(-128.0, -120.0))
    finally:
        m1.set_post_backend(prev)
    assert isinstance(host, np.ndarray) and torch.is_tensor(got) and got.is_cuda and got.shape == host.shape == (40, 68, 2)
    assert _report('predict_landmarks', got.cpu().numpy(), host) <= _bar(host)


@pytest.mark.parametrize('T,segment,kept', [(40, 16, 32), (44, 16, 44)])
def test_one_segment_loop_on_device_keeps_the_hosts_rows(dev, golden, T, segment, kept):
    """The clip driver's one loop with the 'device' backend on short segments: 16, 16 and a dropped 8; 16, 16 and a kept 12.
    Compared with the host backend as test_stage_on_device_matches_reference_golden does (no eyes: fewer than 46 rows)."""
    from animateportrait_amd import module1 as m1
    from test_module1_gpu import _nets
    gd = golden('module1.npz')
    netc, netg = _nets(gd, dev)
    g = torch.Generator().manual_seed(T)
    au, spk, fid = torch.randn(T, 18, 80, generator=g), torch.randn(256, generator=g), gd['fid'].view(-1)

    def run():
        fl = m1.predict_landmarks_speaker_aware(netg, netc, au, spk, fid, segment=segment)
        return fl, m1.to_image_landmarks(fl, scale=0.01, shift=(-128.0, -120.0), eyes=False, rng=np.random.RandomState(0))
    host_fl, host_img = run()
    prev = m1.set_post_backend('device')
    try:
        fl, img = run()
    finally:
        m1.set_post_backend(prev)
    assert isinstance(host_fl, np.ndarray) and host_fl.shape == (kept, 204)
    assert torch.is_tensor(fl) and fl.is_cuda and fl.dtype == torch.float32 and fl.shape == (kept, 204)
    assert torch.is_tensor(img) and img.is_cuda and img.shape == (kept, 68, 3)
    _report('one loop T %d segment %d, device vs host landmarks' % (T, segment), fl.cpu().numpy(), host_fl)
    assert _report('one loop T %d segment %d, image landmarks' % (T, segment), img.cpu().numpy(), host_img) <= _bar(host_img)


# ------------------------------------------------------------------------------------------------------------- end to end
def test_clip_streamer_takes_the_device_sequence(dev, golden):
    """mel windows -> Module1 with post-processing on the device -> ClipStreamer(triangulate='device'): the frames of the
    device sequence are those of the same sequence handed over after .cpu()."""
    import contextlib
    import io
    from animateportrait_amd import audio, module1 as m1, stream
    from animateportrait_amd.options.base_options import TestOptions
    from animateportrait_amd.models import create_model
    from animateportrait_amd.synthetic import make_landmarks
    from test_module1_gpu import _nets
    gd = golden('module1.npz')
    netc, netg = _nets(gd, dev)
    w = audio.clip_audio_features(os.path.join(GOLDEN, 'female12.wav'), max_frames=64)
    spk = torch.randn(256, generator=torch.Generator().manual_seed(3))
    prev = m1.set_post_backend('device')
    try:
        fl = m1.predict_landmarks_speaker_aware(netg, netc, w, spk, gd['fid'].view(-1))
        img = m1.to_image_landmarks(fl, scale=0.01, shift=(-128.0, -128.0), rng=np.random.RandomState(0))[:, :, :2]
    finally:
        m1.set_post_backend(prev)
    assert img.is_cuda and img.shape == (64, 68, 2)
    lm0 = make_landmarks(1, torch.Generator().manual_seed(9))[0]
    seq = (lm0.to(dev)[None] + torch.clamp(img - img.mean(0, keepdim=True), -6.0, 6.0))[:24].contiguous()
    opt = TestOptions().parse(['--model', 'geomcgt_ifw_test', '--netG', 'resnet_9blocks_rcatland32_full_ifw',
                               '--dataset_mode', 'synthetic', '--name', 'drawing_stream', '--output_nc', '1', '--ngf', '8',
                               '--netg_resb_div', '3', '--netg_resb_disp', '3', '--gpu_ids', '0'])
    with contextlib.redirect_stdout(io.StringIO()):
        torch.manual_seed(1)
        model = create_model(opt)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, 256), torch.linspace(-1, 1, 256), indexing='ij')
    photo = torch.stack([torch.sin(3 * xx + yy), torch.cos(2 * yy - xx), xx * yy], 0).unsqueeze(0).contiguous()
    matte = (((yy / 0.8) ** 2 + (xx / 0.6) ** 2) < 1).float().view(1, 1, 256, 256)
    frames = stream.ClipStreamer(model, batch=16, triangulate='device').run(photo, lm0, seq, matte=matte)
    assert frames.shape == (24, 1, 256, 256) and bool(torch.isfinite(frames).all()) and float(frames.std()) > 1e-3
    frames_cpu = stream.ClipStreamer(model, batch=16, triangulate='device').run(photo, lm0, seq.cpu(), matte=matte)
    assert torch.equal(frames, frames_cpu)


def test_end2end_cli_with_post_on_device(dev, golden, tmp_path, monkeypatch):
    """``end2end --wav ... --module1_post device`` (the set-up of test_end2end_cli_from_wav): with --triangulate device the
    sequence goes to the frame loop as it is, with --triangulate host it crosses once.  Observed with a third run on the host
    backend (--triangulate device): its frames differ from the device backend's by 3.5e-5 grey levels on average, at most 1."""
    from PIL import Image
    from animateportrait_amd import autovc, end2end, module1 as m1
    from animateportrait_amd.synthetic import make_landmarks
    from oracle import generator as og, static_generator as osg
    from test_module1_gpu import _nets
    gd = golden('module1.npz')
    netc, netg = _nets(gd, torch.device('cpu'))
    monkeypatch.chdir(tmp_path)
    os.makedirs('checkpoints/e2e'); os.makedirs('checkpoints/static'); os.makedirs('m1')
    torch.save({'G': netg.state_dict()}, 'm1/g.pth')
    torch.save({'model_g_face_id': netc.state_dict()}, 'm1/c.pth')
    torch.save(og.init_params(og.generator_param_shapes(3, 1, 8, 9, 3, 3), seed=1234), 'checkpoints/e2e/7_net_G_A.pth')
    torch.save(og.init_params(osg.static_param_shapes(3, 1, 64), seed=4321), 'checkpoints/static/drawing.pth')
    yy, xx = np.meshgrid(np.linspace(-1, 1, 256), np.linspace(-1, 1, 256), indexing='ij')
    Image.fromarray(((np.stack([np.sin(3 * xx + yy), np.cos(2 * yy - xx), xx * yy], -1) + 1) * 127.5).astype(np.uint8)).save('photo.png')
    Image.fromarray(((((yy / 0.8) ** 2 + (xx / 0.6) ** 2) < 1) * 255).astype(np.uint8)).save('matte.png')
    lm0 = make_landmarks(1, torch.Generator().manual_seed(9))[0].numpy()
    lm0[0, 0], lm0[16, 0] = 190.0, 70.0
    np.savetxt('photo_lm.txt', np.concatenate([lm0, np.zeros((68, 1))], 1))
    np.savetxt('spk.txt', np.abs(np.random.RandomState(3).randn(256)) * 0.1)
    np.savetxt('trg.txt', np.abs(np.random.RandomState(4).randn(256)) * 0.1)
    torch.manual_seed(5)
    torch.save({'model': autovc.Generator(16, 256, 512, 16).state_dict()}, 'm1/autovc.pth')
    base = ['--photo', 'photo.png', '--matte', 'matte.png', '--wav', os.path.join(GOLDEN, 'female12.wav'), '--photo_landmarks',
            'photo_lm.txt', '--load_a2l_G_name', 'm1/g.pth', '--load_a2l_C_name', 'm1/c.pth', '--max_frames', '64', '--batch', '8',
            '--name', 'e2e', '--epoch', '7', '--ngf', '8', '--checkpoints_dir', 'checkpoints', '--speaker_emb', 'spk.txt',
            '--load_AUTOVC_name', 'm1/autovc.pth', '--autovc_target_emb', 'trg.txt']
    frames = {}
    try:
        for out, extra in (('device', ['--module1_post', 'device', '--triangulate', 'device']),
                           ('crossing', ['--module1_post', 'device', '--triangulate', 'host'])):
            np.random.seed(0)                                    # the blinks come from numpy's global generator
            assert end2end.main(base + ['--out', out] + extra) == 0
            assert m1.get_post_backend() == 'device'
            files = sorted(os.listdir(os.path.join(out, 'frames')))
            assert files == ['%05d.png' % k for k in range(64)]
            frames[out] = np.stack([np.asarray(Image.open(os.path.join(out, 'frames', f))) for f in files]).astype(np.float64)
    finally:
        m1.set_post_backend('host')
    assert m1.get_post_backend() == 'host'
    for name in ('device', 'crossing'):
        assert frames[name].shape == (64, 256, 256, 3) and frames[name].std() > 1.0
    # (the two runs triangulate differently, on the device and with scipy: their frames are close, not equal)
    print('end2end, device post-processing: triangulate device vs host: mean |diff| %.3e grey levels' % np.abs(frames['device'] - frames['crossing']).mean())
