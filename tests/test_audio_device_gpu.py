"""GPU (-m gpu): the device audio front end (audio_device.py, csrc/seq/seq_audio.hip) against audio.py and scipy -- the resampler,
the loudness rule bit for bit, apq_filtfilt against scipy.signal.filtfilt, the log-mel, and the whole stage on the example clip at
16 kHz and at 44.1 kHz, down to the f0 track and Module1's landmarks; the fall-backs."""
import os
import sys

import numpy as np
import pytest
import torch
from scipy import signal

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
pytestmark = pytest.mark.gpu

WAV = os.path.join(GOLDEN, 'female12.wav')
K = 1024             # APQ_FF_TILE: the samples apq_filtfilt stages at a time
F32_STEP = 2.0 ** -23


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def clip16(dev):
    """the example clip: its samples, the host's stages (computed once, left unchanged) and the device object"""
    from animateportrait_amd import audio, audio_device, f0
    x, sr = audio.read_wav(WAV)
    n = audio.normalize_loudness(x)
    host = {'x': x, 'sr': sr, 'normalized': n, 'conditioned': audio.conditioned_signal(n), 'mel': audio.mel_spectrogram(n).astype(np.float32),
            'tracker': f0.tracker_input(n)}
    host['windows'] = audio.window_frames(host['mel'])
    for v in host.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return host, audio_device.ClipAudio(WAV, device=dev)


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ------------------------------------------------------------------------------------------------------------ the resampler
@pytest.mark.parametrize('up,down,lengths', [(160, 441, (1, 2, 441, 442, 1000)), (1, 3, (1, 2, 441, 442, 1000, 48001)), (2, 1, (1, 2, 441, 442, 1000)),
                                             (320, 441, (1, 2, 441, 442, 1000))])
def test_resampler_matches_scipy(dev, up, down, lengths):
    from animateportrait_amd import audio_device
    rs = np.random.RandomState(up * 1000 + down)
    worst = 0.0
    for L in lengths:
        for C in (1, 2):
            x = rs.randn(L, C) * 0.3
            want = signal.resample_poly(x, up, down, axis=0)
            got = audio_device.resample_poly(_up(x, dev), up, down).cpu().numpy()
            assert got.shape == want.shape
            err = np.abs(got - want).max() / np.abs(x).max()
            worst = max(worst, err)
            assert err <= 1e-12, (L, C, err)
    print('resample_poly %d/%d: worst error %.3e of the peak (bar 1e-12)' % (up, down, worst))


# -------------------------------------------------------------------------------------------------------------- the loudness
def _loudness_inputs():
    rs = np.random.RandomState(11)
    ties = (np.arange(-2000, 2000) + 0.5) / 32768.0                       # exactly on .5 quantisation ties, both parities
    peaks = rs.randn(4000) * 1e-3
    peaks[::500] = 0.999
    peaks[250::500] = -1.0                                                # the gain drives these over both clamps
    over = np.array([1.0, -1.0, 1.5, -1.5, 32767.4 / 32768, 32767.5 / 32768, -32768.5 / 32768, 0.3, -0.3])   # the quantiser's own clip
    return {'noise -40 dB': rs.randn(30000) * 0.01, 'noise -20 dB': rs.randn(30000) * 0.1, 'noise -6 dB': rs.randn(30000) * 0.5,
            'zeros': np.zeros(1000), 'below half a step': np.full(777, 1e-6), 'peaks': peaks, 'ties': ties, 'over': over,
            'one sample': np.array([0.25]), '100003 samples': rs.randn(100003) * 0.05, 'two channels': rs.randn(20001, 2) * 0.07}


def test_loudness_is_the_hosts_bit_for_bit(dev):
    from animateportrait_amd import audio, audio_device
    for name, x in _loudness_inputs().items():
        want = audio.normalize_loudness(x)
        got = audio_device.normalize_loudness(_up(x, dev)).cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got, want), (name, np.abs(got - want).max())
        q = np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int64)
        assert audio_device.loudness_sumsq(_up(x, dev)) == int((q * q).sum()), name
    peaks = audio.normalize_loudness(_loudness_inputs()['peaks']) * 32768
    assert peaks.max() == 32767 and peaks.min() == -32768                  # the case does reach both clamps


def test_loudness_on_the_resamplers_own_output(dev):
    """44.1 kHz noise: the device rule on the device resampler's output is the host rule on the same numbers bit for bit, and it is
    the host chain's too: the two resamplers agree to 1e-12, which moves a 16-bit sample only where 32768 x lies within 1e-9 of a
    half integer -- no sample of this seed does (asserted)."""
    from animateportrait_amd import audio, audio_device
    x = np.random.RandomState(21).randn(44100, 2) * 0.1
    y_dev = audio_device.resample_poly(_up(x, dev), 160, 441)
    got = audio_device.normalize_loudness(y_dev).cpu().numpy()
    assert np.array_equal(got, audio.normalize_loudness(y_dev.cpu().numpy()))
    y_host = audio.resample_to_16k(x, 44100)
    frac = np.abs(y_host * 32768.0 - np.floor(y_host * 32768.0) - 0.5)
    assert (frac > 1e-9).all()                                             # the exclusion set is empty
    assert np.array_equal(got, audio.normalize_loudness(y_host))


# --------------------------------------------------------------------------------------------------------------- the filter
def _filter_signals(L, rs):
    def impulse(i):
        x = np.zeros(L)
        x[i] = 1.0
        return x
    return {'impulse at 0': impulse(0), 'impulse at L - 1': impulse(L - 1), 'impulse mid-signal': impulse(L // 2), 'constant': np.full(L, 0.7),
            'ramp': np.arange(L) / float(L), 'noise': rs.randn(L) * 0.3}


@pytest.mark.parametrize('name', ['butter(5, 30 / 8000, high)', 'butter(2, 0.2)'])
def test_filtfilt_matches_scipy(dev, name):
    """apq_filtfilt against scipy.signal.filtfilt in float64 within 1e-10 of the signal's peak.  Measured on the MI355X: 0 on every
    case of both filters -- the kernel runs lfilter's recurrence in lfilter's order, so the bits are scipy's.  (The blocked scan
    the kernel was first meant to be misses this bar by six orders and more for the high-pass)"""
    from animateportrait_amd import audio_device
    b, a = signal.butter(5, 30.0 / 8000.0, 'high') if name.startswith('butter(5') else signal.butter(2, 0.2)
    pad = 3 * len(b)
    rs = np.random.RandomState(len(b))
    worst = 0.0
    for L in (pad + 1, K - 1, K, K + 1, 2 * K + 7, 40001, K - 2 * pad, 3 * K - 2 * pad):       # the last two: the extension ends a tile
        for what, x in _filter_signals(L, rs).items():
            want = signal.filtfilt(b, a, x)
            got = audio_device.filtfilt(b, a, _up(x, dev)).cpu().numpy()
            err = np.abs(got - want).max() / np.abs(x).max()
            worst = max(worst, err)
            assert err <= 1e-10, (L, what, err)
    print('filtfilt %s: worst error %.3e of the peak (bar 1e-10)' % (name, worst))


def test_filtfilt_normalises_by_a0_as_lfilter_does(dev):
    from animateportrait_amd import audio_device
    b, a = signal.butter(3, 0.1)
    x = np.random.RandomState(4).randn(3000)
    want = signal.filtfilt(b * 2.5, a * 2.5, x)
    got = audio_device.filtfilt(b * 2.5, a * 2.5, _up(x, dev)).cpu().numpy()
    assert np.abs(got - want).max() <= 1e-10 * np.abs(x).max()


# --------------------------------------------------------------------------------------------------------------- the log-mel
@pytest.mark.parametrize('L', [600, 768, 769, 4097])
def test_logmel_matches_the_host_on_short_signals(dev, L):
    from animateportrait_amd import audio, audio_device
    x = np.random.RandomState(L).randn(L) * 0.1
    want = audio.mel_spectrogram(x).astype(np.float32)
    clip = audio_device.ClipAudio(x, 16000, device=dev, normalize=False)
    assert clip.on_device
    got = clip.mel().cpu().numpy()
    assert clip.conditioned.shape[0] == L + (L % 256 == 0)
    assert np.array_equal(clip.conditioned.cpu().numpy(), audio.conditioned_signal(x))      # the filter and the dither have the host's bits
    err = np.abs(got.astype(np.float64) - want).max()
    print('log-mel L = %d: %s frames, distance %.3e (bar 2.4e-7)' % (L, got.shape, err))
    assert got.shape == want.shape == (clip.conditioned.shape[0] // 256 + 1, 80) and got.dtype == np.float32 and err <= 2.4e-7


def test_logmel_on_the_example_clip(dev, clip16):
    from animateportrait_amd import audio_device
    host, clip = clip16
    got = clip.mel().cpu().numpy()
    err = np.abs(got.astype(np.float64) - host['mel']).max()
    g = np.load(os.path.join(GOLDEN, 'audio.npz'))
    raw = audio_device.ClipAudio(host['x'], host['sr'], device=dev, normalize=False).mel().cpu().numpy()
    gerr = np.abs(raw.astype(np.float64) - g['S']).max()
    print('log-mel female12.wav: distance to the host %.3e (bar 2.4e-7), to the reference-made golden %.3e (bar 2e-6)' % (err, gerr))
    assert got.shape == host['mel'].shape == (818, 80) and err <= 2.4e-7
    assert raw.shape == g['S'].shape and gerr < 2e-6


# ----------------------------------------------------------------------------------------------------------- the whole stage
def test_stage_on_the_example_clip(dev, clip16):
    from animateportrait_amd import audio
    host, clip = clip16
    assert clip.on_device and clip.samples_16k.dtype == torch.float64 and tuple(clip.samples_16k.shape) == (209319, 2)
    assert np.array_equal(clip.normalized.cpu().numpy(), host['normalized'])
    w = audio.clip_audio_features(WAV, backend='device')
    assert w.is_cuda and w.dtype == torch.float32 and tuple(w.shape) == host['windows'].shape == (800, 18, 80)
    err = np.abs(w.cpu().numpy().astype(np.float64) - host['windows']).max()
    print('female12.wav: device windows vs host windows %.3e (bar 2.4e-7)' % err)
    assert err <= 2.4e-7
    assert tuple(audio.clip_audio_features(WAV, max_frames=50, backend='device').shape) == (50, 18, 80)
    half = audio.clip_audio_features(WAV, max_frames=50, backend='device', converter=lambda m: m * 0.5)       # the converter sees a CUDA tensor
    assert np.abs(half.cpu().numpy() - 0.5 * host['windows'][:50]).max() <= 2.4e-7

    t = clip.tracker_input()
    assert t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == host['tracker'].shape
    got = t.cpu().numpy()
    step = np.abs(np.spacing(host['tracker']))
    same = float((got == host['tracker']).mean())
    print('female12.wav: tracker input equal on %.5f of the samples (bar 0.999), worst %.2f fp32 steps (bar 1)'
          % (same, float((np.abs(got - host['tracker']) / step).max())))
    assert (np.abs(got - host['tracker']) <= step).all() and same >= 0.999


def test_f0_track_from_the_clip_object(dev, clip16):
    from animateportrait_amd import f0
    host, clip = clip16
    want = f0.f0_track(host['normalized'], 'F', dev)
    got = f0.f0_track(clip, 'F', dev)
    got_t = f0.f0_track(clip.tracker_input(), 'F', dev)
    assert got.shape == want.shape == (818,) and np.array_equal(got, got_t)
    assert np.array_equal(got < 0, want < 0)                               # the same voiced and unvoiced frames
    v = want >= 0
    err = float(np.abs(got[v] - want[v]).max(initial=0))
    print('female12.wav: f0_norm from ClipAudio vs from host samples %.3e on %d voiced frames (bar 1e-5)' % (err, int(v.sum())))
    assert err <= 1e-5


def test_module1_landmarks_from_device_windows(dev, clip16, golden):
    """seeded Module1 weights, the raw mel windows (as --no_autovc feeds them): device windows against host windows"""
    from animateportrait_amd import audio, module1 as m1
    from test_stream_cpu import _seeded
    host, _ = clip16
    gd = golden('module1.npz')
    netc = _seeded(m1.Audio2LandmarkContent(use_prior_net=True, drop_out=0.5), gd, 'c_', 78).to(dev)
    netg = _seeded(m1.Audio2LandmarkPos(drop_out=0.5), gd, 'g_', 79).to(dev)
    spk = torch.randn(256, generator=torch.Generator().manual_seed(3))
    fid = gd['fid'].view(-1)
    w = audio.clip_audio_features(WAV, max_frames=600, backend='device')
    assert w.is_cuda
    want = m1.predict_landmarks_speaker_aware(netg, netc, host['windows'][:600], spk, fid)
    got = m1.predict_landmarks_speaker_aware(netg, netc, w, spk, fid)
    want, got = (a.cpu().numpy() if torch.is_tensor(a) else a for a in (want, got))
    err = np.abs(got - want).max() / np.abs(want).max()
    print('Module1 landmarks from device windows vs host windows: %.3e of the range (bar 1e-4)' % err)
    assert got.shape == want.shape == (600, 204) and err < 1e-4


def test_stage_on_a_44100_hz_version_of_the_clip(dev, clip16):
    """the clip resampled to 44.1 kHz on the host (4 s of it), then both front ends from there: windows within 1e-5"""
    from animateportrait_amd import audio, audio_device
    host, _ = clip16
    x44 = signal.resample_poly(host['x'][:64000], 441, 160, axis=0)
    x44 = np.clip(np.round(x44 * 32768.0), -32768, 32767) / 32768.0          # as a 16-bit file holds it
    n = audio.normalize_loudness(audio.resample_to_16k(x44, 44100))
    want = audio.window_frames(audio.mel_spectrogram(n).astype(np.float32))
    clip = audio_device.ClipAudio(x44, 44100, device=dev)
    assert clip.on_device and tuple(clip.samples_16k.shape) == (64000, 2)
    rerr = np.abs(clip.samples_16k.cpu().numpy() - audio.resample_to_16k(x44, 44100)).max()
    moved = int((clip.normalized.cpu().numpy() != n).sum())
    got = audio_device.clip_audio_features(clip).cpu().numpy()
    err = np.abs(got.astype(np.float64) - want).max()
    print('44.1 kHz clip: resampler vs scipy %.3e, 16-bit samples that differ %d of %d, windows vs the host path %.3e (bar 1e-5)'
          % (rerr, moved, n.size, err))
    assert got.shape == want.shape and err <= 1e-5


# ------------------------------------------------------------------------------------------------------------ the fall-backs
def test_a_refused_rate_and_a_cpu_device_give_the_host_result_and_the_notice(dev, capsys):
    from animateportrait_amd import audio, audio_device
    x = np.random.RandomState(9).randn(16001) * 0.1
    for sr, device, names in ((16001, dev, 'taps'), (16000, torch.device('cpu'), 'cpu')):
        capsys.readouterr()
        clip = audio_device.ClipAudio(x, sr, device=device)
        out = capsys.readouterr().out
        assert not clip.on_device and out.count('the audio front end runs on the host') == 1 and names in out
        n = audio.normalize_loudness(audio.resample_to_16k(x, sr))
        assert clip.mel().device.type == torch.device(device).type
        assert np.array_equal(clip.mel().cpu().numpy(), audio.mel_spectrogram(n).astype(np.float32))
        assert np.array_equal(clip.conditioned.cpu().numpy(), audio.conditioned_signal(n))
        w = audio_device.clip_audio_features(clip, max_frames=20)
        assert isinstance(w, np.ndarray) and np.array_equal(w, audio.window_frames(audio.mel_spectrogram(n).astype(np.float32))[:20])
    t = torch.zeros(2000, dtype=torch.float64)                              # a CPU tensor is no input of a launch
    for call in (lambda: audio_device.filtfilt([1.0, 0.5], [1.0, -0.5], t), lambda: audio_device.logmel_frames(t),
                 lambda: audio_device.resample_poly(t.view(-1, 1), 1, 3), lambda: audio_device.loudness_sumsq(t)):
        with pytest.raises(TypeError):
            call()


# -------------------------------------------------------------------------------------------------------------- integration
def test_end2end_stage_with_the_device_front_end(dev, golden, tmp_path, monkeypatch, capsys):
    """``end2end.landmarks_from_audio`` with ``--audio_frontend device --f0 device --module1_post device`` and stand-in checkpoints
    (the set-up of tests/test_f0_gpu.py's end2end test): one ``read_wav`` call, Module1 is handed a CUDA tensor of windows, and
    windows and landmarks are those of the host front end to the converter's run-to-run rounding (1e-5 of the range, the bar that
    test uses for the same comparison)."""
    from animateportrait_amd import audio, autovc, end2end, module1 as m1
    from animateportrait_amd.synthetic import make_landmarks
    from test_stream_cpu import _seeded
    gd = golden('module1.npz')
    netc = _seeded(m1.Audio2LandmarkContent(use_prior_net=True, drop_out=0.5), gd, 'c_', 78)
    netg = _seeded(m1.Audio2LandmarkPos(drop_out=0.5), gd, 'g_', 79)
    monkeypatch.chdir(tmp_path)
    os.makedirs('m1')
    torch.save({'G': netg.state_dict()}, 'm1/g.pth')
    torch.save({'model_g_face_id': netc.state_dict()}, 'm1/c.pth')
    lm0 = make_landmarks(1, torch.Generator().manual_seed(9))[0].numpy()
    lm0[0, 0], lm0[16, 0] = 190.0, 70.0
    np.savetxt('photo_lm.txt', np.concatenate([lm0, np.zeros((68, 1))], 1))
    np.savetxt('spk.txt', np.abs(np.random.RandomState(3).randn(256)) * 0.1)
    np.savetxt('trg.txt', np.abs(np.random.RandomState(4).randn(256)) * 0.1)
    torch.manual_seed(5)
    torch.save({'model': autovc.Generator(16, 256, 512, 16).state_dict()}, 'm1/autovc.pth')
    base = ['--photo', 'photo.png', '--out', 'o', '--wav', WAV, '--photo_landmarks', 'photo_lm.txt', '--load_a2l_G_name', 'm1/g.pth',
            '--load_a2l_C_name', 'm1/c.pth', '--max_frames', '48', '--speaker_emb', 'spk.txt', '--load_AUTOVC_name', 'm1/autovc.pth',
            '--autovc_target_emb', 'trg.txt', '--f0', 'device', '--module1_post', 'device']
    seen, reads = [], []
    real, real_read = m1.predict_landmarks_speaker_aware, audio.read_wav

    def spy(net_g, net_c, windows, *args, **kw):
        seen.append(windows)
        return real(net_g, net_c, windows, *args, **kw)

    def counted(path):
        reads.append(path)
        return real_read(path)
    monkeypatch.setattr(m1, 'predict_landmarks_speaker_aware', spy)
    monkeypatch.setattr(audio, 'read_wav', counted)
    before = m1.get_post_backend()
    try:
        np.random.seed(0)
        a = end2end.make_parser().parse_known_args(base + ['--audio_frontend', 'device'])[0]
        _, seq_d = end2end.landmarks_from_audio(a, dev)
        n_device = len(reads)
        np.random.seed(0)
        a = end2end.make_parser().parse_known_args(base)[0]
        assert a.audio_frontend is None
        _, seq_h = end2end.landmarks_from_audio(a, dev)
    finally:
        m1.set_post_backend(before)
    assert n_device == 1 and len(reads) - n_device == 2                    # the host front end reads the file for the mel and for the tracker
    assert 'runs on the host' not in capsys.readouterr().out
    wd, wh = seen
    assert torch.is_tensor(wd) and wd.is_cuda and tuple(wd.shape) == (48, 18, 80) and isinstance(wh, np.ndarray)
    werr = float(np.abs(wd.cpu().numpy() - wh).max())
    assert torch.is_tensor(seq_d) and seq_d.is_cuda and seq_d.shape == seq_h.shape
    serr = float((seq_d - seq_h).abs().max() / seq_h.abs().max())
    print('end2end stage: windows device vs host front end %.3e (bar %.3e), landmarks %.3e of the range (bar 1e-4)'
          % (werr, 1e-5 * np.abs(wh).max(), serr))
    assert werr <= 1e-5 * np.abs(wh).max() and serr < 1e-4
