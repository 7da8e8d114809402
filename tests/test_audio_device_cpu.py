"""CPU (-m "not gpu"): the device audio front end's host side -- the new symbols of libapseq.so and their host-only argument
checks, the resampler's cached taps under a numpy restatement of the kernel's index arithmetic against scipy, the dither table,
the unchanged default of audio.clip_audio_features, the fall-back of a CPU-only call and the option of end2end.  Nothing here
launches a kernel."""
import os
import re

import numpy as np
import pytest
import torch
from scipy import signal

from conftest import GOLDEN, ROOT

A = 0x10000          # a stand-in address, aligned to everything the kernels ask for
WAV = os.path.join(GOLDEN, 'female12.wav')

NEW = ('apq_resample_poly', 'apq_loudness_sumsq', 'apq_loudness_apply', 'apq_filtfilt', 'apq_logmel_frames')


def _lib():
    from animateportrait_amd import _seqapi
    return _seqapi.lib()


def test_new_symbols_and_twins_exist_and_the_abi_stays():
    from animateportrait_amd import _seqapi
    for name in NEW:
        for n in (name, name + '_ok'):
            assert n in _seqapi.SIGNATURES and hasattr(_lib(), n), n
    for n in ('apq_loudness_workspace_bytes', 'apq_filtfilt_workspace_bytes'):
        assert n in _seqapi.SIGNATURES and hasattr(_lib(), n), n
    assert _lib().apq_abi_version() == 1 == _seqapi.ABI_VERSION
    hdr = open(os.path.join(ROOT, 'include', 'animateportrait_seq.h')).read()
    for macro, value in (('APQ_RS_MAX_RATE', _seqapi.RS_MAX_RATE), ('APQ_RS_MAX_TAPS', _seqapi.RS_MAX_TAPS), ('APQ_RS_MAX_C', _seqapi.RS_MAX_C),
                         ('APQ_RS_MAX_L', _seqapi.RS_MAX_L), ('APQ_LOUD_MAX_N', _seqapi.LOUD_MAX_N), ('APQ_LOUD_MAX_BLOCKS', _seqapi.LOUD_MAX_BLOCKS),
                         ('APQ_FF_MAX_M', _seqapi.FF_MAX_M), ('APQ_FF_MAX_L', _seqapi.FF_MAX_L), ('APQ_FF_TILE', _seqapi.FF_TILE)):
        assert int(re.search(r'#define\s+%s\s+(\w+)' % macro, hdr).group(1), 0) == value, macro
    assert _seqapi.LOUD_MAX_N * 2 ** 30 < 2 ** 53 <= (_seqapi.LOUD_MAX_N + 1) * 2 ** 30         # where numpy's mean stays exact
    assert _lib().apq_loudness_workspace_bytes(1) == 8 and _lib().apq_loudness_workspace_bytes(8388607) == 8 * 256
    assert _lib().apq_filtfilt_workspace_bytes(1000, 5) == 8 * (1000 + 36)


# ---------------------------------------------------------------------------------------------------- the host-only checks
CALLS = {
    'apq_resample_poly': dict(x=A, h=A, y=A + 0x100000, L=44100, C=2, N=8821, up=160, down=441),
    'apq_loudness_sumsq': dict(x=A, workspace=A + 8, sum=A, N=160000),
    'apq_loudness_apply': dict(x=A, y=A, N=160000, gain=1.5, apply_gain=1),
    'apq_filtfilt': dict(x=A, y=A + 0x100000, b=A, a=A, zi=A, workspace=A, L=160000, M=5),
    'apq_logmel_frames': dict(x=A, window=A, basis=A, out=A, L=160000, n_fft=1024, hop=256, n_mels=80),
}

ACCEPTED = [
    ('apq_resample_poly', dict()), ('apq_resample_poly', dict(L=1, C=1)), ('apq_resample_poly', dict(up=1, down=3, N=61)),
    ('apq_resample_poly', dict(up=2, down=1, N=41)), ('apq_resample_poly', dict(up=640, down=441, N=12801)),
    ('apq_resample_poly', dict(up=320, down=441, N=8821)), ('apq_resample_poly', dict(up=2, down=3, N=61)), ('apq_resample_poly', dict(up=1, down=2, N=41)),
    ('apq_resample_poly', dict(up=1024, down=1024, N=16383)), ('apq_resample_poly', dict(x=A + 8, h=A + 8, y=A + 24)),
    ('apq_loudness_sumsq', dict()), ('apq_loudness_sumsq', dict(N=1)), ('apq_loudness_sumsq', dict(N=8388607)),
    ('apq_loudness_apply', dict()), ('apq_loudness_apply', dict(N=1, apply_gain=0, gain=0.0)), ('apq_loudness_apply', dict(N=8388607, y=A + 8)),
    ('apq_filtfilt', dict()), ('apq_filtfilt', dict(L=19)), ('apq_filtfilt', dict(M=1, L=7)), ('apq_filtfilt', dict(M=8, L=28)),
    ('apq_filtfilt', dict(M=2, L=10)),
    ('apq_logmel_frames', dict()), ('apq_logmel_frames', dict(L=513)), ('apq_logmel_frames', dict(n_fft=400, hop=160, n_mels=40, L=201)),
    ('apq_logmel_frames', dict(x=A + 8, window=A + 8, basis=A + 4, out=A + 4)), ('apq_logmel_frames', dict(n_mels=128)),
]

REFUSED = [
    ('apq_resample_poly', dict(x=None), -1, 'null x'), ('apq_resample_poly', dict(h=None), -1, 'null h'), ('apq_resample_poly', dict(y=None), -1, 'null y'),
    ('apq_resample_poly', dict(L=0), -1, 'L = 0'), ('apq_resample_poly', dict(C=0), -1, 'C = 0'), ('apq_resample_poly', dict(N=0), -1, 'N = 0'),
    ('apq_resample_poly', dict(up=0), -1, 'up = 0'), ('apq_resample_poly', dict(down=0), -1, 'down = 0'),
    ('apq_resample_poly', dict(C=3), -2, 'C = 3'), ('apq_resample_poly', dict(up=1025), -2, 'up = 1025'), ('apq_resample_poly', dict(down=1025), -2, 'down = 1025'),
    ('apq_resample_poly', dict(N=8820), -2, 'N = 8820 taps is even'), ('apq_resample_poly', dict(N=16385), -2, 'N = 16385 taps'),
    ('apq_resample_poly', dict(up=1000, down=1, L=0x3fffffff), -2, 'elements'), ('apq_resample_poly', dict(L=0x40000000), -2, 'L = 1073741824'),
    ('apq_resample_poly', dict(x=A + 4), -2, 'x is not 8-byte'), ('apq_resample_poly', dict(h=A + 4), -2, 'h is not 8-byte'),
    ('apq_resample_poly', dict(y=A + 2), -2, 'y is not 8-byte'),
    ('apq_loudness_sumsq', dict(x=None), -1, 'null x'), ('apq_loudness_sumsq', dict(workspace=None), -1, 'null workspace'),
    ('apq_loudness_sumsq', dict(sum=None), -1, 'null sum'), ('apq_loudness_sumsq', dict(N=0), -1, 'N = 0'),
    ('apq_loudness_sumsq', dict(N=8388608), -2, 'N = 8388608'), ('apq_loudness_sumsq', dict(x=A + 4), -2, 'x is not'),
    ('apq_loudness_sumsq', dict(workspace=A + 4), -2, 'workspace is not'), ('apq_loudness_sumsq', dict(sum=A + 4), -2, 'sum is not'),
    ('apq_loudness_apply', dict(x=None), -1, 'null x'), ('apq_loudness_apply', dict(y=None), -1, 'null y'), ('apq_loudness_apply', dict(N=0), -1, 'N = 0'),
    ('apq_loudness_apply', dict(N=8388608), -2, 'N = 8388608'), ('apq_loudness_apply', dict(apply_gain=2), -1, 'apply_gain = 2'),
    ('apq_loudness_apply', dict(gain=0.0), -1, 'gain'), ('apq_loudness_apply', dict(gain=float('nan')), -1, 'gain'),
    ('apq_loudness_apply', dict(gain=float('inf')), -1, 'gain'), ('apq_loudness_apply', dict(x=A + 4), -2, 'x is not'),
    ('apq_loudness_apply', dict(y=A + 4), -2, 'y is not'),
    ('apq_filtfilt', dict(x=None), -1, 'null x'), ('apq_filtfilt', dict(y=None), -1, 'null y'), ('apq_filtfilt', dict(b=None), -1, 'null b'),
    ('apq_filtfilt', dict(a=None), -1, 'null a'), ('apq_filtfilt', dict(zi=None), -1, 'null zi'), ('apq_filtfilt', dict(workspace=None), -1, 'null workspace'),
    ('apq_filtfilt', dict(L=0), -1, 'L = 0'), ('apq_filtfilt', dict(L=18), -2, 'L = 18'), ('apq_filtfilt', dict(M=2, L=9), -2, 'L = 9'),
    ('apq_filtfilt', dict(M=0), -2, 'M = 0'), ('apq_filtfilt', dict(M=9), -2, 'M = 9'), ('apq_filtfilt', dict(L=0x3fffffc1), -2, 'L = 1073741761'),
    ('apq_filtfilt', dict(y=A), -2, 'y is x'), ('apq_filtfilt', dict(x=A + 4), -2, 'x is not'), ('apq_filtfilt', dict(y=A + 4), -2, 'y is not'),
    ('apq_filtfilt', dict(workspace=A + 4), -2, 'workspace is not'),
    ('apq_logmel_frames', dict(x=None), -1, 'null x'), ('apq_logmel_frames', dict(window=None), -1, 'null window'),
    ('apq_logmel_frames', dict(basis=None), -1, 'null basis'), ('apq_logmel_frames', dict(out=None), -1, 'null out'),
    ('apq_logmel_frames', dict(L=0), -1, 'L = 0'), ('apq_logmel_frames', dict(hop=0), -1, 'hop = 0'), ('apq_logmel_frames', dict(n_mels=0), -1, 'n_mels = 0'),
    ('apq_logmel_frames', dict(n_fft=0), -1, 'n_fft = 0'), ('apq_logmel_frames', dict(n_fft=401), -2, 'n_fft = 401 is odd'),
    ('apq_logmel_frames', dict(n_fft=1026), -2, 'n_fft = 1026'), ('apq_logmel_frames', dict(n_fft=14), -2, 'n_fft = 14'),
    ('apq_logmel_frames', dict(L=512), -2, 'L = 512'), ('apq_logmel_frames', dict(n_mels=129), -2, 'n_mels = 129'),
    ('apq_logmel_frames', dict(hop=1025), -2, 'hop = 1025 above n_fft = 1024'), ('apq_logmel_frames', dict(L=256 * 65536), -2, 'T = 65537'),
    ('apq_logmel_frames', dict(x=A + 4), -2, 'x is not 8-byte'), ('apq_logmel_frames', dict(window=A + 4), -2, 'window is not 8-byte'),
    ('apq_logmel_frames', dict(basis=A + 1), -2, 'basis is not'), ('apq_logmel_frames', dict(out=A + 2), -2, 'out is not'),
]


@pytest.mark.parametrize('name,kw', ACCEPTED)
def test_twins_accept_the_served_region(name, kw):
    from animateportrait_amd import _seqapi
    args = dict(CALLS[name], **kw)
    assert getattr(_lib(), name + '_ok')(*args.values()) == 1, _seqapi.last_error()


@pytest.mark.parametrize('name,kw,code,names', REFUSED)
def test_twins_refuse_and_name_the_reason(name, kw, code, names):
    """the _ok twin says no with the reason; the launching call returns the code with a null stream without touching a device"""
    from animateportrait_amd import _seqapi
    assert code == {-1: _seqapi.ERR_INVALID, -2: _seqapi.ERR_UNSUPPORTED}[code]
    args = dict(CALLS[name], **kw)
    assert getattr(_lib(), name + '_ok')(*CALLS[name].values()) == 1
    assert getattr(_lib(), name + '_ok')(*args.values()) == 0
    assert names in _seqapi.last_error(), _seqapi.last_error()
    assert getattr(_lib(), name)(*args.values(), None) == code
    assert names in _seqapi.last_error(), _seqapi.last_error()


# ------------------------------------------------------------------------------------------------------------ the resampler
def resample_restated(x, h, up, down):
    """seq_audio.hip's resample_poly_kernel in numpy: per output its phase's taps only, ascending, signal zero outside [0, L)"""
    x = np.asarray(x, np.float64)
    flat = x.ndim == 1
    x = x.reshape(x.shape[0], -1)
    L, N = x.shape[0], h.shape[0]
    half = (N - 1) // 2
    pre_pad = down - half % down
    pre_remove = (half + pre_pad) // down
    n_out = -(-L * up // down)
    y = np.zeros((n_out, x.shape[1]))
    for o in range(n_out):
        m = (o + pre_remove) * down - pre_pad
        xi, j0 = m // up, m % up
        for j in range(j0, N, up):
            if xi < 0:
                break
            if xi < L:
                y[o] += h[j] * x[xi]
            xi -= 1
    return y[:, 0] if flat else y


@pytest.mark.parametrize('up,down', [(160, 441), (1, 3), (2, 1), (320, 441)])
def test_cached_taps_and_the_kernels_index_arithmetic_reproduce_scipy(up, down):
    from animateportrait_amd import audio_device
    h = audio_device.resample_taps(up, down)
    assert h is audio_device.resample_taps(up, down) and h.dtype == np.float64 and h.shape == (20 * max(up, down) + 1,)
    rs = np.random.RandomState(up * 1000 + down)
    for L in (1, 2, 441, 442, 1000):
        for C in (1, 2):
            x = rs.randn(L, C) * 0.3
            want = signal.resample_poly(x, up, down, axis=0)
            got = resample_restated(x, h, up, down)
            assert got.shape == want.shape == (-(-L * up // down), C)
            assert np.abs(got - want).max() <= 1e-12 * np.abs(x).max(), (L, C)


def test_rate_ratio_is_resample_to_16k_s():
    from animateportrait_amd import audio_device
    assert [audio_device.rate_ratio(sr) for sr in (8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000)] == \
        [(2, 1), (640, 441), (1, 1), (320, 441), (2, 3), (1, 2), (160, 441), (1, 3)]
    for sr in (8000, 11025, 22050, 24000, 32000, 44100, 48000):
        for C in (1, 2):
            assert audio_device.refusal(sr, sr, C, True, 'cuda') is None
    assert 'taps' in audio_device.refusal(16001, 16001, 1, True, 'cuda')
    assert 'channels' in audio_device.refusal(16000, 16000, 3, True, 'cuda')
    assert 'loudness' in audio_device.refusal(16000, 8388608, 1, True, 'cuda') and audio_device.refusal(16000, 8388608, 1, False, 'cuda') is None
    assert 'cpu' in audio_device.refusal(16000, 16000, 1, True, 'cpu')


# ---------------------------------------------------------------------------------------------------------------- the dither
def test_dither_table_is_a_prefix_of_the_fixed_sequence():
    from animateportrait_amd import audio_device
    for n in (1, 624, 625, 100001, 7):
        assert np.array_equal(audio_device.dither_host(n), np.random.RandomState(0).rand(n)), n
        assert np.array_equal(audio_device.dither_table(n, torch.device('cpu')).numpy(), np.random.RandomState(0).rand(n)), n


def test_highpass_is_conditioned_signal_s():
    from animateportrait_amd import audio_device
    b, a, zi = audio_device.highpass()
    wb, wa = signal.butter(5, 30.0 / 8000.0, btype='high')
    assert np.array_equal(b, wb) and np.array_equal(a, wa) and np.array_equal(zi, signal.lfilter_zi(wb, wa))


def test_loudness_gain_is_normalize_loudness_s():
    from animateportrait_amd import audio
    x = np.random.RandomState(5).randn(5000, 2) * 0.05
    q = np.clip(np.round(x * 32768.0), -32768, 32767)
    rms = int(np.sqrt(np.mean(q ** 2)))
    gain = 10.0 ** ((-20.0 - 20.0 * np.log10(rms / 32768.0)) / 20.0)
    assert audio.loudness_gain(rms) == gain
    v = q * gain
    v = np.where(v > 32767.0, 32767.0, np.where(v < -32767.0, -32768.0, v))
    assert np.array_equal(audio.normalize_loudness(x), np.floor(v) / 32768.0)


# ------------------------------------------------------------------------------------------------------------ the interface
def test_default_backend_is_the_host_and_keeps_its_bits():
    from animateportrait_amd import audio
    a = audio.clip_audio_features(WAV, max_frames=40)
    b = audio.clip_audio_features(WAV, max_frames=40, backend='host')
    assert isinstance(a, np.ndarray) and a.dtype == np.float32 and a.shape == (40, 18, 80) and np.array_equal(a, b)
    with pytest.raises(ValueError, match='backend'):
        audio.clip_audio_features(WAV, backend='gpu')


def test_window_frames_device_is_window_frames():
    from animateportrait_amd import audio, audio_device
    mel = np.random.RandomState(2).rand(40, 80).astype(np.float32)
    for T in (40, 19, 18, 5):
        got = audio_device.window_frames_device(torch.from_numpy(mel[:T]))
        want = audio.window_frames(mel[:T])
        assert tuple(got.shape) == want.shape and np.array_equal(got.numpy(), want)


def test_device_backend_without_a_gpu_falls_back_with_the_notice(capsys, monkeypatch):
    from animateportrait_amd import audio, audio_device
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    want = audio.clip_audio_features(WAV, max_frames=30, converter=lambda m: m * 0.5)
    got = audio.clip_audio_features(WAV, max_frames=30, converter=lambda m: m * 0.5, backend='device')
    out = capsys.readouterr().out
    assert out.count('the audio front end runs on the host') == 1 and 'cpu' in out
    assert isinstance(got, np.ndarray) and np.array_equal(got, want)
    clip = audio_device.ClipAudio(WAV, device='cpu')
    assert not clip.on_device and capsys.readouterr().out.count('runs on the host') == 1
    x, sr = audio.read_wav(WAV)
    n = audio.normalize_loudness(x)
    assert np.array_equal(clip.samples_16k.numpy(), x) and np.array_equal(clip.normalized.numpy(), n)
    assert np.array_equal(clip.conditioned.numpy(), audio.conditioned_signal(n))
    assert np.array_equal(clip.mel().numpy(), audio.mel_spectrogram(n).astype(np.float32))
    from animateportrait_amd import f0
    assert np.array_equal(clip.tracker_input().numpy(), f0.tracker_input(n))


def test_end2end_parser_knows_the_option():
    from animateportrait_amd import end2end
    ap = end2end.make_parser()
    base = ['--photo', 'p.png', '--out', 'o']
    assert ap.parse_args(base).audio_frontend is None                                  # the default selects nothing new
    assert ap.parse_args(base + ['--audio_frontend', 'device']).audio_frontend == 'device'
    assert ap.parse_args(base + ['--audio_frontend', 'host']).audio_frontend == 'host'
    with pytest.raises(SystemExit):
        ap.parse_args(base + ['--audio_frontend', 'gpu'])
