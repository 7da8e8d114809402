"""CPU (-m "not gpu"): the f0 track -- the float64 restatement (tests/f0_reference.py, the contract of f0.py and
csrc/seq/seq_f0.hip) against signals whose f0 is known, the host-only argument checks of apq_f0_candidates / apq_f0_track, the
signal both the mel spectrogram and the tracker start from, the two defined degenerate normalisations and the options of
end2end.  Nothing here launches a kernel."""
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import f0_reference as R

A = 0x10000          # a stand-in address, aligned to everything the kernels ask for
INTERIOR = slice(3, -3)


@pytest.fixture(scope='module')
def tracks():
    cache = {}

    def get(name, make, gender='F'):
        if name not in cache:
            cache[name] = R.f0_track(make(), gender)
        return cache[name]
    return get


@pytest.mark.parametrize('freq,gender', [(220.0, 'F'), (311.3, 'F'), (440.0, 'F'), (590.0, 'F'), (110.0, 'M')])
def test_restatement_finds_a_steady_tone(tracks, freq, gender):
    """Interior frames all voiced and within 2e-3 relative of the truth (a bare NCCF-plus-parabola prototype gave at most 9.2e-4
    over these five tones: a 2x margin).  Measured with this restatement: 3.2e-4, 2.3e-4, 4.5e-4, 9.2e-4, 3.4e-4."""
    r = tracks('tone%g' % freq, lambda: R.harmonic_signal(freq, 1), gender)
    lf = r['log_f0'][INTERIOR]
    assert r['log_f0'].shape == (16000 // 256 + 1,) and (lf != R.UNVOICED).all()
    err = float(np.abs(np.exp(lf) / freq - 1.0).max())
    print('tone %g Hz %s: worst relative error %.3e (bar 2e-3)' % (freq, gender, err))
    assert err <= 2e-3
    f0n = r['f0_norm']
    assert ((f0n[INTERIOR] >= 0) & (f0n[INTERIOR] <= 1)).all()


def test_restatement_follows_a_glide(tracks):
    """A linear glide 120 -> 300 Hz against the instantaneous frequency at the frame's centre sample.  The correlation pairs a
    window that starts 60 samples before the centre with one a lag later, so the estimate belongs to a slightly later instant:
    this restatement's own worst error is 6.97e-3 relative; the bar is that, doubled: 1.4e-2."""
    freq = np.linspace(120.0, 300.0, 16000)
    r = tracks('glide', lambda: R.harmonic_signal(freq, 2))
    lf = r['log_f0']
    truth = freq[np.minimum(np.arange(lf.shape[0]) * 256, 15999)]
    assert (lf[INTERIOR] != R.UNVOICED).all()
    err = float(np.abs(np.exp(lf[INTERIOR]) / truth[INTERIOR] - 1.0).max())
    print('glide: worst relative error %.3e (bar 1.4e-2)' % err)
    assert err <= 1.4e-2


def test_restatement_finds_the_edges_of_a_gap(tracks):
    """A 200 Hz tone silent for 200 ms (samples 6400 .. 9599: the frames 25 .. 37 are centred in the gap)"""
    r = tracks('gap', lambda: R.harmonic_signal(200.0, 3, gap=(6400, 9600)))
    voiced = r['path'] >= 0
    off = np.nonzero(~voiced)[0]
    print('gap: unvoiced frames %d .. %d (truth 25 .. 37)' % (off[0], off[-1]))
    assert (np.diff(off) == 1).all() and abs(int(off[0]) - 25) <= 2 and abs(int(off[-1]) - 37) <= 2


@pytest.mark.parametrize('which', ['silence', 'noise'])
def test_restatement_leaves_silence_and_noise_unvoiced(tracks, which):
    make = (lambda: np.zeros(16000, np.float32)) if which == 'silence' else (lambda: R.harmonic_signal(0.0, 5, amp=0.0))
    r = tracks(which, make)
    assert (r['path'] == -1).all() and (r['f0_norm'] == R.UNVOICED).all()
    if which == 'silence':
        # (I = 1 exactly; 0.2 / (1 - 0.8) is 1 to an ulp)
        assert (r['count'] == 0).all() and (r['rr'] == 1).all() and np.abs(r['s'] - 1).max() <= 1e-15


def test_degenerate_normalisations_are_defined():
    """No voiced frame: every frame stays -1e10; zero deviation: the voiced frames get 0.5 (the reference divides by zero)"""
    lf = np.full(7, R.UNVOICED)
    assert (R.speaker_normalization(lf) == R.UNVOICED).all()
    lf[3] = np.log(220.0)
    out = R.speaker_normalization(lf)
    assert out[3] == 0.5 and (np.delete(out, 3) == R.UNVOICED).all()
    lf[5] = np.log(220.0)
    out = R.speaker_normalization(lf)
    assert out[3] == 0.5 and out[5] == 0.5
    lf[5] = np.log(440.0)                   # two values: +-1 deviation -> (+-0.25 + 1) / 2
    out = R.speaker_normalization(lf)
    assert np.allclose(out[[3, 5]], [0.375, 0.625], atol=1e-12)


def test_conditioned_signal_is_the_mel_path():
    """mel_spectrogram starts from conditioned_signal: same bits (tests/golden/audio.npz pins mel_spectrogram itself in
    test_audio_cpu.py), first channel, the 1e-6 sample behind a multiple of 256, and the frame count of the tracker."""
    from animateportrait_amd import audio, f0
    rs = np.random.RandomState(0)
    for n in (1024, 1500):
        x = rs.randn(n, 2) * 0.1
        wav = audio.conditioned_signal(x)
        assert wav.dtype == np.float64 and wav.shape == (n + 1 if n % 256 == 0 else n,)
        assert np.array_equal(wav, audio.conditioned_signal(x[:, 0]))
        mel = audio.mel_spectrogram(x)
        d_mel = np.dot(audio.stft_magnitude(wav), audio.mel_filterbank().T)
        by_hand = (20 * np.log10(np.maximum(np.exp(-100 / 20 * np.log(10)), d_mel)) - 16 + 100) / 100
        assert np.array_equal(mel, by_hand)
        assert mel.shape[0] == R.frame_count(wav.shape[0]) == wav.shape[0] // 256 + 1
        t = f0.tracker_input(x)
        assert t.dtype == np.float32 and np.array_equal(t, R.tracker_input(wav))
    x, sr = audio.read_wav(os.path.join(GOLDEN, 'female12.wav'))
    wav = audio.conditioned_signal(audio.normalize_loudness(audio.resample_to_16k(x, sr)))
    assert R.frame_count(wav.shape[0]) == 818
    assert f0.lag_range('F') == R.lag_range('F') == (27, 160) and f0.lag_range('M') == R.lag_range('M') == (64, 320)
    with pytest.raises(ValueError):
        f0.lag_range('X')


def test_header_and_binding_agree_on_the_f0_constants():
    from animateportrait_amd import _seqapi
    hdr = open(os.path.join(ROOT, 'include', 'animateportrait_seq.h')).read()
    for macro, value in (('APQ_F0_HOP', _seqapi.F0_HOP), ('APQ_F0_CANDS', _seqapi.F0_CANDS), ('APQ_F0_STATES', _seqapi.F0_STATES),
                         ('APQ_F0_MIN_LAG', _seqapi.F0_MIN_LAG), ('APQ_F0_MAX_LAG', _seqapi.F0_MAX_LAG),
                         ('APQ_F0_UNVOICED', _seqapi.F0_UNVOICED)):
        assert int(re.search(r'#define\s+%s\s+(\d+)' % macro, hdr).group(1)) == value, macro
    assert _seqapi.F0_CANDS == R.N_CANDS and _seqapi.F0_HOP == R.HOP and _seqapi.F0_MAX_LAG == R.lag_range('M')[1]
    for name in ('apq_f0_candidates', 'apq_f0_candidates_ok', 'apq_f0_track', 'apq_f0_track_ok'):
        assert name in _seqapi.SIGNATURES and hasattr(_seqapi.lib(), name)
    assert _seqapi.lib().apq_abi_version() == 1


def _cand_ok(x=A, L=16000, T=63, kmin=27, kmax=160, count=A, lag=A, val=A, rr=A, s=A):
    from animateportrait_amd import _seqapi
    return _seqapi.lib().apq_f0_candidates_ok(x, L, T, kmin, kmax, count, lag, val, rr, s)


def _track_ok(count=A, lag=A, val=A, rr=A, s=A, T=63, kmax=160, fs=16000.0, back=A + 1, path=A + 3, f0=A):
    from animateportrait_amd import _seqapi
    return _seqapi.lib().apq_f0_track_ok(count, lag, val, rr, s, T, kmax, fs, back, path, f0)


@pytest.mark.parametrize('kw', [dict(), dict(L=1, T=1), dict(L=255, T=1), dict(L=257, T=2), dict(L=300, T=6), dict(kmin=64, kmax=320),
                                dict(kmin=2, kmax=2), dict(T=65536)])
def test_f0_candidates_ok_accepts_the_served_region(kw):
    assert _cand_ok(**kw) == 1


@pytest.mark.parametrize('kw,names', [
    (dict(x=None), 'null x'), (dict(count=None), 'null count'), (dict(lag=None), 'null lag'), (dict(val=None), 'null val'),
    (dict(rr=None), 'null rr'), (dict(s=None), 'null s'), (dict(L=0), 'L = 0'), (dict(T=0), 'T = 0'), (dict(T=65537), 'T = 65537'),
    (dict(kmin=1), 'kmin = 1'), (dict(kmax=321), 'kmax = 321'), (dict(kmin=161), 'kmin = 161 above kmax = 160'),
    (dict(x=A + 2), 'x is not'), (dict(count=A + 2), 'count is not'), (dict(lag=A + 1), 'lag is not'), (dict(val=A + 2), 'val is not'),
    (dict(rr=A + 3), 'rr is not'), (dict(s=A + 2), 's is not'),
])
def test_f0_candidates_ok_refuses_and_names_the_reason(kw, names):
    from animateportrait_amd import _seqapi
    assert _cand_ok() == 1
    assert _cand_ok(**kw) == 0
    assert names in _seqapi.last_error(), _seqapi.last_error()


@pytest.mark.parametrize('kw,names', [
    (dict(count=None), 'null count'), (dict(back=None), 'null back'), (dict(path=None), 'null path'), (dict(f0=None), 'null f0'),
    (dict(T=0), 'T = 0'), (dict(T=65537), 'T = 65537'), (dict(kmax=1), 'kmax = 1'), (dict(kmax=321), 'kmax = 321'),
    (dict(fs=0.0), 'fs is not'), (dict(fs=float('nan')), 'fs is not'), (dict(lag=A + 2), 'lag is not'), (dict(f0=A + 2), 'f0 is not'),
])
def test_f0_track_ok_refuses_and_names_the_reason(kw, names):
    from animateportrait_amd import _seqapi
    assert _track_ok() == 1 and _track_ok(T=1) == 1 and _track_ok(T=65536, kmax=320) == 1
    assert _track_ok(**kw) == 0
    assert names in _seqapi.last_error(), _seqapi.last_error()


def test_f0_calls_refuse_without_launching():
    """The launching calls apply the same checks first and touch no device (there is none here)."""
    from animateportrait_amd import _seqapi
    lib = _seqapi.lib()
    assert lib.apq_f0_candidates(A, 16000, 63, 27, 321, A, A, A, A, A, None) == _seqapi.ERR_UNSUPPORTED
    assert lib.apq_f0_candidates(None, 16000, 63, 27, 160, A, A, A, A, A, None) == _seqapi.ERR_INVALID
    assert lib.apq_f0_track(A, A, A, A, A, 65537, 160, 16000.0, A, A, A, None) == _seqapi.ERR_UNSUPPORTED
    assert lib.apq_f0_track(A, A, A, A, A, 63, 160, 16000.0, A, None, A, None) == _seqapi.ERR_INVALID
    with pytest.raises(RuntimeError, match='null path'):
        _seqapi.check(lib.apq_f0_track(A, A, A, A, A, 63, 160, 16000.0, A, None, A, None), 'f0_track')


BASE = ['--photo', 'p.png', '--out', 'o']
WAV = BASE + ['--wav', 'a.wav', '--photo_landmarks', 'lm.txt', '--speaker_emb', 'spk.txt']


def test_end2end_parser_takes_the_f0_options():
    from animateportrait_amd import end2end
    ap = end2end.make_parser()
    a = ap.parse_args(BASE)
    assert a.f0 is None and a.f0_gender == 'F' and a.f0_npy is None            # the default selects nothing new
    a = ap.parse_args(BASE + ['--f0', 'device', '--f0_gender', 'M'])
    assert a.f0 == 'device' and a.f0_gender == 'M'
    assert ap.parse_args(BASE + ['--f0', 'npy', '--f0_npy', 'f.npy']).f0 == 'npy'
    for bad in (['--f0', 'host'], ['--f0_gender', 'X']):
        with pytest.raises(SystemExit):
            ap.parse_args(BASE + bad)


@pytest.mark.parametrize('args,names', [
    (WAV + ['--f0', 'device', '--f0_npy', 'f.npy'], 'does not go with --f0_npy'),
    (WAV + ['--f0', 'npy'], '--f0 npy needs --f0_npy'),
    (WAV + ['--f0', 'device', '--no_autovc'], '--f0 device'),
    (BASE + ['--landmarks_npy', 'l.npy', '--f0', 'device'], '--f0 device'),
])
def test_end2end_refuses_contradicting_f0_options(args, names, capsys):
    """argparse errors: raised before any file is read or the device is touched"""
    from animateportrait_amd import end2end
    with pytest.raises(SystemExit) as e:
        end2end.main(args)
    assert e.value.code == 2 and names in capsys.readouterr().err
