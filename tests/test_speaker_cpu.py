"""CPU (-m "not gpu"): the speaker embedding's host side -- the window slicing, the volume normalisation and the mono mix of
speaker.py against tests/speaker_reference.py and hand-worked cases, the checkpoint loader, the host-only argument checks of
apq_mel_frames / apq_speaker_head, the header's constants and the options of end2end.  Nothing here launches a kernel."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

import speaker_reference as R

A = 0x10000          # a stand-in address, aligned to everything the kernels ask for


# ------------------------------------------------------------------------------------------------------------------ slicing
@pytest.mark.parametrize('n,starts,pad_to', [
    (25600, [0], 25600),                 # two windows; the second covers (25600 - 8000) / 25600 = 0.6875 and is dropped
    (27200, [0, 50], 33600),             # (27200 - 8000) / 25600 = 0.75 exactly: kept
    (27199, [0], 25600),                 # one sample less: dropped
    (1, [0], 25600),                     # the only window stays whatever it covers
    (40000, [0, 50, 100], 41600),
    (209319, list(range(0, 1151, 50)), 209600),
])
def test_partial_slices_by_hand_and_against_the_reference(n, starts, pad_to):
    from animateportrait_amd import speaker
    got, pad = speaker.partial_slices(n)
    assert got.tolist() == starts and pad == pad_to
    ref, ref_pad = R.partial_slices(n)
    assert [a for a, _ in ref] == starts and all(b - a == 160 for a, b in ref) and ref_pad == pad_to


def test_partial_slices_against_the_reference_over_a_range():
    from animateportrait_amd import speaker
    for n in list(range(1, 60000, 797)) + [8000 * k + d for k in range(3, 9) for d in (-1, 0, 1)] + [960000]:
        got, pad = speaker.partial_slices(n)
        ref, ref_pad = R.partial_slices(n)
        assert got.tolist() == [a for a, _ in ref] and pad == ref_pad, n
    with pytest.raises(ValueError):
        speaker.partial_slices(0)


# ---------------------------------------------------------------------------------------------------------------- the signal
def _dbfs(wav):
    return 20 * np.log10(np.sqrt(np.mean((wav * 32767.0) ** 2)) / 32767.0)


def test_normalize_volume_raises_a_quiet_signal_and_leaves_a_loud_one():
    from animateportrait_amd import speaker
    rs = np.random.RandomState(0)
    quiet = rs.randn(16000) * 1e-3                       # about -60 dBFS
    out = speaker.normalize_volume(quiet)
    assert _dbfs(quiet) < -55 and abs(_dbfs(out) + 30.0) < 1e-9
    assert np.allclose(out, R.normalize_volume(quiet), rtol=1e-15, atol=0)
    loud = rs.randn(16000) * 0.2                         # about -14 dBFS
    assert speaker.normalize_volume(loud) is loud or np.array_equal(speaker.normalize_volume(loud), loud)
    lowered = speaker.normalize_volume(loud, increase_only=False)
    assert abs(_dbfs(lowered) + 30.0) < 1e-9
    silence = np.zeros(100)
    assert np.array_equal(speaker.normalize_volume(silence), silence)


def test_preprocess_wav_averages_the_channels_of_the_stereo_fixture():
    from animateportrait_amd import audio, speaker
    x, sr = audio.read_wav(os.path.join(GOLDEN, 'female12.wav'))
    assert x.ndim == 2 and x.shape[1] == 2 and sr == 16000 and not np.array_equal(x[:, 0], x[:, 1])
    wav = speaker.preprocess_wav(x, sr)
    assert wav.dtype == np.float32 and wav.shape == (x.shape[0],)
    want = speaker.normalize_volume(x.mean(axis=1)).astype(np.float32)
    assert np.array_equal(wav, want) and np.array_equal(wav, R.preprocess_wav(x, sr))
    first = speaker.normalize_volume(x[:, 0]).astype(np.float32)
    assert not np.array_equal(wav, first)                # not the mel path's first channel
    # another rate goes through the polyphase resampler; a mask is applied last
    half = speaker.preprocess_wav(x[:32000], 32000)
    assert half.shape == (16000,) and np.array_equal(half, R.preprocess_wav(x[:32000], 32000))
    keep = np.arange(x.shape[0]) % 3 != 0
    assert np.array_equal(speaker.preprocess_wav(x, sr, keep=keep), wav[keep])
    with pytest.raises(ValueError):
        speaker.preprocess_wav(x, sr, keep=keep[:-1])


def test_reference_filterbank_and_window_are_the_modules():
    from animateportrait_amd import audio
    assert np.array_equal(R.slaney_filterbank(16000, 400, 40, 0.0, 8000.0), audio.mel_filterbank(16000, 400, 40, 0.0, 8000.0))
    assert np.array_equal(R.slaney_filterbank(16000, 1024, 80, 90.0, 7600.0), audio.mel_filterbank())
    from scipy import signal
    assert np.allclose(R.hann_periodic(400), signal.get_window('hann', 400, fftbins=True), rtol=0, atol=1e-15)


def test_reference_mel_is_the_stft_of_audio_py():
    """the reference's framing against audio.stft_magnitude (pinned to the reference project's own function) at 1024 / 256"""
    from animateportrait_amd import audio
    x = np.random.RandomState(1).randn(4099) * 0.1
    basis = audio.mel_filterbank()
    want = np.dot(audio.stft_magnitude(x), basis.T.astype(np.float64))
    got = R.mel_frames(x, R.hann_periodic(1024), basis, 256, 1)
    assert got.shape == want.shape == (4099 // 256 + 1, 80)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


# ---------------------------------------------------------------------------------------------------------------- checkpoint
def _state(seed=3):
    sd = {k: torch.from_numpy(v) for k, v in R.seeded_weights(seed).items()}
    sd['similarity_weight'] = torch.tensor([10.0])
    sd['similarity_bias'] = torch.tensor([-5.0])
    return sd


def test_load_encoder_reads_the_published_layout(tmp_path, monkeypatch):
    from animateportrait_amd import speaker
    monkeypatch.setattr(speaker, '_device', lambda device: torch.device('cpu'))       # no GPU here: the loader's own work only
    sd = _state()
    path = str(tmp_path / 'pretrained.pt')
    torch.save({'step': 1, 'model_state': sd}, path)
    enc = speaker.load_encoder(path)
    assert not enc.training and enc.lstm_backend == 'library'
    got = enc.state_dict()
    assert sorted(got) == sorted(k for k in sd if not k.startswith('similarity'))
    assert all(torch.equal(got[k], sd[k]) for k in got)
    assert enc.lstm.input_size == 40 and enc.lstm.hidden_size == 256 and enc.lstm.num_layers == 3 and enc.lstm.batch_first
    assert speaker.load_encoder(path, lstm_backend='hip').lstm_backend == 'hip'
    missing = {k: v for k, v in sd.items() if k != 'lstm.weight_hh_l2'}
    torch.save({'model_state': missing}, path)
    with pytest.raises(RuntimeError, match='lstm.weight_hh_l2'):
        speaker.load_encoder(path)
    torch.save({'model_state': dict(sd, extra=torch.zeros(1))}, path)
    with pytest.raises(RuntimeError, match='extra'):
        speaker.load_encoder(path)
    torch.save(sd, path)
    with pytest.raises(RuntimeError, match='model_state'):
        speaker.load_encoder(path)
    with pytest.raises(ValueError):
        speaker.VoiceEncoder('cudnn')


def test_the_embedding_has_no_host_path():
    from animateportrait_amd import speaker
    enc = speaker.VoiceEncoder()
    with pytest.raises(ValueError, match='GPU'):
        enc.embed_utterance(np.zeros(16000, np.float32))
    with pytest.raises(TypeError):
        speaker.mel_frames(torch.zeros(1000), torch.zeros(400, dtype=torch.float64), torch.zeros(40, 201), 160, 2)
    with pytest.raises(TypeError):
        speaker.head(torch.zeros(2, 256), torch.zeros(256, 256), torch.zeros(256))


# --------------------------------------------------------------------------------------------------------- the host-only checks
def _mel_ok(x=A, window=A, basis=A, out=A, L=25600, n_fft=400, hop=160, n_mels=40, power=2):
    from animateportrait_amd import _seqapi
    return _seqapi.lib().apq_mel_frames_ok(x, window, basis, out, L, n_fft, hop, n_mels, power)


def _head_ok(h=A, w=A, b=A, partial=A, embed=A, B=24):
    from animateportrait_amd import _seqapi
    return _seqapi.lib().apq_speaker_head_ok(h, w, b, partial, embed, B)


@pytest.mark.parametrize('kw', [dict(), dict(L=201), dict(n_fft=1024, hop=256, n_mels=80, power=1, L=513), dict(n_fft=16, hop=16, n_mels=1, L=9),
                                dict(n_fft=18, hop=1, L=10), dict(n_mels=128), dict(hop=400), dict(L=160 * 65535 + 159), dict(window=A + 8),
                                dict(x=A + 4, basis=A + 4, out=A + 4)])
def test_mel_frames_ok_accepts_the_served_region(kw):
    from animateportrait_amd import _seqapi
    assert _mel_ok(**kw) == 1, _seqapi.last_error()


MEL_REFUSED = [
    (dict(x=None), -1, 'null x'), (dict(window=None), -1, 'null window'), (dict(basis=None), -1, 'null basis'), (dict(out=None), -1, 'null out'),
    (dict(L=0), -1, 'L = 0'), (dict(hop=0), -1, 'hop = 0'), (dict(n_mels=0), -1, 'n_mels = 0'), (dict(n_fft=0), -1, 'n_fft = 0'),
    (dict(power=3), -1, 'power = 3'), (dict(power=0), -1, 'power = 0'),
    (dict(n_fft=401), -2, 'n_fft = 401 is odd'), (dict(n_fft=1026, L=4000), -2, 'n_fft = 1026'), (dict(n_fft=14), -2, 'n_fft = 14'),
    (dict(L=200), -2, 'L = 200'), (dict(n_mels=129), -2, 'n_mels = 129'), (dict(hop=401), -2, 'hop = 401 above n_fft = 400'),
    (dict(L=160 * 65536), -2, 'T = 65537'),
    (dict(x=A + 2), -2, 'x is not'), (dict(window=A + 4), -2, 'window is not 8-byte'), (dict(basis=A + 1), -2, 'basis is not'),
    (dict(out=A + 2), -2, 'out is not'),
]

HEAD_REFUSED = [
    (dict(h=None), -1, 'null h'), (dict(w=None), -1, 'null w'), (dict(b=None), -1, 'null b'), (dict(partial=None), -1, 'null partial'),
    (dict(embed=None), -1, 'null embed'), (dict(B=0), -1, 'B = 0'), (dict(B=4097), -2, 'B = 4097'),
    (dict(h=A + 2), -2, 'h is not'), (dict(w=A + 1), -2, 'w is not'), (dict(b=A + 3), -2, 'b is not'), (dict(partial=A + 2), -2, 'partial is not'),
    (dict(embed=A + 2), -2, 'embed is not'),
]


@pytest.mark.parametrize('kw,code,names', MEL_REFUSED)
def test_mel_frames_refuses_and_names_the_reason(kw, code, names):
    """the _ok twin says no with the reason; the launching call returns the code without touching a device (there is none)"""
    from animateportrait_amd import _seqapi
    assert _mel_ok() == 1
    assert _mel_ok(**kw) == 0
    assert names in _seqapi.last_error(), _seqapi.last_error()
    args = dict(dict(x=A, window=A, basis=A, out=A, L=25600, n_fft=400, hop=160, n_mels=40, power=2), **kw)
    assert code == {-1: _seqapi.ERR_INVALID, -2: _seqapi.ERR_UNSUPPORTED}[code]
    assert _seqapi.lib().apq_mel_frames(*args.values(), None) == code
    assert names in _seqapi.last_error(), _seqapi.last_error()


@pytest.mark.parametrize('kw,code,names', HEAD_REFUSED)
def test_speaker_head_refuses_and_names_the_reason(kw, code, names):
    from animateportrait_amd import _seqapi
    assert _head_ok() == 1 and _head_ok(B=1) == 1 and _head_ok(B=4096) == 1
    assert _head_ok(**kw) == 0
    assert names in _seqapi.last_error(), _seqapi.last_error()
    args = dict(dict(h=A, w=A, b=A, partial=A, embed=A, B=24), **kw)
    assert _seqapi.lib().apq_speaker_head(*args.values(), None) == code
    assert names in _seqapi.last_error(), _seqapi.last_error()
    with pytest.raises(RuntimeError, match='libapseq speaker_head'):
        _seqapi.check(code, 'speaker_head')


def test_header_and_binding_agree_on_the_speaker_constants():
    from animateportrait_amd import _seqapi, speaker
    hdr = open(os.path.join(ROOT, 'include', 'animateportrait_seq.h')).read()
    for macro, value in (('APQ_MEL_MIN_FFT', _seqapi.MEL_MIN_FFT), ('APQ_MEL_MAX_FFT', _seqapi.MEL_MAX_FFT),
                         ('APQ_MEL_MAX_MELS', _seqapi.MEL_MAX_MELS), ('APQ_ALIGN_F64', _seqapi.ALIGN_F64), ('APQ_SPK_E', _seqapi.SPK_E),
                         ('APQ_SPK_MAX_B', _seqapi.SPK_MAX_B)):
        assert int(re.search(r'#define\s+%s\s+(\d+)' % macro, hdr).group(1)) == value, macro
    assert _seqapi.SPK_E == _seqapi.LSTM_H == R.E == speaker.EMBED
    assert (speaker.MEL_N_FFT, speaker.MEL_HOP, speaker.MEL_BANDS, speaker.PARTIAL_FRAMES) == (R.N_FFT, R.HOP, R.N_MELS, R.PARTIAL)
    for name in ('apq_mel_frames', 'apq_mel_frames_ok', 'apq_speaker_head', 'apq_speaker_head_ok'):
        assert name in _seqapi.SIGNATURES and hasattr(_seqapi.lib(), name)
    assert _seqapi.lib().apq_abi_version() == 1


# --------------------------------------------------------------------------------------------------------------------- end2end
BASE = ['--photo', 'p.png', '--out', 'o']
WAV = BASE + ['--wav', 'a.wav', '--photo_landmarks', 'lm.txt']


def test_end2end_parser_takes_the_speaker_options():
    from animateportrait_amd import end2end
    ap = end2end.make_parser()
    a = ap.parse_args(BASE)
    assert a.speaker_emb_from is None and a.speaker_encoder is None             # the default selects nothing new
    a = ap.parse_args(WAV + ['--speaker_emb_from', 'wav', '--speaker_encoder', 'enc.pt'])
    assert a.speaker_emb_from == 'wav' and a.speaker_encoder == 'enc.pt'
    assert ap.parse_args(WAV + ['--speaker_emb_from', 'txt', '--speaker_emb', 's.txt']).speaker_emb_from == 'txt'
    with pytest.raises(SystemExit):
        ap.parse_args(BASE + ['--speaker_emb_from', 'resemblyzer'])


@pytest.mark.parametrize('args,names', [
    (WAV + ['--speaker_emb_from', 'wav', '--speaker_encoder', 'e.pt', '--speaker_emb', 's.txt'], 'does not go with --speaker_emb'),
    (BASE + ['--landmarks_npy', 'l.npy', '--speaker_emb_from', 'wav', '--speaker_encoder', 'e.pt'], '--speaker_emb_from wav needs --wav'),
    (WAV + ['--speaker_emb_from', 'wav'], '--speaker_emb_from wav needs --speaker_encoder'),
    (WAV + ['--speaker_emb', 's.txt', '--speaker_encoder', 'e.pt'], '--speaker_encoder goes with --speaker_emb_from wav'),
    (WAV, '--wav needs --speaker_emb'),                                          # as before
    (WAV + ['--speaker_emb_from', 'txt'], '--wav needs --speaker_emb'),
])
def test_end2end_refuses_contradicting_speaker_options(args, names, capsys):
    """argparse errors: raised before any file is read or the device is touched"""
    from animateportrait_amd import end2end
    with pytest.raises(SystemExit) as e:
        end2end.main(args)
    assert e.value.code == 2 and names in capsys.readouterr().err
