"""The clip's speaker embedding restated in float64 numpy (own code, written from resemblyzer as published: ``preprocess_wav``
without its silence trim, ``wav_to_mel_spectrogram``, ``compute_partial_slices``, ``VoiceEncoder.forward`` /
``embed_utterance``, and the reference's ``get_spk_emb``): the contract of animateportrait_amd/speaker.py and
csrc/seq/seq_speaker.hip, and the reference of their tests.

  * mel: frames of the reflect-padded signal (numpy's 'reflect', n_fft / 2 a side) centred on the samples t hop, times the window,
    ``np.fft.rfft``, ``|X| ** power``, times the filter bank; T = L // hop + 1 frames.  No log.
  * the LSTM is written out with PyTorch's gate order i, f, g, o and zero initial state.
  * head: relu(w h + b) / its L2 norm per window; the mean over the windows / its L2 norm.  A window whose ReLU output is all zero
    stays zero and counts in the mean; when all are zero the embedding is zero (resemblyzer divides 0 by 0 in both places).
  * weights are seeded, uniform in +-1/16 (PyTorch's default for 256 hidden units).

resemblyzer, librosa and webrtcvad are absent from the build image, and so is the published checkpoint: parity of this file with
resemblyzer / librosa themselves and with ``pretrained.pt`` is unpinned.  The silence trim is not restated at all."""
import numpy as np
from scipy import signal

FS = 16000
N_FFT, HOP, N_MELS = 400, 160, 40
PARTIAL = 160
E = 256
LAYERS = 3
INT16_MAX = 32767


def hann_periodic(n):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n, dtype=np.float64) / n)


def slaney_filterbank(sr, n_fft, n_mels, fmin, fmax):
    """librosa 0.7's ``filters.mel`` (Slaney scale, Slaney area normalisation) -> float32 (n_mels, n_fft / 2 + 1)"""
    f_sp, min_log_hz, logstep = 200.0 / 3, 1000.0, np.log(6.4) / 27.0
    min_log_mel = min_log_hz / f_sp

    def to_mel(f):
        return min_log_mel + np.log(f / min_log_hz) / logstep if f >= min_log_hz else f / f_sp

    def to_hz(m):
        return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)
    freqs = np.linspace(0.0, sr / 2.0, 1 + n_fft // 2)
    edges = to_hz(np.linspace(to_mel(float(fmin)), to_mel(float(fmax)), n_mels + 2))
    ramps = edges[:, None] - freqs[None, :]
    lower = -ramps[:-2] / np.diff(edges)[:-1, None]
    upper = ramps[2:] / np.diff(edges)[1:, None]
    w = np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (edges[2:] - edges[:-2]))[:, None]
    return w.astype(np.float32)


def mel_frames(x, window, basis, hop, power):
    """x (L,), window (n_fft,), basis (n_mels, n_fft / 2 + 1), whatever their types -> float64 (L // hop + 1, n_mels)"""
    x = np.asarray(x, dtype=np.float64)
    window = np.asarray(window, dtype=np.float64)
    n_fft = window.shape[0]
    assert n_fft % 2 == 0 and x.shape[0] > n_fft // 2 and power in (1, 2)
    padded = np.pad(x, n_fft // 2, mode='reflect')
    T = x.shape[0] // hop + 1
    frames = np.stack([padded[t * hop:t * hop + n_fft] for t in range(T)])
    mag = np.abs(np.fft.rfft(frames * window[None, :], axis=1)) ** power
    return mag @ np.asarray(basis, dtype=np.float64).T


def mel_power(wav):
    """``wav_to_mel_spectrogram``: 400 / 160 / 40 bands over 0 .. 8000 Hz, power 2, periodic Hann"""
    return mel_frames(wav, hann_periodic(N_FFT), slaney_filterbank(FS, N_FFT, N_MELS, 0.0, FS / 2.0), HOP, 2)


def normalize_volume(wav, target_dbfs=-30, increase_only=True):
    wav = np.asarray(wav, dtype=np.float64)
    rms = np.sqrt(np.mean((wav * INT16_MAX) ** 2))
    if rms == 0:
        return wav
    change = target_dbfs - 20.0 * np.log10(rms / INT16_MAX)
    if change < 0 and increase_only:
        return wav
    return wav * 10.0 ** (change / 20.0)


def preprocess_wav(x, sr):
    """mono by the channels' mean, 16 kHz by scipy's polyphase filter, -30 dBFS; float32 as ``librosa.load`` hands it on"""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 2:
        x = x.mean(axis=1)
    if sr != FS:
        g = np.gcd(int(sr), FS)
        x = signal.resample_poly(x, FS // g, int(sr) // g)
    return normalize_volume(x).astype(np.float32)


def partial_slices(n_samples, rate=2, min_coverage=0.75):
    """``compute_partial_slices`` -> (list of (first, last + 1) mel frames, length the signal is zero-padded to)"""
    n_frames = int(np.ceil((n_samples + 1) / HOP))
    frame_step = int(np.round((FS / rate) / HOP))
    steps = max(n_frames - PARTIAL + frame_step + 1, 1)
    mel = [(i, i + PARTIAL) for i in range(0, steps, frame_step)]
    first, stop = mel[-1][0] * HOP, mel[-1][1] * HOP
    coverage = (n_samples - first) / (stop - first)
    if coverage < min_coverage and len(mel) > 1:
        mel = mel[:-1]
    return mel, mel[-1][1] * HOP


def seeded_weights(seed):
    """A state dict in resemblyzer's layout (without the similarity scalars): float32 arrays, uniform in +-1/16"""
    rs = np.random.RandomState(seed)
    k = 1.0 / np.sqrt(E)

    def draw(*shape):
        return rs.uniform(-k, k, size=shape).astype(np.float32)
    sd = {}
    for layer in range(LAYERS):
        sd['lstm.weight_ih_l%d' % layer] = draw(4 * E, N_MELS if layer == 0 else E)
        sd['lstm.weight_hh_l%d' % layer] = draw(4 * E, E)
        sd['lstm.bias_ih_l%d' % layer] = draw(4 * E)
        sd['lstm.bias_hh_l%d' % layer] = draw(4 * E)
    sd['linear.weight'] = draw(E, E)
    sd['linear.bias'] = draw(E)
    return sd


def _sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


def lstm_last_hidden(x, sd):
    """x (B, T, 40) -> (B, 256): h_{T-1} of the last of the three layers; gates i, f, g, o"""
    seq = np.asarray(x, dtype=np.float64)
    for layer in range(LAYERS):
        w_ih, w_hh, b_ih, b_hh = (np.asarray(sd['lstm.%s_l%d' % (n, layer)], dtype=np.float64)
                                  for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh'))
        B, T = seq.shape[:2]
        h, c = np.zeros((B, E)), np.zeros((B, E))
        out = np.empty((B, T, E))
        for t in range(T):
            gates = seq[:, t] @ w_ih.T + b_ih + h @ w_hh.T + b_hh
            i, f, g, o = _sigmoid(gates[:, :E]), _sigmoid(gates[:, E:2 * E]), np.tanh(gates[:, 2 * E:3 * E]), _sigmoid(gates[:, 3 * E:])
            c = f * c + i * g
            h = o * np.tanh(c)
            out[:, t] = h
        seq = out
    return seq[:, -1]


def head(h, w, b):
    """h (B, 256) -> (embed (256,), partials (B, 256)), float64"""
    v = np.maximum(np.asarray(h, np.float64) @ np.asarray(w, np.float64).T + np.asarray(b, np.float64), 0.0)
    norm = np.sqrt((v * v).sum(axis=1, keepdims=True))
    partial = np.divide(v, norm, out=np.zeros_like(v), where=norm > 0)
    mean = partial.mean(axis=0)
    n = np.sqrt((mean * mean).sum())
    return (mean / n if n > 0 else np.zeros_like(mean)), partial


def padded(wav):
    """the utterance zero-padded to its last window's end, and the windows' first frames"""
    wav = np.asarray(wav, dtype=np.float32)
    mel, pad_to = partial_slices(wav.shape[0])
    if pad_to > wav.shape[0]:
        wav = np.concatenate([wav, np.zeros(pad_to - wav.shape[0], np.float32)])
    return wav, [a for a, _ in mel]


def embed_from_mel(mel, starts, sd):
    windows = np.stack([mel[a:a + PARTIAL] for a in starts])
    return head(lstm_last_hidden(windows, sd), sd['linear.weight'], sd['linear.bias'])


def embed_utterance(wav, sd):
    """16 kHz float32 samples -> (embed (256,), partials (B, 256)), float64"""
    wav, starts = padded(wav)
    return embed_from_mel(mel_power(wav), starts, sd)


def speaker_embedding(samples, sr, sd, segment_len=960000):
    """``get_spk_emb`` -> (256,) float64: the plain mean of the segments' embeddings"""
    wav = preprocess_wav(samples, sr)
    n = max(1, wav.shape[0] // segment_len)
    return np.mean([embed_utterance(wav[segment_len * i:segment_len * (i + 1)], sd)[0] for i in range(n)], axis=0)
