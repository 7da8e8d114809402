"""The clip's speaker embedding on the device: what ``get_spk_emb`` (Module1/thirdparty/resemblyer_util/speaker_emb.py, called at
main_end2end_module2.py:216-219) gets from resemblyzer's ``preprocess_wav`` and ``VoiceEncoder.embed_utterance`` -- the 256
numbers that condition the AutoVC converter (``autovc.convert_mel``) and Module1's speaker-aware branch.

Restated from resemblyzer as published (the package is not in the build image): 40 mel bands of a 400-point power spectrum every
10 ms (no log), windows of 160 frames every 50 frames, a 3-layer LSTM with 256 hidden units, linear + ReLU + L2 norm per window,
the mean over the windows and its L2 norm; per 60 s segment, then the plain mean over the segments.  Its float64 statement,
tests/speaker_reference.py, is the contract of the two launches behind this module (apq_mel_frames, apq_speaker_head of
libapseq.so, csrc/seq/seq_speaker.hip); the LSTM between them is ``nn.LSTM`` or, with ``lstm_backend='hip'``, the batched kernel
(lstm_hip.lstm_forward_batched).  Parity with resemblyzer / librosa themselves and with the published checkpoint is unpinned.

Two deviations from the reference:
  * ``preprocess_wav`` does NOT trim long silences: resemblyzer's third step needs webrtcvad, which is absent.  The embedding of a
    clip with long pauses therefore differs from the reference's.  A caller that has a voice-activity detector passes its
    per-sample mask as ``keep``.  The resampler is scipy's polyphase filter (audio.resample_to_16k), not resampy's.
  * a window whose ReLU output is all zero stays zero (and still counts in the mean), and an utterance whose windows are all zero
    gets the zero vector; the reference divides 0 by 0 there.  Digital silence keeps its level in ``normalize_volume`` for the
    same reason.

There is no host path: a call the library refuses raises.

    python -m animateportrait_amd.speaker --wav A.wav --encoder pretrained.pt --out emb.txt
"""
import argparse
import sys

import numpy as np
import torch
from torch import nn

from . import _seqapi as Q
from . import audio, lstm_hip, ops

FS = audio.SAMPLE_RATE
MEL_N_FFT, MEL_HOP, MEL_BANDS = 400, 160, 40       # 25 ms windows every 10 ms
PARTIAL_FRAMES = 160                               # a window: 1.6 s
EMBED = Q.SPK_E
SEGMENT_LEN = 960000                               # get_spk_emb: 60 s
LSTM_BACKENDS = ('library', 'hip')
INT16_MAX = 32767


def normalize_volume(wav, target_dbfs=-30, increase_only=True):
    """rms over ``wav * 32767``, gain ``10 ** ((target - 20 log10(rms / 32767)) / 20)``; with ``increase_only`` the signal is
    unchanged when the gain would lower its level.  Digital silence is returned as it is."""
    wav = np.asarray(wav)
    rms = np.sqrt(np.mean((wav.astype(np.float64) * INT16_MAX) ** 2))
    if rms == 0:
        return wav
    change = target_dbfs - 20.0 * np.log10(rms / INT16_MAX)
    if change < 0 and increase_only:
        return wav
    return wav * (10.0 ** (change / 20.0))


def preprocess_wav(x, sr, keep=None):
    """samples as read, (T,) or (T, channels), at ``sr`` Hz -> float32 (T',) at 16 kHz: the channels are AVERAGED (librosa.load's
    mono; the mel path of audio.py takes the first channel), resampled (scipy's polyphase filter, not resampy), raised to
    -30 dBFS.  Resemblyzer then trims long silences with webrtcvad; that step is NOT restated, so a clip with long pauses embeds
    differently here.  ``keep``: a boolean mask per 16 kHz sample from the caller's own detector, applied last."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim >= 2:
        x = x.mean(axis=1)
    x = normalize_volume(audio.resample_to_16k(x, sr))
    if keep is not None:
        keep = np.asarray(keep, dtype=bool)
        if keep.shape != x.shape:
            raise ValueError('speaker.preprocess_wav: keep has shape %s, the 16 kHz signal %s' % (keep.shape, x.shape))
        x = x[keep]
    return x.astype(np.float32)


def partial_slices(n_samples, rate=2, min_coverage=0.75):
    """``compute_partial_slices``: -> (starts, pad_to): the first mel frame of every 160-frame window, and the length in samples
    the signal is zero-padded to when it is shorter (the last window's end)."""
    if n_samples < 1:
        raise ValueError('speaker.partial_slices: %d samples' % n_samples)
    if not 0 < min_coverage <= 1:
        raise ValueError('speaker.partial_slices: min_coverage %r, served: (0, 1]' % (min_coverage,))
    n_frames = -(-(n_samples + 1) // MEL_HOP)
    frame_step = int(np.round(FS / rate / MEL_HOP))
    if not 0 < frame_step <= PARTIAL_FRAMES:
        raise ValueError('speaker.partial_slices: rate %r gives a step of %d frames, served: 1 .. %d' % (rate, frame_step, PARTIAL_FRAMES))
    steps = max(n_frames - PARTIAL_FRAMES + frame_step + 1, 1)
    starts = list(range(0, steps, frame_step))
    coverage = (n_samples - starts[-1] * MEL_HOP) / float(PARTIAL_FRAMES * MEL_HOP)
    if coverage < min_coverage and len(starts) > 1:
        starts = starts[:-1]
    return np.asarray(starts, dtype=np.int64), (starts[-1] + PARTIAL_FRAMES) * MEL_HOP


def _device(device):
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != 'cuda':
        raise ValueError('speaker: the embedding runs on the GPU, not on %s' % dev)
    return dev


def _is(t, dtype, dims):
    return torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and t.dim() == dims and t.is_contiguous()


def mel_frames(x, window, basis, hop, power, out=None):
    """One apq_mel_frames launch.  x (L,) float32, window (n_fft,) float64, basis (n_mels, n_fft / 2 + 1) float32, contiguous
    CUDA tensors -> (L // hop + 1, n_mels) float32: the mel bands of |STFT|^power of the reflect-padded signal."""
    if not (_is(x, torch.float32, 1) and _is(window, torch.float64, 1) and _is(basis, torch.float32, 2)):
        raise TypeError('speaker.mel_frames takes contiguous CUDA tensors: x float32 (L,), window float64 (n_fft,), basis float32 (n_mels, bins)')
    L, n_fft, n_mels = x.shape[0], window.shape[0], basis.shape[0]
    if basis.shape[1] != n_fft // 2 + 1 or hop < 1:
        raise ValueError('speaker.mel_frames: basis %s and hop %d do not go with n_fft %d' % (tuple(basis.shape), hop, n_fft))
    T = L // hop + 1
    if out is None:
        out = torch.empty(T, n_mels, dtype=torch.float32, device=x.device)
    elif not (_is(out, torch.float32, 2) and tuple(out.shape) == (T, n_mels) and out.device == x.device):
        raise ValueError('speaker.mel_frames: out must be a contiguous float32 tensor of shape %s on %s' % ((T, n_mels), x.device))
    with torch.cuda.device(x.device):
        Q.check(Q.lib().apq_mel_frames(ops._ptr(x), ops._ptr(window), ops._ptr(basis), ops._ptr(out), L, n_fft, int(hop), n_mels,
                                       int(power), ops._stream()), 'mel_frames')
    return out


_MEL_TABLES = {}


def _mel_tables(dev):
    key = str(dev)
    if key not in _MEL_TABLES:
        n = np.arange(MEL_N_FFT, dtype=np.float64)
        window = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / MEL_N_FFT)                  # periodic Hann
        basis = audio.mel_filterbank(FS, MEL_N_FFT, MEL_BANDS, 0.0, FS / 2.0)
        _MEL_TABLES[key] = (torch.from_numpy(window).to(dev), torch.from_numpy(np.ascontiguousarray(basis)).to(dev))
    return _MEL_TABLES[key]


def mel_power(wav, device=None):
    """``wav_to_mel_spectrogram``: 16 kHz samples (numpy or a float32 CUDA tensor), (L,) -> (L // 160 + 1, 40) float32 on the
    device: 400-point power spectrum, periodic Hann, 40 Slaney bands over 0 .. 8000 Hz.  There is no log.  One launch."""
    if torch.is_tensor(wav):
        x = wav.contiguous()
    else:
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(wav, dtype=np.float32).reshape(-1))).to(_device(device))
    window, basis = _mel_tables(x.device)
    return mel_frames(x, window, basis, MEL_HOP, 2)


def head(h, w, b, out=None):
    """One apq_speaker_head launch.  h (B, 256), w (256, 256), b (256,) float32 CUDA -> (embed (256,), partials (B, 256)).
    ``out``: such a pair to write into."""
    if not (_is(h, torch.float32, 2) and _is(w, torch.float32, 2) and _is(b, torch.float32, 1)) or h.shape[1] != EMBED or \
            tuple(w.shape) != (EMBED, EMBED) or b.shape[0] != EMBED:
        raise TypeError('speaker.head takes contiguous float32 CUDA tensors: h (B, 256), w (256, 256), b (256,)')
    B = h.shape[0]
    if out is None:
        out = (torch.empty(EMBED, device=h.device), torch.empty(B, EMBED, device=h.device))
    embed, partial = out
    if not (_is(embed, torch.float32, 1) and embed.shape[0] == EMBED and _is(partial, torch.float32, 2) and tuple(partial.shape) == (B, EMBED)
            and embed.device == h.device and partial.device == h.device):
        raise ValueError('speaker.head: out must be contiguous float32 tensors of shapes (256,) and (%d, 256) on %s' % (B, h.device))
    with torch.cuda.device(h.device):
        Q.check(Q.lib().apq_speaker_head(ops._ptr(h), ops._ptr(w), ops._ptr(b), ops._ptr(partial), ops._ptr(embed), B, ops._stream()),
                'speaker_head')
    return embed, partial


class VoiceEncoder(nn.Module):
    """resemblyzer's VoiceEncoder at inference.  ``lstm_backend``: 'library' = nn.LSTM (the default: a clip has a few dozen windows
    and the batched kernel gives a workgroup 16 of them; profiles/speaker_embed.json), 'hip' = one apq_lstm_layer_fwd launch per
    layer."""

    def __init__(self, lstm_backend='library'):
        super().__init__()
        if lstm_backend not in LSTM_BACKENDS:
            raise ValueError('speaker: LSTM backend %r (known: %s)' % (lstm_backend, ', '.join(LSTM_BACKENDS)))
        self.lstm_backend = lstm_backend
        self.lstm = nn.LSTM(MEL_BANDS, EMBED, 3, batch_first=True)
        self.linear = nn.Linear(EMBED, EMBED)

    def last_hidden(self, mels):
        """(B, 160, 40) windows -> (B, 256): the last layer's h_{T-1}"""
        if self.lstm_backend == 'hip':
            if not lstm_hip.supported_batched(self.lstm, mels):
                raise RuntimeError('speaker: the batched LSTM kernel does not serve this call (%s); there is no other path behind '
                                   "lstm_backend='hip'" % (Q.last_error() or 'the module is in training mode or autograd is on'))
            return lstm_hip.lstm_forward_batched(self.lstm, mels, last_only=True)
        return self.lstm(mels)[1][0][-1].contiguous()

    def embed_utterance(self, wav, rate=2, min_coverage=0.75):
        """16 kHz samples (L,) (``preprocess_wav``) -> (embed (256,), partials (B, 256)), device tensors: mel, the windows, three
        LSTM layers, the head."""
        dev = self.linear.weight.device
        if dev.type != 'cuda':
            raise ValueError('speaker: the embedding runs on the GPU; the encoder is on %s' % dev)
        wav = np.asarray(wav, dtype=np.float32).reshape(-1)
        starts, pad_to = partial_slices(wav.shape[0], rate, min_coverage)
        if pad_to > wav.shape[0]:
            wav = np.concatenate([wav, np.zeros(pad_to - wav.shape[0], np.float32)])
        with torch.no_grad():
            mel = mel_power(wav, dev)
            rows = torch.from_numpy(starts[:, None] + np.arange(PARTIAL_FRAMES)[None, :]).to(dev)
            mels = mel[rows]                                                         # (B, 160, 40)
            was_training = self.training
            self.eval()
            try:
                h = self.last_hidden(mels)
            finally:
                self.train(was_training)
            return head(h, self.linear.weight.contiguous(), self.linear.bias.contiguous())


def load_encoder(path, device=None, lstm_backend='library'):
    """resemblyzer's ``pretrained.pt``: a dict whose 'model_state' holds lstm.*, linear.* and the two similarity scalars of its
    training loss, which are accepted and ignored.  Every other missing or extra key is an error."""
    ck = torch.load(path, map_location='cpu')
    if not isinstance(ck, dict) or 'model_state' not in ck:
        raise RuntimeError("speaker.load_encoder: %s has no 'model_state' (resemblyzer's pretrained.pt layout)" % path)
    sd = {k: v for k, v in ck['model_state'].items() if k not in ('similarity_weight', 'similarity_bias')}
    enc = VoiceEncoder(lstm_backend)
    enc.load_state_dict(sd, strict=True)
    return enc.to(_device(device)).eval()


def speaker_embedding(samples, sr, encoder, segment_len=SEGMENT_LEN, keep=None):
    """``get_spk_emb``: samples as read -> (256,) float32 numpy: ``preprocess_wav``, ``max(1, len // segment_len)`` segments,
    one ``embed_utterance`` each, the plain mean of their embeddings (not renormalised)."""
    wav = preprocess_wav(samples, sr, keep)
    if wav.shape[0] < 1:
        raise ValueError('speaker.speaker_embedding: no samples')
    n = max(1, wav.shape[0] // int(segment_len))
    embeds = torch.stack([encoder.embed_utterance(wav[segment_len * i:segment_len * (i + 1)])[0] for i in range(n)])
    return embeds.cpu().numpy().astype(np.float64).mean(axis=0).astype(np.float32)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--wav', required=True)
    ap.add_argument('--encoder', required=True, help="resemblyzer's pretrained.pt")
    ap.add_argument('--out', required=True, help='txt, 256 numbers: what end2end --speaker_emb reads')
    ap.add_argument('--lstm', choices=LSTM_BACKENDS, default='library')
    ap.add_argument('--segment_len', type=int, default=SEGMENT_LEN)
    a = ap.parse_args(argv)
    if a.segment_len < 1:
        ap.error('--segment_len %d' % a.segment_len)
    x, sr = audio.read_wav(a.wav)
    emb = speaker_embedding(x, sr, load_encoder(a.encoder, None, a.lstm), a.segment_len)
    np.savetxt(a.out, emb)
    print('wrote', a.out)
    return 0


if __name__ == '__main__':
    sys.exit(main())
