"""The audio front end of audio.py on the device (opt-in: ``audio.clip_audio_features(..., backend='device')``, ``end2end
--audio_frontend device``): the decoded samples are uploaded once, and the resampler, the loudness rule, the zero-phase high-pass,
the dither and the log-mel spectrogram run on fp64 CUDA tensors in libapseq.so (csrc/seq/seq_audio.hip: apq_resample_poly,
apq_loudness_sumsq / apq_loudness_apply, apq_filtfilt, apq_logmel_frames).  audio.py is the contract:
  * the resampler agrees with ``scipy.signal.resample_poly`` to 1e-12 of the signal's peak (another summation order);
  * the loudness rule, the filter and the dither have the host's bits -- the filter because apq_filtfilt runs lfilter's own
    recurrence one sample after the other (a blocked parallel scan was measured and cannot hold 1e-10 for this filter, DESIGN.md
    4e-4);
  * the log-mel agrees to two fp32 steps.
One ``ClipAudio`` serves the mel windows and the f0 tracker (f0.py), so a clip is read, resampled, normalised and filtered once.
The only copy back to the host is the 8-byte sum of squares the loudness gain is computed from (audio.loudness_gain, the host's
own expression).  A CPU device, more than two channels, a rate whose filter the resampler does not serve and clips beyond the
loudness rule's exact range are computed by audio.py's functions instead, after one printed notice."""
import os

import numpy as np
import torch
from scipy import signal

from . import _seqapi as Q
from . import audio, ops

_TAPS = {}            # (up, down) -> fp64 numpy taps; (up, down, device) -> the device copy
_TABLES = {}          # device -> (window fp64, basis fp32)
_FILTER = []          # [(b, a, zi)] of the front end's high-pass
_DITHER = {'host': np.zeros(0)}          # 'host' -> RandomState(0).rand(n) so far; device -> its device copy


def rate_ratio(sr):
    """(up, down) of ``audio.resample_to_16k``"""
    g = np.gcd(int(sr), audio.SAMPLE_RATE)
    return audio.SAMPLE_RATE // g, int(sr) // g


def resample_taps(up, down):
    """The filter ``scipy.signal.resample_poly`` designs by default: a Kaiser-5.0 ``firwin`` of 20 max(up, down) + 1 taps with its
    cut-off at the lower Nyquist rate, times ``up``.  fp64 numpy, built once per (up, down)."""
    key = (int(up), int(down))
    if key not in _TAPS:
        max_rate = max(key)
        h = signal.firwin(2 * 10 * max_rate + 1, 1.0 / max_rate, window=('kaiser', 5.0)).astype(np.float64)
        h *= key[0]
        _TAPS[key] = h
    return _TAPS[key]


def _device_taps(up, down, dev):
    key = (int(up), int(down), str(dev))
    if key not in _TAPS:
        _TAPS[key] = torch.from_numpy(resample_taps(up, down)).to(dev)
    return _TAPS[key]


def dither_host(n):
    """``np.random.RandomState(0).rand(n)``: a prefix of one fixed sequence, made once and grown on demand"""
    if _DITHER['host'].shape[0] < n:
        _DITHER['host'] = np.random.RandomState(0).rand(max(int(n), 2 * _DITHER['host'].shape[0]))
    return _DITHER['host'][:n]


def dither_table(n, dev):
    """... as a device fp64 tensor"""
    key = str(dev)
    if key not in _DITHER or _DITHER[key].shape[0] < n:
        dither_host(n)
        _DITHER[key] = torch.from_numpy(_DITHER['host']).to(dev)
    return _DITHER[key][:n]


def highpass():
    """(b, a, zi) of ``audio.conditioned_signal``'s 5th-order 30 Hz Butterworth high-pass, fp64 numpy"""
    if not _FILTER:
        b, a = signal.butter(5, 30.0 / (0.5 * audio.SAMPLE_RATE), btype='high', analog=False)
        _FILTER.append((np.ascontiguousarray(b, np.float64), np.ascontiguousarray(a, np.float64),
                        np.ascontiguousarray(signal.lfilter_zi(b, a), np.float64)))
    return _FILTER[0]


def _tables(dev):
    key = str(dev)
    if key not in _TABLES:
        window = signal.get_window('hann', audio.N_FFT, fftbins=True).astype(np.float64)
        _TABLES[key] = (torch.from_numpy(window).to(dev), torch.from_numpy(np.ascontiguousarray(audio.mel_filterbank())).to(dev))
    return _TABLES[key]


def _f64(t, dims):
    return torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float64 and t.dim() == dims and t.is_contiguous()


# ------------------------------------------------------------------------------------------------------------- the launches
def resample_poly(x, up, down, taps=None):
    """One apq_resample_poly launch.  x (L, C) fp64 contiguous CUDA -> (ceil(L up / down), C): ``signal.resample_poly(x, up, down,
    axis=0)``; ``taps``: a device fp64 filter instead of scipy's default."""
    if not _f64(x, 2):
        raise TypeError('audio_device.resample_poly takes a contiguous float64 CUDA tensor (L, C)')
    h = _device_taps(up, down, x.device) if taps is None else taps
    L, C = x.shape
    y = torch.empty((-(-L * int(up) // int(down)), C), dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        Q.check(Q.lib().apq_resample_poly(ops._ptr(x), ops._ptr(h), ops._ptr(y), L, C, h.shape[0], int(up), int(down), ops._stream()),
                'resample_poly')
    return y


def loudness_sumsq(x):
    """Both launches of apq_loudness_sumsq on a contiguous fp64 CUDA tensor of any shape and the 8-byte copy back (which
    synchronises): the exact integer sum of the squared 16-bit samples."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float64 and x.is_contiguous()):
        raise TypeError('audio_device.loudness_sumsq takes a contiguous float64 CUDA tensor')
    n = x.numel()
    with torch.cuda.device(x.device):
        ws = torch.empty(max(1, int(Q.lib().apq_loudness_workspace_bytes(min(n, Q.LOUD_MAX_N))) // 8) + 1, dtype=torch.int64, device=x.device)
        Q.check(Q.lib().apq_loudness_sumsq(ops._ptr(x), ops._ptr(ws[1:]), ops._ptr(ws), n, ops._stream()), 'loudness_sumsq')
    return int(ws[:1].cpu()[0])


def normalize_loudness(x, target_dbfs=-20.0):
    """``audio.normalize_loudness`` on a contiguous fp64 CUDA tensor, bit for bit: the sum of squares on the device, the rms and
    the gain on the host with the host's expression, the gain applied on the device."""
    s = loudness_sumsq(x)
    n = x.numel()
    rms = int(np.sqrt(np.float64(s) / n))                      # np.mean of exactly representable sums, then audioop's truncation
    y = torch.empty_like(x)
    gain = audio.loudness_gain(rms, target_dbfs) if rms else 0.0
    with torch.cuda.device(x.device):
        Q.check(Q.lib().apq_loudness_apply(ops._ptr(x), ops._ptr(y), n, float(gain), 1 if rms else 0, ops._stream()), 'loudness_apply')
    return y


def filtfilt(b, a, x, zi=None):
    """One apq_filtfilt launch: ``signal.filtfilt(b, a, x)`` with scipy's defaults on a contiguous fp64 CUDA tensor (L,); b and a
    are host arrays of equal length."""
    if not _f64(x, 1):
        raise TypeError('audio_device.filtfilt takes a contiguous float64 CUDA tensor (L,)')
    b = np.ascontiguousarray(b, np.float64).reshape(-1)
    a = np.ascontiguousarray(a, np.float64).reshape(-1)
    if b.shape != a.shape:
        raise ValueError('audio_device.filtfilt: b has %d coefficients, a %d' % (b.shape[0], a.shape[0]))
    zi = np.ascontiguousarray(signal.lfilter_zi(b, a) if zi is None else zi, np.float64).reshape(-1)
    L, M = x.shape[0], b.shape[0] - 1
    if zi.shape[0] != M:
        raise ValueError('audio_device.filtfilt: zi has %d values, the filter order is %d' % (zi.shape[0], M))
    y = torch.empty_like(x)
    with torch.cuda.device(x.device):
        ws = torch.empty(max(1, int(Q.lib().apq_filtfilt_workspace_bytes(L, M)) // 8), dtype=torch.float64, device=x.device)
        Q.check(Q.lib().apq_filtfilt(ops._ptr(x), ops._ptr(y), b.ctypes.data, a.ctypes.data, zi.ctypes.data, ops._ptr(ws), L, M,
                                     ops._stream()), 'filtfilt')
    return y


def logmel_frames(x):
    """One apq_logmel_frames launch: conditioned samples (L,) fp64 CUDA -> (L // 256 + 1, 80) float32, ``audio.mel_spectrogram``'s
    map of the 1024-point STFT."""
    if not _f64(x, 1):
        raise TypeError('audio_device.logmel_frames takes a contiguous float64 CUDA tensor (L,)')
    window, basis = _tables(x.device)
    out = torch.empty((x.shape[0] // audio.HOP + 1, audio.N_MELS), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        Q.check(Q.lib().apq_logmel_frames(ops._ptr(x), ops._ptr(window), ops._ptr(basis), ops._ptr(out), x.shape[0], audio.N_FFT,
                                          audio.HOP, audio.N_MELS, ops._stream()), 'logmel_frames')
    return out


def window_frames_device(mel, num_window_frames=audio.WINDOW_FRAMES):
    """``audio.window_frames`` (step 1) as a view: (T, 80) tensor -> (max(T - 18, 0), 18, 80)"""
    n = mel.shape[0] - num_window_frames
    if n <= 0:
        return mel.new_zeros((0, num_window_frames) + tuple(mel.shape[1:]))
    return mel.unfold(0, num_window_frames, 1)[:n].permute(0, 2, 1)


# ------------------------------------------------------------------------------------------------------------------ the clip
def refusal(sr, length, channels, normalize=True, device=None):
    """Why the device front end does not serve such a clip (a string), or None"""
    dev = torch.device(device) if device is not None else None
    if dev is not None and dev.type != 'cuda':
        return 'the device is %s' % dev
    if dev is None and not torch.cuda.is_available():
        return 'there is no GPU'
    if channels > Q.RS_MAX_C:
        return '%d channels (served: up to %d)' % (channels, Q.RS_MAX_C)
    up, down = rate_ratio(sr)
    n16 = -(-length * up // down)
    if (up, down) != (1, 1) and (max(up, down) > Q.RS_MAX_RATE or 20 * max(up, down) + 1 > Q.RS_MAX_TAPS):
        return 'the rate %d Hz needs a filter of %d taps (served: up to %d)' % (sr, 20 * max(up, down) + 1, Q.RS_MAX_TAPS)
    if normalize and n16 * channels > Q.LOUD_MAX_N:
        return '%d samples (the loudness rule is exact up to %d)' % (n16 * channels, Q.LOUD_MAX_N)
    if n16 <= audio.N_FFT // 2:
        return '%d samples at 16 kHz (served: above %d)' % (n16, audio.N_FFT // 2)
    return None


class ClipAudio:
    """The clip's samples on the device and what the front end makes of them, each computed on first use and kept:
      ``samples_16k`` (T, C) fp64, ``normalized`` (T, C) fp64, ``conditioned`` (T or T + 1,) fp64 (``audio.conditioned_signal``),
      ``mel()`` (frames, 80) float32, ``tracker_input()`` (T or T + 1,) float32 (``f0.tracker_input``).
    path_or_samples: a wav file, or samples as ``audio.read_wav`` returns them with their rate ``sr`` (default 16 kHz).
    ``on_device`` is False when audio.py computed them instead (module docstring); the tensors then hold the host's results, on
    ``device``."""

    def __init__(self, path_or_samples, sr=None, device=None, normalize=True):
        if isinstance(path_or_samples, (str, os.PathLike)):
            x, file_sr = audio.read_wav(path_or_samples)
            sr = file_sr if sr is None else sr
        else:
            x = np.asarray(path_or_samples, dtype=np.float64)
        if x.ndim not in (1, 2) or x.shape[0] < 1:
            raise ValueError('ClipAudio: samples of shape %s' % (x.shape,))
        self.sr = audio.SAMPLE_RATE if sr is None else int(sr)
        self.normalize = bool(normalize)
        self.mono = x.ndim == 1
        if device is None:
            device = torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else torch.device('cpu')
        self.device = torch.device(device)
        self.reason = refusal(self.sr, x.shape[0], 1 if self.mono else x.shape[1], self.normalize, self.device)
        self.on_device = self.reason is None
        self._host = x
        self._cache = {}
        if self.on_device:
            self._raw = torch.from_numpy(np.array(x.reshape(x.shape[0], -1), order='C')).to(self.device)      # the one upload
        else:
            print('audio_device: %s; the audio front end runs on the host (audio.py)' % self.reason)

    def _get(self, name, make):
        if name not in self._cache:
            self._cache[name] = make()
        return self._cache[name]

    # ---- the host's results, when the device does not serve the clip
    def _host_stage(self, name):
        def make():
            if name == 'samples_16k':
                return audio.resample_to_16k(self._host, self.sr)
            if name == 'normalized':
                x = self._host_stage('samples_16k')
                return audio.normalize_loudness(x) if self.normalize else x
            if name == 'conditioned':
                return audio.conditioned_signal(self._host_stage('normalized'))
            return audio.mel_spectrogram(self._host_stage('normalized')).astype(np.float32)
        return self._get('host_' + name, make)

    def _from_host(self, name):
        a = self._host_stage(name)
        if name in ('samples_16k', 'normalized'):
            a = a.reshape(a.shape[0], -1)
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    @property
    def samples_16k(self):
        def make():
            if not self.on_device:
                return self._from_host('samples_16k')
            up, down = rate_ratio(self.sr)
            return self._raw if (up, down) == (1, 1) else resample_poly(self._raw, up, down)
        return self._get('samples_16k', make)

    @property
    def normalized(self):
        def make():
            if not self.on_device:
                return self._from_host('normalized')
            return normalize_loudness(self.samples_16k) if self.normalize else self.samples_16k
        return self._get('normalized', make)

    @property
    def conditioned(self):
        def make():
            if not self.on_device:
                return self._from_host('conditioned')
            x = self.normalized[:, 0]
            if x.shape[0] % 256 == 0:
                x = torch.cat((x, torch.full((1,), 1e-06, dtype=torch.float64, device=x.device)))
            b, a, zi = highpass()
            y = filtfilt(b, a, x.contiguous(), zi)
            return y * 0.95 + (dither_table(y.shape[0], y.device) - 0.5) * 1e-06      # numpy's operations in numpy's order
        return self._get('conditioned', make)

    def mel(self):
        return self._get('mel', lambda: logmel_frames(self.conditioned) if self.on_device else self._from_host('mel'))

    def tracker_input(self):
        return self._get('tracker_input', lambda: self.conditioned.to(torch.float32) * 32768)


def clip_audio_features(path, max_frames=None, normalize=True, converter=None, device=None, au_mean_std=None):
    """``audio.clip_audio_features(..., backend='device')``: the windows (F, 18, 80) as a float32 CUDA tensor.  ``path`` may be a
    ``ClipAudio``.  The converter is called with the device mel and may return a tensor or an array.  A clip the device does not
    serve gives the host's windows (numpy), after ClipAudio's notice.  ``au_mean_std``: as in ``audio.clip_audio_features``."""
    clip = path if isinstance(path, ClipAudio) else ClipAudio(path, device=device, normalize=normalize)
    if not clip.on_device:
        s = clip._host_stage('mel')
        if converter is not None:
            s = np.asarray(converter(s), dtype=np.float32)
        w = audio.window_frames(audio.normalize_mel(s, au_mean_std))
        return w if max_frames is None else w[:max_frames]
    s = clip.mel()
    if converter is not None:
        s = torch.as_tensor(converter(s), dtype=torch.float32, device=s.device)
    w = window_frames_device(audio.normalize_mel(s, au_mean_std))
    return (w if max_frames is None else w[:max_frames]).contiguous()
