"""The clip's f0 track on the device: what ``extract_f0_func_audiofile`` gets from ``sptk.rapt`` and ``speaker_normalization``
(Module1/src/autovc/retrain_version/vocoder_spec/extract_f0_func.py:120-125), as ``autovc.convert_mel`` takes it -- one value per
mel frame, in [0, 1] where voiced and -1e10 where unvoiced.

The algorithm is RAPT as published (Talkin 1995, the get_f0 defaults) with one NCCF pass at the full rate; its float64
statement, tests/f0_reference.py, is the contract of the two launches behind this module (apq_f0_candidates, apq_f0_track of
libapseq.so, csrc/seq/seq_f0.hip).  pysptk is not in the build image: parity with ``sptk.rapt`` itself is unpinned.

Two cases the reference leaves to a division by zero are defined here: a clip without a voiced frame stays all -1e10, and a
clip whose voiced log-f0 has zero deviation (one voiced frame, say) gets 0.5 on its voiced frames.

There is no host path: a call the library refuses raises."""
import numpy as np
import torch

from . import _seqapi as Q
from . import audio, ops

FS = audio.SAMPLE_RATE
UNVOICED = -1e10
GENDERS = {'F': (100, 600), 'M': (50, 250)}      # Hz; the converter passes 'F' (AutoVC_mel_Convertor_retrain_version.py:228)


def lag_range(gender):
    """(Kmin, Kmax) = (ceil(fs / hi), floor(fs / lo)) in samples"""
    if gender not in GENDERS:
        raise ValueError("f0: gender %r, served: 'F' (100 .. 600 Hz), 'M' (50 .. 250 Hz)" % (gender,))
    lo, hi = GENDERS[gender]
    return -(-FS // hi), FS // lo


def tracker_input(samples_16k):
    """samples at 16 kHz as read -> the float32 signal the tracker sees: ``float32(conditioned_signal) * 32768``"""
    return audio.conditioned_signal(samples_16k).astype(np.float32) * np.float32(32768)


def _device(device):
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != 'cuda':
        raise ValueError('f0: the tracker runs on the GPU, not on %s' % dev)
    return dev


def _check_tables(where, tab, T):
    for name, dt, shape in (('count', torch.int32, (T,)), ('lag', torch.float32, (T, Q.F0_CANDS)), ('val', torch.float32, (T, Q.F0_CANDS)),
                            ('rr', torch.float32, (T,)), ('s', torch.float32, (T,))):
        a = tab[name]
        if not (torch.is_tensor(a) and a.is_cuda and a.dtype == dt and tuple(a.shape) == shape and a.is_contiguous()):
            raise ValueError('f0.%s: %s must be a contiguous CUDA tensor of %s, shape %s' % (where, name, dt, shape))


def candidates(x, gender='F', device=None, frames=None, out=None):
    """x: the tracker's input (``tracker_input``; numpy or a float32 CUDA tensor), (L,).  One apq_f0_candidates launch.
    -> dict of device tensors: count (T,) int32, lag (T, 19), val (T, 19), rr (T,), s (T,); T = L // 256 + 1 unless ``frames``.
    ``out``: such a dict to write into."""
    kmin, kmax = lag_range(gender)
    if torch.is_tensor(x):
        if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 1):
            raise TypeError('f0.candidates takes a 1-d float32 CUDA tensor or a numpy array')
        x = x.contiguous()
    else:
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(-1))).to(_device(device))
    L = x.shape[0]
    T = L // Q.F0_HOP + 1 if frames is None else int(frames)
    if L < 1 or T < 1:
        raise ValueError('f0.candidates: %d samples, %d frames' % (L, T))
    dev = x.device
    tab = out
    if tab is None:
        tab = {'count': torch.empty(T, dtype=torch.int32, device=dev), 'lag': torch.empty(T, Q.F0_CANDS, device=dev),
               'val': torch.empty(T, Q.F0_CANDS, device=dev), 'rr': torch.empty(T, device=dev), 's': torch.empty(T, device=dev)}
    _check_tables('candidates', tab, T)
    with torch.cuda.device(dev):
        Q.check(Q.lib().apq_f0_candidates(ops._ptr(x), L, T, kmin, kmax, ops._ptr(tab['count']), ops._ptr(tab['lag']),
                                          ops._ptr(tab['val']), ops._ptr(tab['rr']), ops._ptr(tab['s']), ops._stream()), 'f0_candidates')
    return tab


def track(tab, gender='F', out=None):
    """The tables of ``candidates`` (device tensors) -> dict of device tensors: f0 (T,) float32 (f0_norm), path (T,) uint8
    (the chosen candidate, 255 = unvoiced), back (T, 20) uint8.  One apq_f0_track launch.  ``out``: such a dict to write into."""
    _, kmax = lag_range(gender)
    count, lag, val, rr, s = (tab[k] for k in ('count', 'lag', 'val', 'rr', 's'))
    T = count.shape[0]
    _check_tables('track', tab, T)
    dev = count.device
    if out is None:
        out = {'f0': torch.empty(T, device=dev), 'path': torch.empty(T, dtype=torch.uint8, device=dev),
               'back': torch.empty(T, Q.F0_STATES, dtype=torch.uint8, device=dev)}
    for name, dt, shape in (('f0', torch.float32, (T,)), ('path', torch.uint8, (T,)), ('back', torch.uint8, (T, Q.F0_STATES))):
        a = out[name]
        if not (torch.is_tensor(a) and a.device == dev and a.dtype == dt and tuple(a.shape) == shape and a.is_contiguous()):
            raise ValueError('f0.track: out[%r] must be a contiguous tensor of %s, shape %s, on %s' % (name, dt, shape, dev))
    with torch.cuda.device(dev):
        Q.check(Q.lib().apq_f0_track(ops._ptr(count), ops._ptr(lag), ops._ptr(val), ops._ptr(rr), ops._ptr(s), T, kmax, float(FS),
                                     ops._ptr(out['back']), ops._ptr(out['path']), ops._ptr(out['f0']), ops._stream()), 'f0_track')
    return out


def f0_from_tracker_input(x, gender='F', device=None):
    """``tracker_input`` (numpy, a float32 CUDA tensor or an ``audio_device.ClipAudio``) -> f0_norm (T,) float64 numpy: both
    launches, then the one copy to the host (which synchronises)"""
    if hasattr(x, 'tracker_input'):
        x = x.tracker_input()
        if not x.is_cuda:                                    # a clip the device front end did not serve: its host signal
            x = x.numpy()
    f0 = track(candidates(x, gender, device), gender)['f0'].cpu().numpy().astype(np.float64)
    return np.where(f0 < 0, UNVOICED, f0)


def f0_track(samples_16k, gender='F', device=None):
    """samples at 16 kHz (what ``audio.mel_spectrogram`` takes) -> f0_norm (T,) numpy, T the mel's frame count.
    An ``audio_device.ClipAudio`` (or the CUDA tensor of its ``tracker_input()``) is tracked from its device signal: nothing is
    conditioned on the host."""
    if hasattr(samples_16k, 'tracker_input'):
        return f0_from_tracker_input(samples_16k, gender, device)
    if torch.is_tensor(samples_16k):
        return f0_from_tracker_input(samples_16k, gender, device)
    return f0_from_tracker_input(tracker_input(samples_16k), gender, device)
