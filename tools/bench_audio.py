"""What the audio front end costs on either side (audio.py on the host, audio_device.py / csrc/seq/seq_audio.hip on the device), for
the example clip tests/golden/female12.wav as it is (16 kHz, 13 s, stereo) and for a 44.1 kHz version of it that this tool makes
with scipy on the host before anything is timed.

The stage is timed from samples in host memory to what its two consumers read on the device:
  host    resample_to_16k, normalize_loudness, mel_spectrogram, window_frames and the upload of the windows; then
          f0.tracker_input (which conditions the signal a second time, as end2end does today) and its upload
  device  ClipAudio: one upload of the samples, resampler, loudness (with its 8-byte read-back), filtfilt, dither, log-mel,
          windows; then tracker_input() from the same conditioned signal
Both backends in ONE process, in alternated rounds, a synchronise before and behind each leg, medians reported.  Each entry point's
time on its own comes from HIP events around repeated launches on the 16 kHz clip's tensors (no profiler is used).

    python tools/bench_audio.py --out profiles/audio_frontend.json

Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
from scipy import signal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def event_ms(fn, reps):
    """median over ``reps`` of the device time of one ``fn()`` between two events"""
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--rounds', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None, help='write the result as JSON here as well')
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('bench_audio: no GPU')
    from animateportrait_amd import audio, audio_device as ad, f0
    dev = torch.device('cuda:0')
    x16, sr = audio.read_wav(os.path.join(ROOT, 'tests', 'golden', 'female12.wav'))
    x44 = signal.resample_poly(x16, 441, 160, axis=0)
    x44 = np.clip(np.round(x44 * 32768.0), -32768, 32767) / 32768.0           # what a 16-bit file at that rate holds
    inputs = {'16000': (x16, sr), '44100': (x44, 44100)}

    def host(x, rate):
        n = audio.normalize_loudness(audio.resample_to_16k(x, rate))
        w = torch.from_numpy(audio.window_frames(audio.mel_spectrogram(n).astype(np.float32))).to(dev)
        t = torch.from_numpy(f0.tracker_input(n)).to(dev)
        return w, t

    def device(x, rate):
        clip = ad.ClipAudio(x, rate, device=dev)
        return ad.clip_audio_features(clip), clip.tracker_input()

    legs = {'%s_%s' % (b, r): (fn, inputs[r]) for r in inputs for b, fn in (('host', host), ('device', device))}
    names = list(legs)
    times, outs = {n: [] for n in names}, {}
    for r in range(a.warmup + a.rounds):
        for n in (names if r % 2 == 0 else names[::-1]):
            fn, (x, rate) = legs[n]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs[n] = fn(x, rate)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if r >= a.warmup:
                times[n].append(dt)
    res = {'device': torch.cuda.get_device_name(0), 'clip': 'tests/golden/female12.wav', 'rounds': a.rounds, 'warmup': a.warmup,
           'unit': 'ms (median over the rounds; min and max beside it)',
           'stage': 'samples in host memory -> mel windows and tracker input on the device, a synchronise before and behind',
           'samples_16k': int(x16.shape[0]), 'samples_44k': int(x44.shape[0]), 'channels': int(x16.shape[1])}
    for n in names:
        res[n] = {'median': 1e3 * statistics.median(times[n]), 'min': 1e3 * min(times[n]), 'max': 1e3 * max(times[n])}
    for r in inputs:
        h, d = res['host_' + r]['median'], res['device_' + r]['median']
        res['winner_' + r] = 'device' if d < h else 'host'
        res['device_over_host_' + r] = d / h
        res['windows_linf_' + r] = float((outs['device_' + r][0] - outs['host_' + r][0]).abs().max())
        res['tracker_input_equal_share_' + r] = float((outs['device_' + r][1] == outs['host_' + r][1]).double().mean())

    # each entry point on its own, on the 16 kHz clip's tensors (and the 44.1 kHz samples for the resampler)
    clip = ad.ClipAudio(x16, sr, device=dev)
    raw44 = torch.from_numpy(np.ascontiguousarray(x44)).to(dev)
    norm, cond = clip.normalized, clip.conditioned
    mono = norm[:, 0].contiguous()
    b, a_, zi = ad.highpass()
    ad.resample_poly(raw44, 160, 441)
    kernels = {'apq_resample_poly (44.1 kHz -> 16 kHz, 2 channels)': lambda: ad.resample_poly(raw44, 160, 441),
               'apq_loudness_sumsq + 8-byte read-back': lambda: ad.loudness_sumsq(clip.samples_16k),
               'apq_loudness_sumsq + read-back + apq_loudness_apply': lambda: ad.normalize_loudness(clip.samples_16k),
               'apq_filtfilt': lambda: ad.filtfilt(b, a_, mono, zi),
               'apq_logmel_frames': lambda: ad.logmel_frames(cond)}
    res['kernels_ms_hip_events'] = {k: event_ms(fn, 9) for k, fn in kernels.items()}
    t0 = time.perf_counter()
    for _ in range(5):
        signal.filtfilt(b, a_, audio.normalize_loudness(x16)[:, 0])
    res['host_filtfilt_ms'] = 1e3 * (time.perf_counter() - t0) / 5       # includes normalize_loudness; see host_normalize_ms
    t0 = time.perf_counter()
    for _ in range(5):
        audio.normalize_loudness(x16)
    res['host_normalize_ms'] = 1e3 * (time.perf_counter() - t0) / 5
    res['not_measured'] = 'end2end as a whole with either front end; clips longer than the example; other GPUs'
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
