"""What the clip's f0 track costs (f0.py, csrc/seq/seq_f0.hip), for the example clip tests/golden/female12.wav (818 frames).

Three legs in ONE process, in alternated rounds, medians reported (as tools/bench_module1.py does):
  device_with_conditioning     f0.f0_track: the host's filtfilt / dither (audio.conditioned_signal), the upload, both launches,
                               the copy of the track to the host
  device_without_conditioning  f0.f0_from_tracker_input on the conditioned signal: upload, both launches, copy
  host_restatement             tests/f0_reference.py: the float64 numpy statement of the same algorithm.  It is NOT pysptk's rapt
                               (absent from the build image), only the contract the kernels are tested against.
Single kernels are not timed here: the two launches are only seen together, between a synchronise before and the copy behind.

    python tools/bench_f0.py --out profiles/f0_track.json

Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--rounds', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None, help='write the result as JSON here as well')
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('bench_f0: no GPU')
    from animateportrait_amd import audio, f0
    import f0_reference as R
    dev = torch.device('cuda:0')
    x, sr = audio.read_wav(os.path.join(ROOT, 'tests', 'golden', 'female12.wav'))
    x = audio.normalize_loudness(audio.resample_to_16k(x, sr))
    xt = f0.tracker_input(x)
    legs = {'device_with_conditioning': lambda: f0.f0_track(x, 'F', dev),
            'device_without_conditioning': lambda: f0.f0_from_tracker_input(xt, 'F', dev),
            'host_restatement': lambda: R.f0_track(xt, 'F')['f0_norm']}
    names = list(legs)
    times, outs = {n: [] for n in names}, {}
    for r in range(a.warmup + a.rounds):
        for n in (names if r % 2 == 0 else names[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs[n] = legs[n]()
            dt = time.perf_counter() - t0
            if r >= a.warmup:
                times[n].append(dt)
    res = {'device': torch.cuda.get_device_name(0), 'clip': 'tests/golden/female12.wav', 'frames': int(len(outs[names[0]])),
           'samples': int(len(xt)), 'rounds': a.rounds, 'warmup': a.warmup, 'unit': 'ms (median over the rounds; min and max beside it)',
           'host_leg': 'tests/f0_reference.py (float64 numpy restatement), not pysptk', 'single_kernels_timed': False}
    for n in names:
        res[n] = {'median': 1e3 * statistics.median(times[n]), 'min': 1e3 * min(times[n]), 'max': 1e3 * max(times[n])}
    voiced = outs['host_restatement'] >= 0
    res['voiced_frames'] = int(voiced.sum())
    res['frames_voicing_differs'] = int(((outs['device_with_conditioning'] >= 0) != voiced).sum())
    res['f0_norm_linf_device_vs_restatement'] = float(np.abs(outs['device_with_conditioning'] - outs['host_restatement'])[voiced & (outs['device_with_conditioning'] >= 0)].max())
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
