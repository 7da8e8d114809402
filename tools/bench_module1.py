"""Where the Module1 stage of a clip spends its time, and what the batched LSTM kernel (libapseq.so) changes about it.

For the example clip's 625 windows (tests/golden/female12.wav; both landmark networks at the reference's configuration with
seeded random weights, as bench.py's stream leg builds them) ``module1.predict_landmarks_speaker_aware`` is timed with both
LSTM backends in ONE process, in alternated rounds, and split into
  (a) networks: the forward passes of the two networks, a device synchronise before and after each, and
  (b) host:     everything else in the call -- the .cpu() copies and landmark_host (_savgol, calib_baseline, solve_inverse_lip).
Medians over the rounds are reported.  Then the kernel alone: one apq_lstm_layer_fwd launch at B = 512, T = 18 and
I in {80, 161, 256} between device events, next to a one-layer nn.LSTM of the same shape.

Then the post-processing backends (module1.set_post_backend: 'host' = numpy / scipy, 'device' = the apq_* calls of libapseq.so),
again alternated in the same process on the same windows, LSTM backend as configured: the stage split as above (for 'device' the
rest is launches and kernels instead of host work), ``to_image_landmarks`` on the stage's output as a line of its own (it is not
part of the stage time above), and both once more with the networks unwrapped -- no synchronise inside the stage, the time a
clip sees.

    python tools/bench_module1.py --out profiles/module1_lstm.json --post_out profiles/module1_post.json

Needs a GPU: there is no CPU mode, a time taken without the device would say nothing."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


class Timed(torch.nn.Module):
    """The network with a synchronise on both sides of its forward; the time between them is summed in ``self.seconds``."""

    def __init__(self, net):
        super().__init__()
        self.net, self.seconds = net, 0.0

    def forward(self, *args):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = self.net(*args)
        torch.cuda.synchronize()
        self.seconds += time.perf_counter() - t0
        return out


def stage_once(m1, pose, content, au, spk, fid):
    pose.seconds = content.seconds = 0.0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fl = m1.predict_landmarks_speaker_aware(pose, content, au, spk, fid)
    torch.cuda.synchronize()
    total = time.perf_counter() - t0
    nets = pose.seconds + content.seconds
    return fl, {'total': total, 'networks': nets, 'host': total - nets, 'pose_net': pose.seconds, 'content_net': content.seconds}


def post_once(m1, pose, content, au, spk, fid):
    """One stage + to_image_landmarks: split (networks wrapped in ``Timed``) and unsplit (the bare networks)."""
    fl, t = stage_once(m1, pose, content, au, spk, fid)
    t['rest'] = t.pop('host')            # everything outside the networks: host work, or launches and kernels
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    img = m1.to_image_landmarks(fl, scale=0.01, shift=(-128.0, -128.0), rng=np.random.RandomState(0))
    torch.cuda.synchronize()
    t['to_image_landmarks'] = time.perf_counter() - t0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fl2 = m1.predict_landmarks_speaker_aware(pose.net, content.net, au, spk, fid)
    torch.cuda.synchronize()
    t['stage_unsplit'] = time.perf_counter() - t0
    t0 = time.perf_counter()
    m1.to_image_landmarks(fl2, scale=0.01, shift=(-128.0, -128.0), rng=np.random.RandomState(0))
    torch.cuda.synchronize()
    t['stage_and_image_unsplit'] = t['stage_unsplit'] + time.perf_counter() - t0
    return fl, img, t


def _medians(times):
    return {k: {'median': 1e3 * statistics.median(t[k] for t in times), 'min': 1e3 * min(t[k] for t in times),
                'max': 1e3 * max(t[k] for t in times)} for k in times[0]}


def post_rounds(m1, pose, content, au, spk, fid, rounds, warmup):
    backends = ('host', 'device')
    prev = m1.get_post_backend()
    times, outs = {b: [] for b in backends}, {}
    try:
        for r in range(warmup + rounds):
            for b in (backends if r % 2 == 0 else backends[::-1]):
                m1.set_post_backend(b)
                fl, img, t = post_once(m1, pose, content, au, spk, fid)
                outs[b] = (np.asarray(fl.cpu() if torch.is_tensor(fl) else fl), np.asarray(img.cpu() if torch.is_tensor(img) else img))
                if r >= warmup:
                    times[b].append(t)
    finally:
        m1.set_post_backend(prev)
    res = {b: _medians(times[b]) for b in backends}
    res['lstm_backend'] = m1.get_lstm_backend()
    res['landmarks_linf_device_vs_host'] = float(np.abs(outs['device'][0] - outs['host'][0]).max())
    res['landmarks_range'] = float(np.abs(outs['host'][0]).max())
    res['image_landmarks_linf_device_vs_host_px'] = float(np.abs(outs['device'][1] - outs['host'][1]).max())
    return res


def kernel_times(dev, reps):
    """ms per launch of one layer at B = 512, T = 18, full output -- the kernel and the library's one-layer LSTM"""
    from animateportrait_amd import _seqapi as Q, ops
    rows = []
    for i in (80, 161, 256):
        torch.manual_seed(i)
        lstm = torch.nn.LSTM(i, 256, 1, batch_first=True).to(dev).eval()
        x = torch.randn(512, 18, i, device=dev)
        out = torch.empty(512, 18, 256, device=dev)
        w = [getattr(lstm, n + '_l0').contiguous() for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')]
        args = [ops._ptr(a) for a in [x] + w + [out]]

        def hip(last_only=0):
            Q.check(Q.lib().apq_lstm_layer_fwd(*args, 512, 18, i, 256, last_only, ops._stream()), 'lstm_layer_fwd')

        def library():
            with torch.no_grad():
                lstm(x)

        row = {'B': 512, 'T': 18, 'I': i, 'H': 256}
        for name, fn in (('hip_ms', hip), ('library_ms', library)):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            row[name] = e0.elapsed_time(e1) / reps
        with torch.no_grad():
            row['linf_vs_library'] = float((out - lstm(x)[0]).abs().max())
        # 2 (I + H) 4H multiply-adds per row and step
        row['hip_tflops'] = 2.0 * (i + 256) * 1024 * 512 * 18 / (row['hip_ms'] * 1e-3) / 1e12
        rows.append(row)
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--rounds', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--kernel_reps', type=int, default=20)
    ap.add_argument('--frames', type=int, default=625)
    ap.add_argument('--out', default=None, help='write the result as JSON here as well')
    ap.add_argument('--post_out', default=None, help='write the post-processing backends\' part of the result as JSON here')
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('bench_module1: no GPU')
    dev = torch.device('cuda:0')
    from animateportrait_amd import audio, module1 as m1
    torch.manual_seed(1234)
    content = Timed(m1.Audio2LandmarkContent(use_prior_net=True, drop_out=0.5).to(dev).eval())
    pose = Timed(m1.Audio2LandmarkPos(drop_out=0.5).to(dev).eval())
    spk = torch.randn(256, generator=torch.Generator().manual_seed(7))
    fid = torch.randn(204, generator=torch.Generator().manual_seed(8)) * 0.1
    au = audio.clip_audio_features(os.path.join(ROOT, 'tests', 'golden', 'female12.wav'), max_frames=a.frames)
    assert au.shape == (a.frames, 18, 80), au.shape
    backends = ('library', 'hip')
    prev = m1.get_lstm_backend()
    times = {b: [] for b in backends}
    fls = {}
    try:
        for r in range(a.warmup + a.rounds):
            for b in (backends if r % 2 == 0 else backends[::-1]):
                m1.set_lstm_backend(b)
                fls[b], t = stage_once(m1, pose, content, au, spk, fid)
                if r >= a.warmup:
                    times[b].append(t)
    finally:
        m1.set_lstm_backend(prev)
    res = {'device': torch.cuda.get_device_name(0), 'windows': a.frames, 'segments': [min(512, a.frames - j) for j in range(0, a.frames, 512)],
           'rounds': a.rounds, 'warmup': a.warmup, 'unit': 'ms (median over the rounds; min and max beside it)', 'stage': {}}
    for b in backends:
        res['stage'][b] = {k: {'median': 1e3 * statistics.median(t[k] for t in times[b]), 'min': 1e3 * min(t[k] for t in times[b]),
                               'max': 1e3 * max(t[k] for t in times[b])} for k in times[b][0]}
    res['landmarks_linf_hip_vs_library'] = float(np.abs(fls['hip'] - fls['library']).max())
    res['landmarks_range'] = float(np.abs(fls['library']).max())
    res['kernel_per_layer'] = kernel_times(dev, a.kernel_reps)
    post = {k: res[k] for k in ('device', 'windows', 'segments', 'rounds', 'warmup', 'unit')}
    post['post'] = post_rounds(m1, pose, content, au, spk, fid, a.rounds, a.warmup)
    res['post'] = post['post']
    text = json.dumps(res, indent=1)
    print(text)
    if a.post_out:
        os.makedirs(os.path.dirname(os.path.abspath(a.post_out)), exist_ok=True)
        with open(a.post_out, 'w') as f:
            f.write(json.dumps(post, indent=1) + '\n')
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
