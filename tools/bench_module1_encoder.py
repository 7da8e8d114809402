"""What the encoder kernels of libapseq.so (csrc/seq/seq_encoder.hip, ``module1.set_encoder_backend('hip')``) change about the pose
network's self-attention encoder: both backends alternated in ONE process, medians over the rounds, a device synchronise on both
sides of every timed call.

  * the encoder alone (seeded weights, in_size 512) at T = 512 and T = 113 -- the two segments of the example clip;
  * the pose network (``Audio2LandmarkPos``) on 512 windows;
  * the Module1 stage of the example clip's 625 windows (``predict_landmarks_speaker_aware``, as tools/bench_module1.py times it);
  * the kernel launches of each encoder path at T = 512, COUNTED with the profiler's device activity records;
  * the parity errors per shape: L-inf of each path to the float64 statement (tests/encoder_reference.py).

    python tools/bench_module1_encoder.py --out profiles/module1_encoder.json

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
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

BACKENDS = ('library', 'hip')


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def alternate(m1, fn, rounds, warmup):
    """ms of ``fn()`` under each backend: {'library': {median, min, max}, 'hip': ...}, the backends taking turns at going first"""
    prev = m1.get_encoder_backend()
    times = {b: [] for b in BACKENDS}
    try:
        for r in range(warmup + rounds):
            for b in (BACKENDS if r % 2 == 0 else BACKENDS[::-1]):
                m1.set_encoder_backend(b)
                _, s = timed(fn)
                if r >= warmup:
                    times[b].append(s)
    finally:
        m1.set_encoder_backend(prev)
    return {b: {'median': 1e3 * statistics.median(v), 'min': 1e3 * min(v), 'max': 1e3 * max(v)} for b, v in times.items()}


def count_launches(m1, fn):
    """kernels on the device during one ``fn()`` under each backend, from the profiler's device records (memory copies and memsets
    are not kernels and are listed beside them)"""
    from torch.profiler import ProfilerActivity, profile
    prev = m1.get_encoder_backend()
    res = {}
    try:
        for b in BACKENDS:
            m1.set_encoder_backend(b)
            fn()
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            dev = [e for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA')]
            other = [e for e in dev if e.name.lower().startswith(('memcpy', 'memset'))]
            names = {}
            for e in dev:
                if e not in other:
                    names[e.name] = names.get(e.name, 0) + 1
            res[b] = {'kernels': sum(names.values()), 'copies_and_memsets': len(other), 'by_name': names}
    finally:
        m1.set_encoder_backend(prev)
    return res


def parity(dev):
    import copy
    import encoder_reference as er
    from animateportrait_amd import encoder_hip
    from test_seq_encoder_cpu import SHAPES, make_encoder, make_x
    enc = make_encoder()
    de = copy.deepcopy(enc).to(dev).eval()
    params = er.params_of(enc)
    rows = []
    for b, t in SHAPES:
        x = make_x(b, t)
        ref = er.encoder_forward(x.numpy(), params)
        with torch.no_grad():
            lib = de(x.to(dev))
            hip = encoder_hip.encoder_forward(de, x.to(dev))
        rows.append({'B': b, 'T': t, 'd_ff': 2048, 'linf_hip_vs_float64': float(np.abs(hip.cpu().double().numpy() - ref).max()),
                     'linf_library_vs_float64': float(np.abs(lib.cpu().double().numpy() - ref).max()),
                     'max_abs_reference': float(np.abs(ref).max())})
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--rounds', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--frames', type=int, default=625)
    ap.add_argument('--out', default=None, help='write the result as JSON here as well')
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('bench_module1_encoder: no GPU')
    dev = torch.device('cuda:0')
    from animateportrait_amd import audio, module1 as m1
    from bench_module1 import Timed, stage_once
    from test_seq_encoder_cpu import make_encoder, make_x
    assert m1.get_encoder_backend() == 'library'
    res = {'device': torch.cuda.get_device_name(0), 'rounds': a.rounds, 'warmup': a.warmup,
           'unit': 'ms (median over the rounds; min and max beside it), host clock around a synchronised call'}
    enc = make_encoder().to(dev).eval()
    res['encoder_alone'] = {}
    with torch.no_grad():
        for t in (512, 113):
            x = make_x(1, t).to(dev)
            res['encoder_alone']['T=%d' % t] = alternate(m1, lambda: enc(x), a.rounds, a.warmup)
        x512 = make_x(1, 512).to(dev)
        try:
            res['encoder_launches_T512'] = count_launches(m1, lambda: enc(x512))
        except Exception as e:          # (a box without the profiler's tracer: say so instead of estimating)
            res['encoder_launches_T512'] = {'not_counted': '%s: %s' % (type(e).__name__, e)}
        torch.manual_seed(1234)
        content = Timed(m1.Audio2LandmarkContent(use_prior_net=True, drop_out=0.5).to(dev).eval())
        pose = Timed(m1.Audio2LandmarkPos(drop_out=0.5).to(dev).eval())
        au512 = torch.randn(512, 18, 80, device=dev)
        emb, fid512, z = torch.randn(512, 256, device=dev), torch.randn(512, 204, device=dev) * 0.1, torch.zeros(512, 128, device=dev)
        res['pose_network_512_windows'] = alternate(m1, lambda: pose.net(au512, emb, fid512, None, z), a.rounds, a.warmup)
    spk = torch.randn(256, generator=torch.Generator().manual_seed(7))
    fid = torch.randn(204, generator=torch.Generator().manual_seed(8)) * 0.1
    au = audio.clip_audio_features(os.path.join(ROOT, 'tests', 'golden', 'female12.wav'), max_frames=a.frames)
    assert au.shape == (a.frames, 18, 80), au.shape
    res['windows'], res['segments'] = a.frames, [min(512, a.frames - j) for j in range(0, a.frames, 512)]
    res['lstm_backend'], res['post_backend'] = m1.get_lstm_backend(), m1.get_post_backend()
    times, fls = {b: [] for b in BACKENDS}, {}
    try:
        for r in range(a.warmup + a.rounds):
            for b in (BACKENDS if r % 2 == 0 else BACKENDS[::-1]):
                m1.set_encoder_backend(b)
                fls[b], t = stage_once(m1, pose, content, au, spk, fid)
                if r >= a.warmup:
                    times[b].append(t)
    finally:
        m1.set_encoder_backend('library')
    res['stage'] = {b: {k: {'median': 1e3 * statistics.median(t[k] for t in times[b]), 'min': 1e3 * min(t[k] for t in times[b]),
                            'max': 1e3 * max(t[k] for t in times[b])} for k in times[b][0]} for b in BACKENDS}
    res['landmarks_linf_hip_vs_library'] = float(np.abs(np.asarray(fls['hip']) - np.asarray(fls['library'])).max())
    res['landmarks_range'] = float(np.abs(np.asarray(fls['library'])).max())
    res['parity'] = parity(dev)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
