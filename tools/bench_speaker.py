"""What the clip's speaker embedding costs (speaker.py, csrc/seq/seq_speaker.hip), for the example clip tests/golden/female12.wav
(13 s, 24 windows of 160 frames), with seeded weights.

Three legs of the embedding stage (the preprocessed 16 kHz signal -> the embedding on the host) in ONE process, in alternated
rounds, medians reported (as tools/bench_f0.py does):
  host_restatement   tests/speaker_reference.py: the float64 numpy statement.  It is NOT resemblyzer (absent from the build
                     image), only the contract the kernels are tested against.
  device_library     speaker.VoiceEncoder('library'): upload, apq_mel_frames, the gather, nn.LSTM, apq_speaker_head, the copy
  device_hip         speaker.VoiceEncoder('hip'): the same with one apq_lstm_layer_fwd launch per layer
Then apq_mel_frames alone at both configurations (400 / 160 / 40 power 2 and 1024 / 256 / 80 power 1 on the clip's samples already
on the device), between two events around a run of launches.  Also recorded: the L-inf error of both device legs and of the plain
fp32 PyTorch statement of the network against float64 (the bar of tests/test_speaker_gpu.py is 4 times the latter).

    python tools/bench_speaker.py --out profiles/speaker_embed.json

Needs a GPU.  No time here is a pass / fail bar."""
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
    ap.add_argument('--kernel_launches', type=int, default=200, help='launches between the two events of a single-kernel timing')
    ap.add_argument('--out', default=None, help='write the result as JSON here as well')
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('bench_speaker: no GPU')
    from animateportrait_amd import audio, speaker
    import speaker_reference as R
    from test_speaker_gpu import plain_fp32_embedding
    dev = torch.device('cuda:0')
    x, sr = audio.read_wav(os.path.join(ROOT, 'tests', 'golden', 'female12.wav'))
    wav = speaker.preprocess_wav(x, sr)
    sd = R.seeded_weights(11)
    encs = {}
    for backend in speaker.LSTM_BACKENDS:
        encs[backend] = speaker.VoiceEncoder(backend)
        encs[backend].load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        encs[backend].to(dev).eval()
    legs = {'host_restatement': lambda: R.embed_utterance(wav, sd)[0],
            'device_library': lambda: encs['library'].embed_utterance(wav)[0].cpu().numpy(),
            'device_hip': lambda: encs['hip'].embed_utterance(wav)[0].cpu().numpy()}
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
    res = {'device': torch.cuda.get_device_name(0), 'clip': 'tests/golden/female12.wav', 'samples': int(len(wav)),
           'windows': int(len(speaker.partial_slices(len(wav))[0])), 'rounds': a.rounds, 'warmup': a.warmup,
           'unit': 'ms (median over the rounds; min and max beside it)',
           'host_leg': 'tests/speaker_reference.py (float64 numpy restatement), not resemblyzer', 'weights': 'seeded, uniform +-1/16'}
    for n in names:
        res[n] = {'median': 1e3 * statistics.median(times[n]), 'min': 1e3 * min(times[n]), 'max': 1e3 * max(times[n])}
    ref = outs['host_restatement']
    res['linf_vs_float64'] = {'device_library': float(np.abs(outs['device_library'] - ref).max()),
                              'device_hip': float(np.abs(outs['device_hip'] - ref).max()),
                              'plain_fp32_pytorch_statement': float(np.abs(plain_fp32_embedding(encs['library'], wav) - ref).max())}
    res['linf_bar'] = 4 * res['linf_vs_float64']['plain_fp32_pytorch_statement']

    # apq_mel_frames alone: events around a run of launches on a warm device, medians over the rounds
    xd = torch.from_numpy(wav).to(dev)
    single = {}
    for name, (n_fft, hop, n_mels, power, fmin, fmax) in {'mel_400_160_40_p2': (400, 160, 40, 2, 0.0, 8000.0),
                                                          'mel_1024_256_80_p1': (1024, 256, 80, 1, 90.0, 7600.0)}.items():
        window = torch.from_numpy(R.hann_periodic(n_fft)).to(dev)
        basis = torch.from_numpy(np.ascontiguousarray(audio.mel_filterbank(16000, n_fft, n_mels, fmin, fmax))).to(dev)
        out = torch.empty(len(wav) // hop + 1, n_mels, device=dev)
        per = []
        for r in range(a.warmup + a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.kernel_launches):
                speaker.mel_frames(xd, window, basis, hop, power, out=out)
            e1.record()
            e1.synchronize()
            if r >= a.warmup:
                per.append(e0.elapsed_time(e1) / a.kernel_launches)
        single[name] = {'frames': int(out.shape[0]), 'median': statistics.median(per), 'min': min(per), 'max': max(per)}
    res['apq_mel_frames_alone'] = dict(single, unit='ms per launch, back to back (%d launches between two events)' % a.kernel_launches)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
