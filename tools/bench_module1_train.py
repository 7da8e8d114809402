"""What one training step of Module1's content branch costs with each LSTM backend (module1.set_lstm_train_backend), and what
the two training kernels of libapseq.so cost per layer.

One ContentTrainer step (module1_train.py: forward, loss, backward, Adam) on a segment of B = 512 windows of T = 18 frames,
the network at the trainer's defaults with seeded weights, is timed with the 'library' and the 'hip' backend in ONE process, in
alternated rounds, a device synchronise on both sides; medians over the rounds are reported.  Then the kernels alone, per layer
input width I in {80, 256}: one apq_lstm_layer_fwd_train and one apq_lstm_layer_bwd launch between device events, next to the
forward + backward of a one-layer nn.LSTM of the same shape.

    python tools/bench_module1_train.py --out profiles/module1_train.json [--errors LOG]

``--errors`` takes the output of ``pytest tests/test_seq_lstm_train_gpu.py -m gpu -s`` and files its ``ERR`` lines (the measured
error of the kernel route and of the library's own fp32 backward against float64) in the result.
Needs a GPU: there is no CPU mode, a time taken without the device would say nothing."""
import argparse
import json
import os
import re
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

B, T, H = 512, 18, 256


def _events(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def kernel_times(dev, reps):
    from animateportrait_amd import _seqapi as Q, ops
    rows = []
    for i in (80, 256):
        torch.manual_seed(i)
        lstm = torch.nn.LSTM(i, H, 1, batch_first=True).to(dev).train()
        x = torch.randn(B, T, i, device=dev)
        dout = torch.randn(B, T, H, device=dev)
        out, gates, cell, dg = (torch.empty(B, T, n, device=dev) for n in (H, 4 * H, H, 4 * H))
        w = [getattr(lstm, n + '_l0').contiguous() for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')]
        w_hh_t = w[1].t().contiguous()
        fa = [ops._ptr(a) for a in [x] + w + [out, gates, cell]]
        ba = [ops._ptr(a) for a in (dout, gates, cell, w_hh_t, dg)]
        xg = x.clone().requires_grad_(True)

        def fwd():
            Q.check(Q.lib().apq_lstm_layer_fwd_train(*fa, B, T, i, H, ops._stream()), 'lstm_layer_fwd_train')

        def bwd():
            Q.check(Q.lib().apq_lstm_layer_bwd(*ba, B, T, H, 0, ops._stream()), 'lstm_layer_bwd')

        def library():
            lstm.zero_grad(set_to_none=True)
            xg.grad = None
            (lstm(xg)[0] * dout).sum().backward()

        rows.append({'B': B, 'T': T, 'I': i, 'H': H, 'fwd_train_ms': _events(fwd, reps), 'bwd_ms': _events(bwd, reps),
                     'library_fwd_bwd_ms': _events(library, reps),
                     # 2 x 4H x H multiply-adds per row and step in dh_rec
                     'bwd_tflops': None})
        rows[-1]['bwd_tflops'] = 2.0 * 4 * H * H * B * (T - 1) / (rows[-1]['bwd_ms'] * 1e-3) / 1e12
    return rows


def parse_errors(path):
    rows = []
    for ln in open(path):                                    # (under -s a test's first line stands behind pytest's progress dot)
        m = re.search(r'\bERR (\S+) (\S+) kernel=(\S+) library=(\S+) range=(\S+)', ln)
        if m:
            rows.append({'case': m.group(1), 'tensor': m.group(2), 'kernel_linf': float(m.group(3)), 'library_linf': float(m.group(4)),
                         'range': float(m.group(5))})
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--rounds', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--kernel_reps', type=int, default=20)
    ap.add_argument('--errors', default=None)
    ap.add_argument('--out', default=None, help='write the result as JSON here as well')
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('bench_module1_train: no GPU')
    dev = torch.device('cuda:0')
    from animateportrait_amd import module1 as m1, module1_train as mt
    g = torch.Generator().manual_seed(5)
    face = torch.randn(1, 204, generator=g) * 0.3
    walk = torch.cumsum(torch.randn(B + T, 204, generator=g) * 0.02, 0) + face
    fls = torch.stack([walk[k:k + T] for k in range(B)]).to(dev)
    aus, face = torch.randn(B, T, 80, generator=g).to(dev), face.to(dev)
    opt = mt.make_parser().parse_args(['--dump_dir', '', '--ckpt_dir', '', '--nepoch', '1'])
    backends = ('library', 'hip')
    prev = m1.get_lstm_train_backend()
    nets, times, losses = {}, {b: [] for b in backends}, {}
    try:
        for b in backends:                                   # a trainer without a dataset: the step alone is timed
            tr = mt.ContentTrainer.__new__(mt.ContentTrainer)
            torch.manual_seed(9)
            tr.opt, tr.C = opt, m1.Audio2LandmarkContent().to(dev)
            tr.opt_C = torch.optim.Adam(tr.C.parameters(), lr=opt.lr, weight_decay=opt.reg_lr)
            tr.C.train()
            nets[b] = tr
        for r in range(a.warmup + a.rounds):
            for b in (backends if r % 2 == 0 else backends[::-1]):
                m1.set_lstm_train_backend(b)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, loss = nets[b].train_content(fls, aus, face, True)
                torch.cuda.synchronize()
                if r >= a.warmup:
                    times[b].append(time.perf_counter() - t0)
                if r == 0:
                    losses[b] = float(loss)
    finally:
        m1.set_lstm_train_backend(prev)
    res = {'device': torch.cuda.get_device_name(0), 'segment': {'B': B, 'T': T}, 'rounds': a.rounds, 'warmup': a.warmup,
           'unit': 'ms (median over the rounds; min and max beside it)',
           'train_step': {b: {'median': 1e3 * statistics.median(times[b]), 'min': 1e3 * min(times[b]), 'max': 1e3 * max(times[b])}
                          for b in backends},
           'first_step_loss': losses, 'kernel_per_layer': kernel_times(dev, a.kernel_reps)}
    if a.errors:
        res['backward_linf_vs_float64'] = parse_errors(a.errors)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
