#!/usr/bin/env python3
"""Time of the static cartoon generator (networks.Photo2CartoonGenerator, ngf 32, 256 x 256) at B = 1 and B = 16, and, in the
same process on the same device, of the test-side restatement (tests/photo2cartoon_reference.py) evaluated in float32 through
PyTorch-ROCm's own operators.  The static cartoon runs once per distinct photo, so this is a finding, not a gate.

Each batch size is one child process under its own time limit; the script stops at the first one that fails.  Per child: both
paths are warmed up (code objects loaded, weights packed, MIOpen's algorithms picked), then timed in alternation -- REPEATS
rounds of ITERS forwards each between device events -- and the median round and the spread are reported, with the L-inf
difference of the two outputs.

    python tools/bench_cartoon_static.py [--out profiles/r12_cartoon_static.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES, NGF, SIZE, WARMUP, REPEATS, ITERS, LIMIT_S = (1, 16), 32, 256, 3, 7, 5, 240


def child(batch):
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import photo2cartoon_reference as pr
    from animateportrait_amd import networks, style_ops
    dev = torch.device('cuda:0')
    sd = pr.init_params(pr.param_shapes(NGF), 2468)
    G = networks.Photo2CartoonGenerator(ngf=NGF).to(dev)
    G.load_state_dict(sd, strict=True)
    sd_dev = {k: v.to(dev) for k, v in sd.items()}
    x = style_ops.quantize_u8(torch.rand(batch, 3, SIZE, SIZE, generator=torch.Generator().manual_seed(5)) * 2 - 1).to(dev)

    def ours():
        return G(x)

    def stock():
        return pr.generator_forward(sd_dev, x, torch.float32, dev)

    for fn in (ours, stock):
        for _ in range(WARMUP):
            y = fn()
    torch.cuda.synchronize()
    diff = float((ours() - stock()).abs().max())
    times = {'ours': [], 'stock': []}
    for _ in range(REPEATS):
        for tag, fn in (('ours', ours), ('stock', stock)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(ITERS):
                y = fn()
            e1.record()
            e1.synchronize()
            times[tag].append(e0.elapsed_time(e1) / ITERS)
    del y
    out = {'batch': batch}
    for tag, t in times.items():
        t = sorted(t)
        out[tag + '_ms'] = round(t[len(t) // 2], 3)
        out[tag + '_ms_min_max'] = [round(t[0], 3), round(t[-1], 3)]
    out['linf_ours_vs_stock_fp32'] = diff
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', type=int, default=None)
    a = ap.parse_args()
    if a.child is not None:
        child(a.child)
        return 0
    rows = []
    for b in BATCHES:
        # a fresh process per step, under its own limit; the first failure ends the run
        r = subprocess.run(['timeout', '-k', '10', str(LIMIT_S), sys.executable, os.path.abspath(__file__), '--child', str(b)],
                           stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            print('B = %d failed with status %d; stopping' % (b, r.returncode), file=sys.stderr)
            return r.returncode
        rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(rows[-1])
    result = {'workload': 'Photo2CartoonGenerator ngf %d, %d x %d, forward' % (NGF, SIZE, SIZE), 'warmup': WARMUP, 'repeats': REPEATS,
              'iters_per_repeat': ITERS, 'rows': rows}
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(result, f, indent=1)
            f.write('\n')
    print(json.dumps(result))
    return 0


if __name__ == '__main__':
    sys.exit(main())
