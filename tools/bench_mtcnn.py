#!/usr/bin/env python3
"""Milliseconds per image of the device MTCNN detector (animateportrait_amd.mtcnn, libapface.so), for 1 image and a batch of
16, at 320 x 106 (the source resized with PIL BILINEAR) and at the full source photo; and, in the same run, of a stock
PyTorch-ROCm fp32 rendering of the same three nets on the same levels and the same number of cut-outs (the nets alone:
no resampling, no box arithmetic -- the floor a framework-only detector would have to add those to).

    python tools/bench_mtcnn.py --photo /path/to/wflw.png --weights MTCNN/weights [--rounds 7] [--out profiles/mtcnn_bench.json]

Medians of alternated rounds (device, torch, device, ...), each round timed with events around the whole batch after one
untimed warm-up round.  A detection includes its read-back."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as Fn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from animateportrait_amd import mtcnn  # noqa: E402


class TorchNets:
    """the three nets in stock PyTorch, fp32, from the same weight files"""

    def __init__(self, weights, device):
        raw = mtcnn._read_raw(weights)
        self.p = {net: {k: torch.from_numpy(v).to(device) for k, v in d.items()} for net, d in raw.items()}

    def _stack(self, net, x, spec):
        p = self.p[net]
        for kind, arg in spec:
            if kind == 'conv':
                x = Fn.prelu(Fn.conv2d(x, p['features.%s.weight' % arg], p['features.%s.bias' % arg]),
                             p['features.prelu%s.weight' % arg[-1]])
            else:
                x = Fn.max_pool2d(x, arg, 2, ceil_mode=True)
        return x

    def pnet(self, level_u8):
        x = ((level_u8.float() - 127.5) * 0.0078125).permute(2, 0, 1)[None]
        x = self._stack('pnet', x, [('conv', 'conv1'), ('pool', 2), ('conv', 'conv2'), ('conv', 'conv3')])
        p = self.p['pnet']
        return Fn.softmax(Fn.conv2d(x, p['conv4_1.weight'], p['conv4_1.bias']), 1), Fn.conv2d(x, p['conv4_2.weight'], p['conv4_2.bias'])

    def tail(self, net, cuts_u8):
        x = ((cuts_u8.float() - 127.5) * 0.0078125).permute(0, 3, 1, 2)
        p = self.p[net]
        if net == 'rnet':
            x = self._stack(net, x, [('conv', 'conv1'), ('pool', 3), ('conv', 'conv2'), ('pool', 3), ('conv', 'conv3')])
            fc, heads = 'conv4', ('conv5_1', 'conv5_2')
        else:
            x = self._stack(net, x, [('conv', 'conv1'), ('pool', 3), ('conv', 'conv2'), ('pool', 3), ('conv', 'conv3'), ('pool', 2),
                                     ('conv', 'conv4')])
            fc, heads = 'conv5', ('conv6_1', 'conv6_2', 'conv6_3')
        x = x.transpose(3, 2).reshape(x.shape[0], -1)
        x = Fn.prelu(Fn.linear(x, p['features.%s.weight' % fc], p['features.%s.bias' % fc]), p['features.prelu%s.weight' % fc[-1]])
        outs = [Fn.linear(x, p[h + '.weight'], p[h + '.bias']) for h in heads]
        outs[0] = Fn.softmax(outs[0], 1)
        return outs


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--photo', required=True, help='the source photo (the reference tree\'s wflw.png, 2979 x 996)')
    ap.add_argument('--weights', default=mtcnn.DEFAULT_WEIGHTS)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    from PIL import Image
    dev = torch.device('cuda')
    full = Image.open(a.photo).convert('RGB')
    images = {'320x106': np.asarray(full.resize((320, 106), Image.BILINEAR)), '%dx%d' % full.size: np.asarray(full)}
    det = mtcnn.Detector(a.weights)
    nets = TorchNets(a.weights, dev)
    result = {'rounds': a.rounds, 'cases': {}}
    for label, image in images.items():
        img = torch.from_numpy(np.ascontiguousarray(image)).to(dev)
        H, W = image.shape[:2]
        # what the torch nets are fed: the levels, and as many cut-outs as the device detector's stages really see
        job = det._enqueue(img)
        torch.cuda.synchronize()
        if int(job.status):
            raise SystemExit('%s: a stage overflowed its capacity (status %d)' % (label, int(job.status)))
        faces = int(job.n)
        levels = [det.resize_level(img, lh, lw) for _, lh, lw in mtcnn.pyramid(W, H)]
        n_r, n_o = int(job.n_rnet), int(job.n_onet)
        cuts_r = torch.randint(0, 256, (max(n_r, 1), 24, 24, 3), dtype=torch.uint8, device=dev)
        cuts_o = torch.randint(0, 256, (max(n_o, 1), 48, 48, 3), dtype=torch.uint8, device=dev)

        def torch_nets(batch):
            with torch.no_grad():
                for _ in range(batch):
                    for lvl in levels:
                        nets.pnet(lvl)
                    nets.tail('rnet', cuts_r)
                    nets.tail('onet', cuts_o)

        for batch in (1, 16):
            runs = {'device': lambda: det.detect_batch([img] * batch), 'torch_nets': lambda: torch_nets(batch)}
            times = {k: [] for k in runs}
            for k, fn in runs.items():
                fn()                                     # warm-up, untimed
            torch.cuda.synchronize()
            for _ in range(a.rounds):
                for k, fn in runs.items():               # alternated
                    times[k].append(timed(fn) / batch)
            case = {k: round(statistics.median(v), 3) for k, v in times.items()}
            case.update(faces=faces, rnet_boxes=n_r, onet_boxes=n_o, levels=len(levels))
            result['cases']['%s batch %d' % (label, batch)] = case
            print('%-22s device %8.3f ms/image   torch nets alone %8.3f ms/image   (%d faces, %d / %d boxes to R-Net / O-Net)'
                  % ('%s x%d' % (label, batch), case['device'], case['torch_nets'], faces, n_r, n_o))
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
