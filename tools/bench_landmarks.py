"""What the photo's 68 landmarks cost on the device (landmarks.py, fan.py, csrc/face/face_fan.hip), at the full architecture
FAN(num_modules=4, width=256, depth=4) with SEEDED weights (the published checkpoint is not part of this repository) on a seeded
512 x 512 picture with a given face box.

Two legs of one detection (picture on the device -> (68, 3) on the host: the crop in both orientations, the forward at B = 2,
the decode) in ONE process, in alternated rounds, medians reported (as tools/bench_speaker.py does):
  device_hip      landmarks.PhotoLandmarks: apf_fan_crop, fan.FAN through ops.conv2d / style_ops, apf_fan_decode
  stock_pytorch   the same crop and decode kernels around the SAME network through stock PyTorch-ROCm operators
                  (tests/fan_reference.py fan_forward in fp32 on the device: F.batch_norm, F.conv2d, ...)
Then the two new kernels alone, back to back between two events.  Also recorded: the L-inf error of the device forward and of the
plain fp32 PyTorch statement against float64 at the architecture of tests/test_fan_gpu.py, FAN(2, 32) on 2 x 128 x 128, and the
test's bar (4 times the latter).

    python tools/bench_landmarks.py --out profiles/photo_landmarks.json

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
        raise SystemExit('bench_landmarks: no GPU')
    from animateportrait_amd import fan, landmarks
    import fan_reference as R
    from test_fan_gpu import network_case, device_fan
    dev = torch.device('cuda:0')
    sd = fan.seeded_state_dict(4, 256, 4, seed=1)
    net = device_fan(sd, 4, 256)
    det = landmarks.PhotoLandmarks(net, dev)
    img = torch.from_numpy(np.random.RandomState(1).randint(0, 256, (512, 512, 3)).astype(np.uint8)).to(dev)
    box = (120.0, 110.0, 400.0, 420.0)
    sd_dev = {k: v.to(dev) for k, v in sd.items()}

    def stock():
        with torch.no_grad():
            maps = R.fan_forward(sd_dev, landmarks.fan_crop(img, box, 256, 'bgr', True), 4).contiguous()
        out = np.zeros((68, 3), np.float32)
        out[:, :2] = landmarks.fan_decode(maps[:1], [box], maps[1:2], True)[0].cpu().numpy()
        return out
    legs = {'device_hip': lambda: det.detect(img, box), 'stock_pytorch': stock}
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
    res = {'device': torch.cuda.get_device_name(0), 'architecture': 'FAN(num_modules=4, width=256, depth=4), crop 256, B = 2 (flip_input)',
           'weights': 'seeded (fan.seeded_state_dict, seed 1); the published checkpoint is not part of this repository',
           'picture': 'seeded noise, 512 x 512, box %s' % (box,), 'rounds': a.rounds, 'warmup': a.warmup,
           'unit': 'ms per detection (median over the rounds; min and max beside it)',
           'fallback_layers': [c.name for c in net.convs() if not all(c._served.values())]}
    for n in names:
        res[n] = {'median': 1e3 * statistics.median(times[n]), 'min': 1e3 * min(times[n]), 'max': 1e3 * max(times[n])}
    res['landmarks_differ_between_the_legs'] = int((outs['device_hip'] != outs['stock_pytorch']).any(1).sum())

    # the two new kernels alone
    maps = torch.randn(2, 68, 64, 64, device=dev)
    single = {}
    for name, fn in {'apf_fan_crop_512_to_2x3x256x256': lambda: landmarks.fan_crop(img, box, 256, 'bgr', True),
                     'apf_fan_decode_68x64x64_flip': lambda: landmarks.fan_decode(maps[:1], [box], maps[1:2], True)}.items():
        per = []
        for r in range(a.warmup + a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.kernel_launches):
                fn()
            e1.record()
            e1.synchronize()
            if r >= a.warmup:
                per.append(e0.elapsed_time(e1) / a.kernel_launches)
        single[name] = {'median': statistics.median(per), 'min': min(per), 'max': max(per)}
    res['kernels_alone'] = dict(single, unit='ms per call (output allocation included), back to back (%d calls between two events)'
                                % a.kernel_launches)

    # accuracy at the test's architecture
    tsd, x, ref, plain_err = network_case(2, 32, 3)
    got = device_fan(tsd, 2, 32)(x.to(dev)).cpu()
    res['linf_vs_float64_FAN_2_32_on_2x128x128'] = {'device_hip': float((got.double() - ref).abs().max()),
                                                    'plain_fp32_pytorch_statement': plain_err, 'largest_map_value': float(ref.abs().max())}
    res['linf_bar'] = 4 * plain_err
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
