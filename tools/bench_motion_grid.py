#!/usr/bin/env python3
"""The motion-grid stage of a streamed clip with the Delaunay triangulation on the host (scipy per frame) and on the device
(ap_delaunay): ClipStreamer.run(profile=True) on a 625-frame synthetic landmark sequence (float landmarks jittered around a
fixed face) at batch 16, full-width generator, stand-in weights.  Both modes run in this process, alternating, after one
warm-up clip each; the medians of the repeats are reported, with the spread.  ap_delaunay's own time per batch of 16 point
sets is taken from device events around a train of launches.  Prints one JSON line.
Usage: python tools/bench_motion_grid.py [--frames 625] [--batch 16] [--repeats 3] [--ngf 64]"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def synthetic_clip(frames, seed=5):
    """a fixed face (68 float landmarks inside the photo) and a sequence that sways and jitters around it"""
    from animateportrait_amd.synthetic import make_landmarks
    lm0 = make_landmarks(1, torch.Generator().manual_seed(seed))[0].float()
    rng = np.random.default_rng(seed)
    t = torch.arange(frames).view(frames, 1, 1).float()
    seq = lm0.unsqueeze(0) + 3.0 * torch.sin(0.11 * t + lm0.unsqueeze(0) / 40.0) + torch.from_numpy(
        rng.uniform(-0.5, 0.5, (frames, 68, 2)).astype(np.float32))
    return lm0, seq.clamp(2.0, 253.0).contiguous()


def kernel_ms(pts, launches=200):
    """ap_delaunay on one batch through the C ABI: device events around `launches` back-to-back launches"""
    import ctypes
    from animateportrait_amd import _capi as C
    n, p = pts.shape[:2]
    tri = torch.empty((n, 2 * p, 3), dtype=torch.int32, device=pts.device)
    count = torch.empty((n,), dtype=torch.int32, device=pts.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(pts.device).cuda_stream)

    def launch():
        C.check(C.lib().ap_delaunay(ctypes.c_void_p(pts.data_ptr()), n, p, 2 * p, ctypes.c_void_p(tri.data_ptr()),
                                    ctypes.c_void_p(count.data_ptr()), stream), 'delaunay')
    for _ in range(10):
        launch()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        launch()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--frames', type=int, default=625)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--ngf', type=int, default=64)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_motion_grid: needs the GPU; there is nothing to measure without one')
    from animateportrait_amd import standins, stream
    from animateportrait_amd.data import motion
    from animateportrait_amd.options.base_options import TestOptions
    from animateportrait_amd.models import create_model
    dev = torch.device('cuda:0')
    opt = TestOptions().parse(['--model', 'geomcgt_ifw_test', '--netG', 'resnet_9blocks_rcatland32_full_ifw',
                               '--dataset_mode', 'synthetic', '--name', 'motion_grid_bench', '--output_nc', '1', '--ngf', str(a.ngf),
                               '--netg_resb_div', '3', '--netg_resb_disp', '3', '--gpu_ids', '0'])
    with contextlib.redirect_stdout(io.StringIO()):
        model = create_model(opt)
    model.aux['netF'] = standins.StandinFlowNet().to(dev)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, 256), torch.linspace(-1, 1, 256), indexing='ij')
    photo = torch.stack([torch.sin(3 * xx + yy), torch.cos(2 * yy - xx), xx * yy], 0).unsqueeze(0).contiguous()
    matte = (((yy / 0.8) ** 2 + (xx / 0.6) ** 2) < 1).float().view(1, 1, 256, 256) * 0.9
    lm0, seq = synthetic_clip(a.frames)
    modes = ('host', 'device')
    streamers = {m: stream.ClipStreamer(model, batch=a.batch, triangulate=m) for m in modes}
    runs = {m: [] for m in modes}
    out = {}
    for rep in range(a.repeats + 1):                       # repeat 0 warms every shape of both modes up and is dropped
        for m in modes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            frames = streamers[m].run(photo, lm0, seq, matte=matte, profile=True)
            torch.cuda.synchronize()
            total = time.perf_counter() - t0
            if rep:
                runs[m].append(dict(streamers[m].timing, clip=total))
            else:
                out[m] = frames
    err = float((out['host'] - out['device']).abs().max())
    # one batch of the clip's point sets (destination landmarks + border points, as cal_motion256 builds them)
    edges = torch.tensor(motion.EDGES, dtype=torch.float32).unsqueeze(0).expand(a.batch, -1, -1)
    pts = torch.cat([seq[:a.batch].flip(-1), edges], 1).contiguous().to(dev)
    _, count = motion.triangulate_device(pts)
    res = {'tool': 'bench_motion_grid', 'frames': a.frames, 'batch': a.batch, 'ngf': a.ngf, 'repeats': a.repeats,
           'device_name': torch.cuda.get_device_name(0),
           'triangles_per_set': sorted(set(count.tolist())),
           'delaunay_kernel_ms_per_batch': round(kernel_ms(pts), 4),
           'frames_linf_host_vs_device': err}
    for m in modes:
        for key in ('motion_grid', 'landmark_maps', 'set_input_netF', 'generator', 'clip'):
            vals = [r[key] for r in runs[m]]
            res['%s_%s_s' % (m, key)] = round(statistics.median(vals), 5)
            if key in ('motion_grid', 'clip'):
                res['%s_%s_s_min_max' % (m, key)] = [round(min(vals), 5), round(max(vals), 5)]
    motion.check_triangulations(dev)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
