#!/usr/bin/env python3
"""What one batch of the umlvdfw_test dataset and of test.py's PNG sink costs: prints ONE JSON line for B = 16 on the
generated tree (tests/testset_fixture.py: three 300x280-class photos, repeated to fill the batch; --draw_op 1, load 286 ->
crop 256).

    python tools/bench_test_dataset.py [--batch 16] [--batches 5] [--out profiles/<round>_test_dataset.json]

batch_device_ms / batch_host_ms: plan_item + make_batch per batch with --data_prep device / host (decode included, nothing
cached; wall clock around a device synchronisation, median over --batches after one warm-up batch);
landmark_map_ms: one apd_landmark_map call on the 2B landmark sets with the 64-segment table, from device events (median
of 20 after a warm-up); landmark_map_op0_ms: the same call drawing discs only;
png_sink_ms: visuals.save_png_batch of nine (B, C, 256, 256) visuals per batch -- the launches, the synchronisation and the
PNG encoding on the pool -- into a temporary directory; frames_to_u8_ms: the nine launches and the synchronisation alone.
Not measured: 512-pixel sources, disk speed (the tree sits in the temporary directory), the reference's own item.

    python tools/bench_test_dataset.py --png_sink [--out profiles/<round>_png_sink.json]

prints ONE JSON line about the two PNG encoders instead (--png_encoder host | device), in one process on the same visuals:
sink_host_ms / sink_device_ms: visuals.save_png_batch of that batch with each encoder (wall clock, median after a warm-up);
png_encode_ms: the nine apd_png_encode calls alone, from device events; sink_*_bytes: what the 144 files weigh;
clip_host_ms / clip_device_ms: end2end.write_frames of a 625-frame clip of 1 x 256 x 256 line drawings (the fixture's
drawing, shifted per frame) with each encoder, once each after a 32-frame warm-up; clip_*_bytes: the 625 files."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def wall(fn, reps):
    ts = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts[1:]), 3)          # the first call warms caches, tables and the pools


def events(fn, reps=20):
    fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return round(statistics.median(ts), 4)


def dir_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def png_sink(args, work, shown, labels):
    """both encoders on the same visuals, then on a 625-frame clip"""
    import png_fixture as pf
    from animateportrait_amd import end2end
    from animateportrait_amd.data import visuals
    dev = next(iter(shown.values())).device
    out = {'batch': args.batch, 'batches': args.batches, 'pngs_per_batch': len(labels) * args.batch, 'png_threads': visuals.PNG_THREADS}
    for enc in ('host', 'device'):
        d = os.path.join(work, 'sink_' + enc)
        os.makedirs(d)
        names = {l: [os.path.join(d, '%d_%s.png' % (i, l)) for i in range(args.batch)] for l in labels}
        out['sink_%s_ms' % enc] = wall(lambda: visuals.save_png_batch(shown, names, encoder=enc), args.batches)
        out['sink_%s_bytes' % enc] = dir_bytes(d)
    out['png_encode_ms'] = events(lambda: [visuals.encode_png_batch(t, slot=l) for l, t in shown.items()])
    out['frames_to_u8_ms'] = events(lambda: [visuals.frames_to_u8(t, slot=l) for l, t in shown.items()])
    base = torch.from_numpy(pf.to_frames(pf.line_drawing()[:, :, :1])).to(dev)               # (1, 1, 256, 256)
    clip = torch.cat([torch.roll(base, (k % 41, k % 59), (2, 3)) for k in range(625)])
    out['clip_frames'], out['clip_batch'] = 625, args.batch
    for enc in ('host', 'device'):
        d = os.path.join(work, 'clip_' + enc)
        os.makedirs(d)
        end2end.write_frames(clip[:32], d, enc, args.batch)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        end2end.write_frames(clip, d, enc, args.batch)
        out['clip_%s_ms' % enc] = round((time.perf_counter() - t0) * 1e3, 1)
        out['clip_%s_bytes' % enc] = dir_bytes(d)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--batches', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--png_sink', action='store_true', help='measure the two PNG encoders instead of the dataset')
    args = ap.parse_args()
    import testset_fixture as tf
    from animateportrait_amd.data import find_dataset_using_name, visuals
    work = tempfile.mkdtemp()
    tf.write_test_tree(os.path.join(work, 'tree'), os.path.join(work, 'lists'))
    torch.cuda.set_device(0)
    dev = torch.device('cuda:0')
    ds = find_dataset_using_name('umlvdfw_test')(tf.options(os.path.join(work, 'lists'), draw_op=1, batch_size=args.batch, num_threads=16))

    def batch(mode):
        return ds.make_batch([ds.plan_item(i % len(ds)) for i in range(args.batch)], mode)
    out = {} if args.png_sink else {'batch': args.batch, 'batches': args.batches, 'draw_op': 1, 'load_size': 286, 'crop_size': 256, 'photos': [list(p) for p in tf.fx.PHOTOS],
           'batch_device_ms': wall(lambda: batch('device'), args.batches),
           'batch_host_ms': wall(lambda: batch('host'), args.batches),
           'host_threads': ds._images.pool()._max_workers}
    item = batch('device')
    lms = torch.cat([item['A_lm_68'], item['tB_lm_68']]).contiguous()
    if not args.png_sink:
        out['landmark_map_ms'] = events(lambda: visuals.landmark_map(lms, ds.segments, 256, 256, 3, 2, op=1))
        out['landmark_map_op0_ms'] = events(lambda: visuals.landmark_map(lms, ds.segments, 256, 256, 3, 2, op=0))
    g = torch.Generator().manual_seed(0)
    labels = ['real_A', 'real_A_lm', 'target_B_lm', 'fake_B', 'fake_B_vis', 'fg_mask', 'fakeB_static', 'fake_B_fore', 'fg_mask1']
    shown = {l: (torch.rand((args.batch, 3 if i % 2 else 1, 256, 256), generator=g) * 2 - 1).to(dev) for i, l in enumerate(labels)}
    shown['real_A'], shown['real_A_lm'] = item['A'], item['A_lm']
    if args.png_sink:
        out = png_sink(args, work, shown, labels)
    else:
        names = {l: [os.path.join(work, 'png', '%d_%s.png' % (i, l)) for i in range(args.batch)] for l in labels}
        os.makedirs(os.path.join(work, 'png'))
        out['png_sink_ms'] = wall(lambda: visuals.save_png_batch(shown, names), args.batches)
        out['frames_to_u8_ms'] = wall(lambda: [visuals.frames_to_u8(t, slot=l) for l, t in shown.items()], args.batches)
        out['png_threads'] = visuals.PNG_THREADS
        out['pngs_per_batch'] = len(labels) * args.batch
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
