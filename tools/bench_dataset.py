#!/usr/bin/env python3
"""What one batch of the umlvd_ifw dataset costs beside the train step it feeds: prints ONE JSON line for B = 16 on a generated
tree (tests/dataset_fixture.py: small sources, 300x280 photos and 100x120 clip frames, so decoding is cheaper than on the
real 512x512 tree; the transforms always produce 286 -> 256 crops, so their cost is representative).

    python tools/bench_dataset.py [--batch 16] [--reps 5] [--no_train_step]

decode_ms: PIL decode of every file of the batch (thread pool, nothing cached); prep_device_ms / prep_host_ms: the image
transforms of the batch from the decoded arrays (uploads and launches, or PIL spread over the same pool of ``host_threads``
threads), same run, same plans; prep_host_1thread_ms: PIL on the calling thread alone; rest_of_batch_ms: discs, motion grids,
static warps and host bookkeeping -- NOT timed by itself but batch_device_ms - prep_device_ms - decode_ms; train_step_ms: optimize_parameters() of geomgm_ifw_fore at ngf = ndf = 64 in plain bf16."""
import argparse
import json
import os
import random
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def timed(fn, reps):
    ts = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts[1:])          # the first call warms caches, tables and the pool


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--no_train_step', action='store_true')
    args = ap.parse_args()
    import dataset_fixture as fx
    from animateportrait_amd.data import create_dataset
    from animateportrait_amd.models import create_model
    from animateportrait_amd.options.base_options import TrainOptions
    work = tempfile.mkdtemp()
    fx.write_tree(os.path.join(work, 'tree'), os.path.join(work, 'lists'))
    argv = ['--model', 'geomgm_ifw_fore', '--netG', 'resnet_9blocks_rcatland32_full_ifw', '--dataset_mode', 'umlvd_ifw',
            '--dataroot', fx.NAME, '--list_dir', os.path.join(work, 'lists'), '--output_nc', '1', '--ngf', '64', '--ndf', '64',
            '--netg_resb_div', '3', '--netg_resb_disp', '3', '--batch_size', str(args.batch), '--gpu_ids', '0',
            '--num_threads', '16', '--precision', 'bf16']
    opt = TrainOptions().parse(argv)
    torch.cuda.set_device(0)
    ds = create_dataset(opt)
    random.seed(1)
    torch.manual_seed(1)
    plans = [ds.plan_sample(i % len(ds)) for i in range(args.batch)]
    jobs = ds._jobs(plans)
    decoded = ds.decode(jobs)
    out = {'batch': args.batch, 'images_per_batch': len(jobs), 'load_size': opt.load_size, 'crop_size': opt.crop_size,
           'decode_ms': round(timed(lambda: ds.decode(jobs), args.reps), 3),
           'prep_device_ms': round(timed(lambda: ds.image_tensors(plans, 'device', decoded), args.reps), 3),
           'prep_host_ms': round(timed(lambda: ds.image_tensors(plans, 'host', decoded), max(1, args.reps // 2)), 3),
           'batch_device_ms': round(timed(lambda: ds.make_batch(plans, 'device'), args.reps), 3)}
    out['rest_of_batch_ms'] = round(max(0.0, out['batch_device_ms'] - out['prep_device_ms'] - out['decode_ms']), 3)
    out['host_threads'] = ds.pool()._max_workers
    ds.pool = lambda: None                     # the host leg again, on the calling thread alone
    out['prep_host_1thread_ms'] = round(timed(lambda: ds.image_tensors(plans, 'host', decoded), 1), 3)
    del ds.pool
    if not args.no_train_step:
        from animateportrait_amd import networks as N, standins
        dev = torch.device('cuda:0')
        model = create_model(opt)
        model.aux['landmarks'] = standins.StandinLandmarkNet().to(dev)
        model.aux['faceloss'] = N.FaceLoss(standins.StandinFaceNet().to(dev))
        model.aux['netF'] = standins.StandinFlowNet().to(dev)
        model.aux['modnet'] = standins.StandinMatteNet().to(dev)
        batch = ds.make_batch(plans, 'device')

        def step():
            model.set_input(batch)
            model.optimize_parameters()
        step()
        out['train_step_ms'] = round(timed(step, args.reps), 3)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
