"""What the rigid registration (apq_rigid_register, csrc/seq/seq_register.hip) costs on the example clip's 625 frames, and that
the Module1 stage does not move while the two head-stabilisation switches are off.

1. The device call against the numpy twin.  ``landmark_post.rigid_register`` with both switches (one launch, a synchronise
   behind it) against ``module1.stabilise_head`` on the host INCLUDING the copy back and the upload the twin needs inside a
   device-resident clip; 15 alternated rounds in one process after a warm-up, medians with min and max.  The frames are
   ``register_reference.seeded_frames`` of the standard face (seed 31).  The accuracy figures of tests/test_register_gpu.py are
   measured on the same frames and written beside the times: the spread between the statement's two float64 SVDs, the ``pose``
   bar made of it, and per flag combination the kernel's ``pose`` error and its ``out`` error in float32 ulps.
2. ``module1.predict_landmarks_speaker_aware`` with the switches off (625 windows of tests/golden/female12.wav, seeded
   networks, both post-processing backends) against the same function of another revision: ``--parent_module1 FILE`` names that
   revision's ``animateportrait_amd/module1.py`` (for the parent commit: ``git show HEAD~1:animateportrait_amd/module1.py``),
   loaded beside this one in the same process and alternated with it round by round.  The verdict compares the difference of the
   medians with the parent's own spread (max - min over its rounds).

    python tools/bench_register.py --out profiles/rigid_register.json [--parent_module1 FILE]

Needs a GPU: there is no CPU mode, a time taken without the device would say nothing."""
import argparse
import importlib.util
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


def _stats(seconds):
    return {'median': 1e3 * statistics.median(seconds), 'min': 1e3 * min(seconds), 'max': 1e3 * max(seconds)}


def registration(dev, frames_n, rounds, warmup):
    import register_reference as rr
    from animateportrait_amd import landmark_post as lp, module1 as m1
    std = np.loadtxt(os.path.join(ROOT, 'tests', 'golden', 'STD_FACE_LANDMARKS.txt')).reshape(204).astype(np.float32)
    frames = rr.seeded_frames(std, frames_n, 31)
    fl, sd = torch.from_numpy(frames).to(dev), torch.from_numpy(std).to(dev)

    def device():
        return lp.rigid_register(fl, sd, center=True, no_x_rot=True)

    def twin():
        return torch.from_numpy(m1.stabilise_head(fl.cpu().numpy(), std, True, True)).to(dev)

    legs = (('device', device), ('numpy_twin_with_copies', twin))
    times, outs = {k: [] for k, _ in legs}, {}
    for r in range(warmup + rounds):
        for name, fn in (legs if r % 2 == 0 else legs[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs[name] = fn()
            torch.cuda.synchronize()
            if r >= warmup:
                times[name].append(time.perf_counter() - t0)
    res = {'frames': frames_n, 'flags': 'CENTER | NO_X_ROT', 'ms': {k: _stats(v) for k, v in times.items()},
           'out_linf_device_vs_twin': float((outs['device'] - outs['numpy_twin_with_copies']).abs().max())}
    # the launch alone, between device events
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = torch.empty_like(fl)
    e0.record()
    for _ in range(50):
        lp.rigid_register(fl, sd, center=True, no_x_rot=True, out=out)
    e1.record()
    torch.cuda.synchronize()
    res['ms']['device_back_to_back_per_call'] = e0.elapsed_time(e1) / 50
    # accuracy on the same frames, as tests/test_register_gpu.py measures it
    ref = {f: rr.rigid_register64(frames, std, f) for f in (0, 1, 2, 3, 4)}
    spread = max(float(np.abs(rr.rigid_register64(frames, std, f, svd='jacobi')[1] - ref[f][1]).max()) for f in (0, 1))
    acc = {'pose_spread_lapack_vs_jacobi': spread, 'pose_bar': max(16.0 * spread, 1e-12), 'per_flags': {}}
    for f in (0, 1, 2, 3, 4):
        got, pose = lp.rigid_register(fl, sd, center=bool(f & 1), no_x_rot=bool(f & 2), register=bool(f & 4), pose=True)
        want = ref[f][0].astype(np.float32)
        ulp = np.spacing(np.abs(want).max(axis=1, keepdims=True)).astype(np.float64)
        acc['per_flags'][str(f)] = {'pose_err': float(np.abs(pose.view(-1, 12).cpu().numpy() - ref[f][1]).max()),
                                    'out_err_ulp': float((np.abs(got.cpu().numpy().astype(np.float64) - want) / ulp).max())}
    res['accuracy'] = acc
    return res


def stage(dev, frames_n, rounds, warmup, parent_path):
    from animateportrait_amd import audio, module1 as m1
    versions = {'this': m1}
    if parent_path:
        spec = importlib.util.spec_from_file_location('animateportrait_amd.module1_parent', parent_path)
        parent = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = parent
        spec.loader.exec_module(parent)
        versions['parent'] = parent
    torch.manual_seed(1234)
    content = m1.Audio2LandmarkContent(use_prior_net=True, drop_out=0.5).to(dev).eval()
    pose = m1.Audio2LandmarkPos(drop_out=0.5).to(dev).eval()
    spk = torch.randn(256, generator=torch.Generator().manual_seed(7))
    fid = torch.randn(204, generator=torch.Generator().manual_seed(8)) * 0.1
    au = audio.clip_audio_features(os.path.join(ROOT, 'tests', 'golden', 'female12.wav'), max_frames=frames_n)
    res = {'windows': int(au.shape[0])}
    for backend in ('host', 'device'):
        names = list(versions)
        times, outs = {n: [] for n in names}, {}
        for n in names:
            versions[n].set_post_backend(backend)
        try:
            for r in range(warmup + rounds):
                for n in (names if r % 2 == 0 else names[::-1]):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fl = versions[n].predict_landmarks_speaker_aware(pose, content, au, spk, fid)
                    torch.cuda.synchronize()
                    if r >= warmup:
                        times[n].append(time.perf_counter() - t0)
                    outs[n] = np.asarray(fl.cpu() if torch.is_tensor(fl) else fl)
        finally:
            for n in names:
                versions[n].set_post_backend('host')
        row = {'ms': {n: _stats(times[n]) for n in names}}
        if 'parent' in versions:
            row['bit_equal_to_parent'] = bool(np.array_equal(outs['this'], outs['parent']))
            diff = row['ms']['this']['median'] - row['ms']['parent']['median']
            spread = row['ms']['parent']['max'] - row['ms']['parent']['min']
            row['median_minus_parent_ms'], row['parent_spread_ms'] = diff, spread
            row['within_parent_spread'] = bool(abs(diff) <= spread)
        res[backend] = row
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--rounds', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--frames', type=int, default=625)
    ap.add_argument('--parent_module1', default=None, help="another revision's animateportrait_amd/module1.py to time the stage against")
    ap.add_argument('--out', default=None, help='write the result as JSON here as well')
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('bench_register: no GPU')
    dev = torch.device('cuda:0')
    res = {'device': torch.cuda.get_device_name(0), 'rounds': a.rounds, 'warmup': a.warmup,
           'unit': 'ms (median over the alternated rounds; min and max beside it)',
           'registration': registration(dev, a.frames, a.rounds, a.warmup),
           'module1_stage_switches_off': stage(dev, a.frames, a.rounds, a.warmup, a.parent_module1)}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
