#!/usr/bin/env python3
"""The sink stage of a clip, three ways in one run: the frames of a 625-frame, 256 x 256, 1-channel line-drawing clip lie on
the device (as ClipStreamer leaves them) and are written as

  png      <out>/frames/%05d.png by apd_png_encode       (end2end.py --png_encoder device: the yardstick)
  avi      <out>/output.avi, MJPG + PCM, by apd_jpeg_encode and util/avi.py   (--video avi --frames none)
  both     the two one after the other                                          (--video avi)

Each is timed from the first launch to the last byte handed to the file system, after one warm-up pass; the JSON line also
carries the JPEG bytes per frame at quality 90 and the time of apd_jpeg_encode alone per batch.

    python tools/bench_video_sink.py [--frames 625] [--out profiles/r10_video_sink.json]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time
import wave

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def clip(frames, size, device):
    """a line drawing that moves: frame k is the fixture's drawing rolled by k pixels, grey, in [-1, 1]"""
    import png_fixture as pf
    base = torch.from_numpy(pf.to_frames(pf.line_drawing(size)[:, :, :1])[0]).to(device)
    return torch.stack([torch.roll(base, shifts=(k % size, (2 * k) % size), dims=(1, 2)) for k in range(frames)])


def main():
    from animateportrait_amd import end2end
    from animateportrait_amd.data import visuals
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=625)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--quality', type=int, default=90)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r10_video_sink.json'))
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    frames = clip(a.frames, a.size, dev)
    work = tempfile.mkdtemp()
    wav = os.path.join(work, 'a.wav')
    with wave.open(wav, 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(np.zeros(a.frames * 256, '<i2').tobytes())
    fdir, video = os.path.join(work, 'frames'), os.path.join(work, 'output.avi')
    os.makedirs(fdir)

    def png():
        end2end.write_frames(frames, fdir, 'device', a.batch, 3)

    def avi():
        end2end.write_avi(frames, video, 62.5, wav, a.batch, None, a.quality)

    def both():
        png()
        avi()

    def timed(fn):
        fn()                                                # warm-up: buffers pinned, files created
        best = float('inf')
        for _ in range(a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            best = min(best, time.perf_counter() - t0)
        return round(best * 1e3, 2)
    res = {'clip_frames': a.frames, 'size': a.size, 'channels': 1, 'batch': a.batch, 'quality': a.quality, 'repeats': a.repeats}
    res['png_device_ms'] = timed(png)
    res['avi_ms'] = timed(avi)
    res['both_ms'] = timed(both)
    res['avi_over_png'] = round(res['avi_ms'] / res['png_device_ms'], 3)
    res['both_over_png'] = round(res['both_ms'] / res['png_device_ms'], 3)
    res['png_bytes'] = sum(os.path.getsize(os.path.join(fdir, f)) for f in os.listdir(fdir))
    res['avi_bytes'] = os.path.getsize(video)
    buf, sizes = visuals.encode_jpeg_batch(frames[:a.batch], channels=1, quality=a.quality, slot='bench')
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(10):
        visuals.encode_jpeg_batch(frames[:a.batch], channels=1, quality=a.quality, slot='bench')
    stop.record()
    torch.cuda.synchronize()
    res['jpeg_encode_ms_per_batch'] = round(start.elapsed_time(stop) / 10, 3)
    res['jpeg_bytes_per_frame_q%d' % a.quality] = round(float(sizes.float().mean()), 1)
    shutil.rmtree(work)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
