#!/usr/bin/env python3
"""The sink stage of the landmark preview (end2end.py --landmark_video avi) beside the sink stage of the clip itself
(--video avi, the yardstick of tools/bench_video_sink.py), in one process and in alternation:

  preview   625 landmark sets -> apd_landmark_vis (512 x 512 x 3, --batch frames per launch) -> apd_jpeg_encode -> landmark_seq2.avi
  clip      625 frames of 256 x 256 x 1 that lie on the device -> apd_jpeg_encode -> output.avi

Each is timed from the first launch to the last byte handed to the file system, after one warm-up pass.  Device events then
time the raster launches of the whole preview alone, and the JPEG encodes of the very same frames alone.

    python tools/bench_landmark_video.py [--frames 625] [--out profiles/r11_landmark_video.json]
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
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def landmark_clip(frames, size=256):
    """(frames, 68, 2) float32 in pixels of a `size` frame: the synthetic face, every point on a small orbit of its own"""
    from animateportrait_amd.synthetic import make_landmarks
    lm0 = make_landmarks(1, torch.Generator().manual_seed(9))[0] * (size / 256.0)
    t = torch.arange(frames).view(frames, 1, 1).float()
    return (lm0.unsqueeze(0) + 3.0 * torch.sin(0.11 * t + lm0.unsqueeze(0) / 40.0)).numpy().astype(np.float32)


def main():
    import bench_video_sink
    from animateportrait_amd import end2end
    from animateportrait_amd.data import visuals
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=625)
    ap.add_argument('--size', type=int, default=512, help='side of the preview frames')
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--quality', type=int, default=90)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r11_landmark_video.json'))
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    frames = bench_video_sink.clip(a.frames, 256, dev)
    seq = landmark_clip(a.frames)
    work = tempfile.mkdtemp()
    wav = os.path.join(work, 'a.wav')
    with wave.open(wav, 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(np.zeros(a.frames * 256, '<i2').tobytes())
    video, preview = os.path.join(work, 'output.avi'), os.path.join(work, 'landmark_seq2.avi')

    def clip_sink():
        end2end.write_avi(frames, video, 62.5, wav, a.batch, None, a.quality)

    def preview_sink():
        end2end.write_landmark_avi(seq, preview, 62.5, dev, wav, a.batch, 256, a.size, a.quality)

    def once(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        return round((time.perf_counter() - t0) * 1e3, 2)
    clip_sink()                                             # warm-up: buffers pinned, files created, code objects loaded
    preview_sink()
    runs = {'clip': [], 'preview': []}
    for _ in range(a.repeats):                              # alternated: both see the same state of a shared host
        runs['clip'].append(once(clip_sink))
        runs['preview'].append(once(preview_sink))
    res = {'clip_frames': a.frames, 'preview_size': a.size, 'clip_size': 256, 'batch': a.batch, 'quality': a.quality, 'repeats': a.repeats,
           'clip_avi_ms_runs': runs['clip'], 'preview_avi_ms_runs': runs['preview'],
           'clip_avi_ms': min(runs['clip']), 'preview_avi_ms': min(runs['preview'])}
    res['preview_over_clip'] = round(res['preview_avi_ms'] / res['clip_avi_ms'], 3)
    res['clip_avi_bytes'], res['preview_avi_bytes'] = os.path.getsize(video), os.path.getsize(preview)
    # the raster launches of the whole preview alone, then the encodes of the same frames alone
    table = visuals.FACE_CONTOURS
    thickness, radius = visuals.face_contour_style(a.size)
    pts = torch.from_numpy(end2end.truncated_landmarks(seq, a.size / 256.0)).to(dev)

    def draw(k0):
        return visuals.landmark_vis(pts[k0:k0 + a.batch], table['segments'], table['colours'], a.size, a.size, radius, thickness,
                                    table['disc_rgb'])
    starts = list(range(0, a.frames, a.batch))
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    raster = []
    for _ in range(a.repeats):
        torch.cuda.synchronize()
        start.record()
        for k0 in starts:
            draw(k0)
        stop.record()
        torch.cuda.synchronize()
        raster.append(round(start.elapsed_time(stop), 3))
    encode = 0.0
    for k0 in starts:
        batch = draw(k0)
        start.record()
        visuals.encode_jpeg_batch(batch, channels=3, quality=a.quality, slot='bench')
        stop.record()
        torch.cuda.synchronize()
        encode += start.elapsed_time(stop)
    res['raster_launches'] = len(starts)
    res['raster_ms_runs'] = raster
    res['raster_ms'] = min(raster)
    res['jpeg_encode_same_frames_ms'] = round(encode, 3)
    res['raster_over_jpeg_encode'] = round(res['raster_ms'] / encode, 3)
    res['raster_store_gb_per_s'] = round(a.frames * 3 * a.size * a.size * 4 / (res['raster_ms'] * 1e-3) / 1e9, 1)
    shutil.rmtree(work)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
