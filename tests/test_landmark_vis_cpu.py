"""apd_landmark_vis without a device: the names the data ABI gained, what apd_landmark_vis_ok serves and refuses, the kernel's
per-pixel rule (csrc/data/landmark_vis.h) compiled for the host under -fsanitize=address,undefined by
tools/landmark_vis_host_check.py against the composition of tests/landmark_vis_reference.py, the bucket-middle encoding of a
drawn byte, the FACE_CONTOURS table and the entry point's new flags."""
import ctypes
import importlib.util
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import landmark_vis_reference as ref          # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ('apd_landmark_vis_ok', 'apd_landmark_vis')


def test_new_names_are_declared_and_exported():
    from animateportrait_amd import _dataapi as D
    header = open(os.path.join(ROOT, 'include', 'animateportrait_data.h')).read()
    assert all(n in D.SIGNATURES and n + '(' in header for n in NEW_NAMES)
    assert '#define APD_ABI_VERSION 1' in header and D.ABI_VERSION == 1
    lib = D.lib()
    assert all(hasattr(lib, n) for n in NEW_NAMES) and lib.apd_abi_version() == 1


def test_ok_serves_the_corners_and_refuses_each_limit():
    """the device pointers are never dereferenced by apd_landmark_vis_ok: any non-null value stands in; seg_host is read"""
    from animateportrait_amd import _dataapi as D
    lib = D.lib()
    x, far = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 40)

    def ok(pts=x, seg=x, rgb=x, bg=None, bg_frames=1, n=2, p=68, s=2, h=37, w=53, radius=1, thickness=2, out=far, table=None):
        table = np.array(table if table is not None else [(0, p - 1)] * s, np.int32).reshape(-1, 2)
        host = table.ctypes.data_as(ctypes.c_void_p) if s else None
        return lib.apd_landmark_vis_ok(pts, seg if s else None, host, rgb if s else None, bg, bg_frames, n, p, s, h, w, radius, thickness,
                                       0xFF0000, 0xFFFFFF, out)
    assert ok() == 1
    assert ok(n=1, p=1, s=0, h=1, w=1, radius=-1, thickness=1) == 1
    assert ok(n=65535, p=1024, s=128, h=1024, w=1024, radius=31, thickness=16) == 1
    assert ok(bg=x, bg_frames=1) == 1 and ok(bg=x, bg_frames=2) == 1
    for bad, word in ((dict(p=0, s=0), 'P = 0'), (dict(p=1025), 'P = 1025'), (dict(s=129), 'S = 129'), (dict(h=1025), '1025 x 53'),
                      (dict(w=0), '37 x 0'), (dict(thickness=0), 'thickness = 0'), (dict(thickness=17), 'thickness = 17'),
                      (dict(radius=32), 'radius = 32'), (dict(radius=-2), 'radius = -2'), (dict(n=0), 'N = 0'), (dict(n=65536), 'N = 65536'),
                      (dict(bg=x, bg_frames=3), 'bg_frames = 3'), (dict(bg=x, bg_frames=0), 'bg_frames = 0'),
                      (dict(table=[(0, 1), (5, 68)]), 'segment 1 names landmark 68 of 68'), (dict(table=[(-1, 1), (5, 6)]), 'landmark -1'),
                      (dict(out=None), 'null'), (dict(pts=None), 'null'), (dict(rgb=None), 'no segment table'),
                      (dict(bg=far, bg_frames=1), 'overlaps'), (dict(bg=ctypes.c_void_p((1 << 40) + 2 * 3 * 37 * 53 * 4 - 4)), 'overlaps')):
        assert ok(**bad) == 0, bad
        assert 'landmark_vis' in D.last_error() and word in D.last_error(), (bad, D.last_error())
    assert ok(bg=ctypes.c_void_p((1 << 40) + 2 * 3 * 37 * 53 * 4)) == 1                     # bg right behind out: no overlap
    # the launching call refuses the same way, before it asks the runtime anything: nothing is launched
    assert lib.apd_landmark_vis(x, None, None, None, None, 1, 2, 68, 0, 37, 53, 32, 2, 0xFF0000, 0xFFFFFF, far, None) < 0
    assert 'radius = 32' in D.last_error()


def test_host_program_equals_the_reference_composition(tmp_path):
    spec = importlib.util.spec_from_file_location('landmark_vis_host_check', os.path.join(ROOT, 'tools', 'landmark_vis_host_check.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    cases = ref.cases()
    expected = {name: ref.expected(c) for name, c in cases.items()}
    # the cases do hold what they are meant to: at the crossing the later segment lies on the earlier, and the disc on both
    pts = ref.painter_points()
    colour = [ref.rgb_bytes(c).tolist() for c in ref.PAINTER_RGB]
    (x, y), (ex, ey) = pts[0, 4], pts[0, 0]
    for name in ('painter_t2_r-1', 'painter_t5_r0', 'painter_t5_r3'):
        first_hidden = expected[name][0, y, x].tolist()
        assert first_hidden == (colour[1] if name.endswith('r-1') else [255, 0, 0]), name
        assert (expected[name][0] == colour[0]).all(-1).sum() > 20                                      # the first segment shows elsewhere
    assert expected['painter_t2_r-1'][0, ey, ex].tolist() == colour[2]                                  # the zero-length segment's cap
    assert expected['painter_t5_r3'][0, y, x + 4].tolist() == colour[1]                                 # beside the disc: the second segment
    assert not (expected['painter_t2_r3'][1] == ref.rgb_bytes(ref.PAINTER_RGB[3])).all(-1).any()           # the segment wholly outside
    got = tool.run(tool.build(str(tmp_path)), str(tmp_path), cases)
    assert tool.compare(cases, got, expected) == 0


def test_bucket_middle_returns_every_byte():
    v = np.arange(256)
    for dtype in (np.float64, np.float32):
        x = ref.bucket_middle(v, dtype)
        assert x.dtype == np.float32 and np.array_equal(ref.to_u8(x), v.astype(np.uint8)), dtype
        assert (np.diff(x) > 0).all() and x[0] > -1          # byte 255 lies above 1: the conversion saturates there, at 255


def test_face_contours_table():
    from animateportrait_amd.data import visuals
    t = visuals.FACE_CONTOURS
    seg, rgb = t['segments'], t['colours']
    assert seg.shape == (64, 2) and seg.dtype == np.int32 and rgb.shape == (64,) and rgb.dtype == np.uint32
    assert seg.min() == 0 and seg.max() == 67 and t['points'] == 68 and t['disc_rgb'] == 0xFF0000
    pairs = [tuple(p) for p in seg.tolist()]
    assert pairs[:16] == [(i, i + 1) for i in range(16)] and set(rgb[:16].tolist()) == {0x1990FF}          # the jaw is drawn first
    closing = [p for p in pairs if p[1] != p[0] + 1]
    assert closing == [(36, 41), (42, 47), (48, 59), (60, 67)]
    assert len(set(pairs)) == 64 and len(set(rgb.tolist())) == 5
    for first, last, colour, count in ((17, 21, 0x32CD32, 4), (22, 26, 0x32CD32, 4), (27, 35, 0x3FE0D0, 8), (36, 41, 0xFF6347, 6),
                                       (42, 47, 0xFF6347, 6), (48, 59, 0xEE82EE, 12), (60, 67, 0xEE82EE, 8)):
        inside = [k for k, (a, b) in enumerate(pairs) if first <= a <= last and first <= b <= last]
        assert len(inside) == count and set(rgb[inside].tolist()) == {colour}, (first, last)
    # no curve joins two parts of the face
    assert not any((a, b) in pairs for a, b in ((16, 17), (21, 22), (26, 27), (35, 36), (41, 42), (47, 48), (59, 60)))
    assert visuals.face_contour_style(256) == (2, 1) and visuals.face_contour_style(512) == (4, 2) and visuals.face_contour_style(255) == (0, 0)


def test_flags():
    from animateportrait_amd import end2end
    ap = end2end.make_parser()
    a = ap.parse_args(['--photo', 'p.png', '--out', 'o'])
    assert (a.landmark_video, a.landmark_video_size, a.landmark_video_quality, a.side_outputs) == ('none', 512, 90, False)
    a = ap.parse_args(['--photo', 'p.png', '--out', 'o', '--landmark_video', 'avi', '--landmark_video_size', '256',
                       '--landmark_video_quality', '75', '--side_outputs'])
    assert (a.landmark_video, a.landmark_video_size, a.landmark_video_quality, a.side_outputs) == ('avi', 256, 75, True)
    for bad in (['--landmark_video_size', '128'], ['--landmark_video_size', '255'], ['--landmark_video_size', '1025'],
                ['--landmark_video', 'mov']):
        with pytest.raises(SystemExit):
            ap.parse_args(['--photo', 'p.png', '--out', 'o'] + bad)
    with pytest.raises(SystemExit):
        end2end.main(['--photo', 'p.png', '--out', 'o', '--landmarks_npy', 'x.npy', '--landmark_video', 'avi', '--landmark_video_quality', '0'])


def test_truncated_landmarks():
    from animateportrait_amd import end2end
    seq = np.array([[[1.9, -1.9], [127.75, 0.49], [np.nan, 1e30]]], np.float32)
    assert end2end.truncated_landmarks(seq, 2.0).tolist() == [[[3, -3], [255, 0], [0, 1 << 20]]]
    assert end2end.truncated_landmarks(seq, 2.0).dtype == np.int32
