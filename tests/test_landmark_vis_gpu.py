"""apd_landmark_vis on the MI355X: every picture equals, byte for byte under apd_frames_to_u8's rule and with no pixel left
out, the composition of oracle/cv_raster primitives in tests/landmark_vis_reference.py; every call writes between guard
values, which must stay intact; a given background passes through bit for bit.  Last: end2end.py --landmark_video avi
--side_outputs writes a preview clip the RIFF reader and PIL read back, and leaves output.avi as it was."""
import ctypes
import os
import sys
import wave

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_fixture as jf                     # noqa: E402
import landmark_vis_reference as ref          # noqa: E402

pytestmark = pytest.mark.gpu
GUARD, GUARD_VALUE = 64, 12345.5              # floats before and after `out`
CASES = ref.cases()


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def expected():
    """the reference pictures, composed once"""
    return {name: ref.expected(case) for name, case in CASES.items()}


def _ptr(t, offset=0):
    return ctypes.c_void_p(t.data_ptr() + offset) if t is not None else None


def _u8(frames):
    """(N, 3, H, W) device float32 -> (N, H, W, 3) uint8 by apd_frames_to_u8"""
    from animateportrait_amd.data import visuals
    return visuals.frames_to_u8(frames, out='device').cpu().numpy()


def _draw_guarded(dev, h, w, pts, seg, rgb, radius, thickness, disc_rgb, bg_rgb, bg=None, front=GUARD):
    """apd_landmark_vis through ctypes into a buffer with `front` guard floats before and GUARD after `out` -> (N, 3, h, w) device
    float32; asserts rc == 0 and the guards.  front = GUARD keeps `out` 16-byte aligned, front = GUARD + 1 does not."""
    from animateportrait_amd import _dataapi as D
    lib = D.lib()
    pts_d = torch.from_numpy(np.ascontiguousarray(pts, np.int32)).to(dev)
    n, p, s = pts.shape[0], pts.shape[1], len(seg)
    seg_h = np.ascontiguousarray(seg, np.int32)
    seg_d = torch.from_numpy(seg_h).to(dev) if s else None
    rgb_d = torch.from_numpy(np.ascontiguousarray(rgb, np.uint32).view(np.int32)).to(dev) if s else None
    count = n * 3 * h * w
    buf = torch.full((front + count + GUARD,), GUARD_VALUE, dtype=torch.float32, device=dev)
    rc = lib.apd_landmark_vis(_ptr(pts_d), _ptr(seg_d), seg_h.ctypes.data_as(ctypes.c_void_p) if s else None, _ptr(rgb_d), _ptr(bg),
                              bg.shape[0] if bg is not None else 1, n, p, s, h, w, radius, thickness, disc_rgb, bg_rgb, _ptr(buf, 4 * front),
                              ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize(dev)
    assert rc == 0, D.last_error()
    assert bool((buf[:front] == GUARD_VALUE).all()) and bool((buf[front + count:] == GUARD_VALUE).all()), 'guards of out'
    return buf[front:front + count].view(n, 3, h, w)


def _differing(got, want):
    return int((got != want).any(-1).sum())


@pytest.mark.parametrize('name', sorted(CASES))
def test_pictures_equal_the_reference(dev, expected, name):
    """every case twice: the same bytes again, every pixel compared; face256 also into an `out` that is not 16-byte aligned"""
    h, w, pts, seg, rgb, radius, thickness, disc_rgb, bg_rgb = CASES[name]
    first = _draw_guarded(dev, *CASES[name])
    got = _u8(first)
    assert got.shape == expected[name].shape
    print('%s: %d pixels differ' % (name, _differing(got, expected[name])))
    assert _differing(got, expected[name]) == 0
    assert len(np.unique(expected[name].reshape(-1, 3), axis=0)) >= (1 if name == 'one1x1' else 3)      # the picture is not blank
    again = _draw_guarded(dev, *CASES[name])
    assert torch.equal(first.view(torch.int32), again.view(torch.int32))
    # only the bucket middles of the colours are ever stored
    levels = torch.from_numpy(ref.bucket_middle(np.arange(256))).to(dev)
    assert bool(torch.isin(first, levels).all())
    if name == 'face256':
        shifted = _draw_guarded(dev, *CASES[name], front=GUARD + 1)
        assert torch.equal(first.view(torch.int32), shifted.contiguous().view(torch.int32))


def test_binding_gives_the_same_frames(dev, expected):
    from animateportrait_amd.data import visuals
    h, w, pts, seg, rgb, radius, thickness, disc_rgb, bg_rgb = CASES['painter_t5_r3']
    out = visuals.landmark_vis(torch.from_numpy(pts).to(dev), seg, rgb, h, w, radius, thickness, disc_rgb, bg_rgb=bg_rgb)
    assert out.shape == (3, 3, h, w) and out.dtype == torch.float32 and out.is_cuda
    assert _differing(_u8(out), expected['painter_t5_r3']) == 0
    assert _differing(_u8(visuals.landmark_vis(pts, seg, rgb, h, w, radius, thickness, disc_rgb, bg_rgb=bg_rgb)), expected['painter_t5_r3']) == 0
    with pytest.raises(ValueError, match='integer'):
        visuals.landmark_vis(torch.from_numpy(pts).to(dev).float(), seg, rgb, h, w, radius, thickness, disc_rgb)
    with pytest.raises(RuntimeError, match='thickness = 17'):
        visuals.landmark_vis(pts, seg, rgb, h, w, radius, 17, disc_rgb)
    with pytest.raises(RuntimeError, match='names landmark 6 of 6'):
        visuals.landmark_vis(pts, [(0, 6)], [0], h, w, radius, thickness, disc_rgb)


@pytest.mark.parametrize('h,w', [(37, 53), (40, 52)])
@pytest.mark.parametrize('shared', [True, False])
def test_background_passes_through(dev, h, w, shared):
    """S = 0 with bg, bg_frames 1 and N: discs only; undrawn pixels are bit-equal to bg as floats (NaN, infinities and values
    beyond [-1, 1] included), drawn ones are the disc colour.  53 columns take the one-column route, 52 the four-column one."""
    pts = ref.painter_points()
    pts[:, :, 0] = pts[:, :, 0] * w // 53                                          # keep the layout inside the narrower frame
    n = pts.shape[0]
    rng = np.random.RandomState(h)
    bg = rng.uniform(-1.2, 1.2, (1 if shared else n, 3, h, w)).astype(np.float32)
    bg[0, :, 0, :6] = [np.nan, np.inf, -np.inf, -0.0, 1.0, -1.0]
    bg_d = torch.from_numpy(bg).to(dev)
    keep = bg_d.clone()
    none = np.zeros((0, 2), np.int32)
    out = _draw_guarded(dev, h, w, pts, none, np.zeros((0,), np.uint32), 3, 2, 0x00FF7F, 0, bg=bg_d)
    assert torch.equal(bg_d.view(torch.int32), keep.view(torch.int32))             # the background itself is only read
    drawn = np.stack([ref.draw(p, none, [], h, w, 3, 2, 0xFFFFFF, 0x000000) for p in pts])[..., 0] > 0        # (N, h, w)
    assert drawn[:, 3:-3, 3:-3].sum() > 3 * 25 and not drawn.all()
    got, full = out.cpu().numpy(), np.broadcast_to(bg, (n, 3, h, w))
    mask = np.broadcast_to(drawn[:, None], got.shape)
    assert np.array_equal(got.view(np.int32)[~mask], np.ascontiguousarray(full).view(np.int32)[~mask])
    assert np.array_equal(got[mask].reshape(-1), np.broadcast_to(ref.bucket_middle([0x00, 0xFF, 0x7F])[None, :, None, None], got.shape)[mask])
    want = np.stack([ref.draw(pts[i], none, [], h, w, 3, 2, 0x00FF7F, bg=ref.to_u8(full[i]).transpose(1, 2, 0)) for i in range(n)])
    assert _differing(_u8(out), want) == 0


def test_end2end_writes_the_landmark_preview(dev, tmp_path):
    """end2end.main --landmark_video avi --landmark_video_size 256 --side_outputs --video avi --frames none on the synthetic 5-frame
    clip of test_end2end_writes_an_avi: landmark_seq2.avi holds 5 MJPG frames of 256 x 256 within check_file's bounds of the
    reference pictures, and the sound; ori_view.png and photo.png decode to the expected bytes; output.avi is what a run without
    the new flags writes."""
    from PIL import Image
    from animateportrait_amd import end2end, standins
    from animateportrait_amd.data import visuals
    from animateportrait_amd.synthetic import make_landmarks
    yy, xx = np.meshgrid(np.linspace(-1, 1, 256), np.linspace(-1, 1, 256), indexing='ij')
    photo = np.stack([np.sin(3 * xx + yy), np.cos(2 * yy - xx), xx * yy], -1)
    Image.fromarray(((photo + 1) * 127.5).astype(np.uint8)).save(tmp_path / 'photo.png')
    Image.fromarray(((((yy / 0.8) ** 2 + (xx / 0.6) ** 2) < 1) * 255).astype(np.uint8)).save(tmp_path / 'matte.png')
    lm0 = make_landmarks(1, torch.Generator().manual_seed(9))[0]
    t = torch.arange(5).view(5, 1, 1).float()
    seq = lm0.unsqueeze(0) + 2.0 * torch.sin(0.3 * t + lm0.unsqueeze(0) / 40.0)
    np.save(tmp_path / 'lm.npy', torch.cat([lm0.unsqueeze(0), seq]).numpy())
    samples = np.random.RandomState(6).randint(-2000, 2000, 5 * 256 + 100).astype('<i2')
    with wave.open(str(tmp_path / 'a.wav'), 'wb') as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(16000)
        f.writeframes(samples.tobytes())

    def prepare(model):
        model.aux['netF'] = standins.StandinFlowNet().to(dev)
        model.aux['modnet'] = standins.StandinMatteNet().to(dev)

    def run(out, extra):
        torch.manual_seed(7)                                          # --allow_random_init: the same weights in both runs
        assert end2end.main(['--photo', str(tmp_path / 'photo.png'), '--matte', str(tmp_path / 'matte.png'), '--landmarks_npy',
                             str(tmp_path / 'lm.npy'), '--out', str(out), '--batch', '2', '--video', 'avi', '--frames', 'none', '--audio',
                             str(tmp_path / 'a.wav'), '--ngf', '8', '--allow_random_init', '--name', 'run', '--checkpoints_dir',
                             str(tmp_path / 'ck')] + extra, prepare_model=prepare) == 0
    plain, full = tmp_path / 'plain', tmp_path / 'full'
    run(plain, [])
    run(full, ['--landmark_video', 'avi', '--landmark_video_size', '256', '--side_outputs'])
    assert 'output.avi' in os.listdir(plain)
    assert set(os.listdir(full)) - set(os.listdir(plain)) == {'landmark_seq2.avi', 'ori_view.png', 'photo.png'}
    assert (full / 'output.avi').read_bytes() == (plain / 'output.avi').read_bytes()
    got = jf.read_avi((full / 'landmark_seq2.avi').read_bytes())
    assert got['avih'][4] == 5 and (got['avih'][8], got['avih'][9]) == (256, 256) and len(got['streams']) == 2
    assert got['streams'][0][0][1] == b'MJPG' and (got['streams'][0][0][7], got['streams'][0][0][6]) == (125, 2)
    video = [p for cc, p in got['movi'] if cc == b'00dc']
    assert len(video) == 5
    assert b''.join(p for cc, p in got['movi'] if cc == b'01wb') == samples.tobytes()
    table = visuals.FACE_CONTOURS
    pts = seq.numpy().astype(np.int32)                                # size_out / --size = 1; vis_landmark's truncation
    for k in range(5):
        want = ref.draw(pts[k], table['segments'], table['colours'], 256, 256, 1, 2, table['disc_rgb'])
        assert len(np.unique(want.reshape(-1, 3), axis=0)) == 7       # white, five curve colours, red
        figures = jf.check_file(video[k], want, 90)
        print('frame %d: %d bytes; PSNR %.3f dB, max error %d; PIL\'s file %.3f dB, %d' % ((k, len(video[k])) + figures))
    seen = _u8(end2end.load_photo(str(tmp_path / 'photo.png'), 256).to(dev))[0]
    assert np.array_equal(np.asarray(Image.open(full / 'photo.png').convert('RGB')), seen)
    marks = np.array([[round(float(x)), round(float(y))] for x, y in lm0.numpy()], np.int64)
    want = ref.draw(marks, np.zeros((0, 2), np.int32), [], 256, 256, round(5 * 256 / 512), 1, 0xFF0000, bg=seen)
    assert (want != seen).any(-1).sum() > 68 and round(5 * 256 / 512) == 2
    view = Image.open(full / 'ori_view.png')
    assert view.mode == 'RGB' and np.array_equal(np.asarray(view), want)
