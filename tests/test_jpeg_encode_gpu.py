"""apd_jpeg_encode on the MI355X: the device's bytes equal those of the encoder's host build (tests/golden/jpeg_host.npz),
every file passes tests/jpeg_fixture.check_file (the marker walker, PIL as decoder, PIL's encoder at the same tables as the
yardstick); every call writes into slots pre-filled with 0xA5 between sentinel guards, which must stay intact, as must every
byte past sizes[n].  Last: end2end.py --video avi --frames none writes a clip the RIFF reader and PIL read back."""
import ctypes
import os
import sys
import wave

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_fixture as jf         # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, FILL, SENTINEL = 4096, 0xA5, 0x3C
IMAGES = jf.images()


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'jpeg_host.npz'))


def _ptr(t, offset=0):
    return ctypes.c_void_p(t.data_ptr() + offset)


def _encode_guarded(dev, frames, channels, quality=90, where='device'):
    """apd_jpeg_encode through ctypes -> (rc, [file bytes], slots (N, slot) uint8 array).  where: 'device', 'pinned' or
    'pageable' memory for the slots and the sizes.  Asserts the guards and the bytes past sizes[n] on success."""
    from animateportrait_amd import _dataapi as D
    lib = D.lib()
    frames = torch.as_tensor(frames, dtype=torch.float32).to(dev).contiguous()
    n, c, h, w = frames.shape
    slot, ws_bytes = lib.apd_jpeg_bound(h, w, channels), lib.apd_jpeg_workspace_bytes(n, h, w, channels)
    assert slot > 0 and ws_bytes > 0

    def make(count, dtype, fill, guard):
        t = torch.full((count + 2 * guard,), SENTINEL, dtype=dtype)
        t[guard:guard + count] = fill
        return t.to(dev) if where == 'device' else t.pin_memory() if where == 'pinned' else t
    buf, sizes = make(n * slot, torch.uint8, FILL, GUARD), make(n, torch.int32, -7, 16)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    rc = lib.apd_jpeg_encode(_ptr(frames), n, c, h, w, channels, quality, _ptr(buf, GUARD), slot, _ptr(sizes, 64), _ptr(ws), ws_bytes,
                             ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize(dev)
    buf, sizes = buf.cpu().numpy(), sizes.cpu().numpy()
    assert (buf[:GUARD] == SENTINEL).all() and (buf[GUARD + n * slot:] == SENTINEL).all(), 'guards of the slots'
    assert (sizes[:16] == SENTINEL).all() and (sizes[16 + n:] == SENTINEL).all(), 'guards of the sizes'
    slots = buf[GUARD:GUARD + n * slot].reshape(n, slot)
    if rc < 0:
        return rc, None, slots
    files = []
    for i in range(n):
        size = int(sizes[16 + i])
        assert 538 < size <= slot, (i, size, slot)
        assert (slots[i, size:] == FILL).all(), 'frame %d: bytes past sizes[n] were written' % i
        files.append(slots[i, :size].tobytes())
    return rc, files, slots


def _u8(dev, frames, channels):
    """the samples the files must hold: apd_frames_to_u8's, the first channel alone for greyscale files"""
    from animateportrait_amd.data import visuals
    want = visuals.frames_to_u8(torch.as_tensor(frames, dtype=torch.float32).to(dev), out='device').cpu().numpy()
    return want if channels == 3 else want[..., :1]


@pytest.mark.parametrize('name,quality', jf.golden_cases())
def test_device_bytes_equal_the_host_build(dev, golden, name, quality):
    im = IMAGES[name]
    channels = im.shape[2]
    frames = jf.to_frames(im)
    assert np.array_equal(_u8(dev, frames, channels)[0], im)          # the frames do carry the image
    rc, files, _ = _encode_guarded(dev, frames, channels, quality)
    assert rc == 0
    print('%s q%d: %d bytes; PSNR %.3f dB, max error %d; PIL\'s file %.3f dB, %d' % ((name, quality, len(files[0])) + jf.measure(files[0], im, quality)))
    assert files[0] == golden[jf.key(name, quality)].tobytes()
    jf.check_file(files[0], im, quality)


@pytest.mark.parametrize('c,channels', [(1, 1), (1, 3), (3, 3)])
def test_three_frames_in_one_call(dev, c, channels):
    """N = 3, 37 x 53: grey to grey, grey tiled to RGB, RGB; with NaN, infinities and values beyond [-1, 1], which clamp"""
    rng = np.random.RandomState(c * 10 + channels)
    frames = rng.uniform(-1, 1, (3, c, 37, 53)).astype(np.float32)
    frames[1] *= 0.6                                                 # lower contrast: a smaller file
    frames[1, 0, 0, :12] = [np.nan, -1.5, 3.0, 1e30, -1e30, np.inf, -np.inf, 1.0000001, -1.0000001, 0.0, 1.0, -1.0]
    frames[2, :, 5:30] = 1.0                                         # rows of white: flat blocks
    want = _u8(dev, frames, channels)
    assert want[1, 0, :12, 0].tolist() == [0, 0, 255, 255, 0, 255, 0, 255, 0, 127, 255, 0]
    rc, files, _ = _encode_guarded(dev, frames, channels)
    assert rc == 0 and len(files) == 3
    for i in range(3):
        jf.check_file(files[i], want[i], 90)
    assert len({len(f) for f in files}) == 3 and len(files[2]) < len(files[0])           # the files differ in size


@pytest.mark.parametrize('name', ['wide8x2048_rgb', 'tall80x24'])
def test_quality_100(dev, name):
    """the longest strings: 768 blocks in one segment (three chunks, carried bits), and ten segments whose RSTm wraps"""
    im = IMAGES[name]
    rc, files, _ = _encode_guarded(dev, jf.to_frames(im), im.shape[2], 100)
    assert rc == 0
    jf.check_file(files[0], im, 100)


def test_same_bytes_again_and_in_pinned_memory(dev):
    frames = np.concatenate([jf.to_frames(IMAGES['noise37x53_rgb']), jf.to_frames(IMAGES['lines256_rgb'][:37, :53]),
                             jf.to_frames(IMAGES['noise37x53_rgb'][::-1])])
    rc, first, _ = _encode_guarded(dev, frames, 3)
    rc2, second, _ = _encode_guarded(dev, frames, 3)
    rc3, pinned, _ = _encode_guarded(dev, frames, 3, where='pinned')
    assert rc == 0 and rc2 == 0 and rc3 == 0
    assert first == second and first == pinned
    assert first[0] != first[2]


def test_pageable_memory_is_refused(dev):
    from animateportrait_amd import _dataapi as D
    rc, _, slots = _encode_guarded(dev, jf.to_frames(IMAGES['noise37x53_grey']), 1, where='pageable')
    assert rc < 0 and 'neither device memory nor pinned' in D.last_error() and (slots == FILL).all()


def test_encode_jpeg_batch_reuses_its_buffer(dev):
    from animateportrait_amd.data import visuals
    rng = np.random.RandomState(3)
    grey = torch.from_numpy(rng.uniform(-1, 1, (3, 1, 37, 53)).astype(np.float32)).to(dev)
    buf, sizes = visuals.encode_jpeg_batch(grey, channels=1, quality=75)
    torch.cuda.synchronize(dev)
    first = [buf.numpy()[i, :int(sizes[i])].tobytes() for i in range(3)]
    again, _ = visuals.encode_jpeg_batch(grey, channels=1, quality=75)
    other, _ = visuals.encode_jpeg_batch(grey, channels=1, quality=75, slot=1)
    torch.cuda.synchronize(dev)
    assert buf.is_pinned() and sizes.is_pinned() and again.data_ptr() == buf.data_ptr() != other.data_ptr()
    want = _u8(dev, grey, 1)
    for i in range(3):
        assert buf.numpy()[i, :int(sizes[i])].tobytes() == first[i]
        jf.check_file(first[i], want[i], 75)
    with pytest.raises(RuntimeError, match='needs C = 1'):
        visuals.encode_jpeg_batch(grey.repeat(1, 3, 1, 1), channels=1)


def test_end2end_writes_an_avi(dev, tmp_path):
    """end2end.main --video avi --frames none on a synthetic 5-frame clip at ngf 8, stand-in aux nets, --allow_random_init:
    output.avi holds 5 MJPG frames within check_file's bounds of the frames ClipStreamer gives for the same seed, and the sound"""
    from PIL import Image
    from animateportrait_amd import end2end, standins, stream
    from animateportrait_amd.models import create_model
    from animateportrait_amd.options.base_options import TestOptions
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
    with wave.open(str(tmp_path / 'a.wav'), 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(samples.tobytes())

    def prepare(model):
        model.aux['netF'] = standins.StandinFlowNet().to(dev)
        model.aux['modnet'] = standins.StandinMatteNet().to(dev)
    model_args = ['--ngf', '8', '--allow_random_init', '--name', 'run', '--checkpoints_dir', str(tmp_path / 'ck')]
    torch.manual_seed(7)                                              # --allow_random_init: the same weights in both builds
    out = tmp_path / 'out'
    assert end2end.main(['--photo', str(tmp_path / 'photo.png'), '--matte', str(tmp_path / 'matte.png'), '--landmarks_npy',
                         str(tmp_path / 'lm.npy'), '--out', str(out), '--batch', '2', '--video', 'avi', '--frames', 'none', '--audio',
                         str(tmp_path / 'a.wav')] + model_args, prepare_model=prepare) == 0
    assert (out / 'output.avi').exists() and not (out / 'frames').exists()
    got = jf.read_avi((out / 'output.avi').read_bytes())
    assert got['avih'][4] == 5 and (got['avih'][8], got['avih'][9]) == (256, 256) and len(got['streams']) == 2
    assert (got['streams'][0][0][7], got['streams'][0][0][6]) == (125, 2)
    video = [p for cc, p in got['movi'] if cc == b'00dc']
    assert len(video) == 5
    assert b''.join(p for cc, p in got['movi'] if cc == b'01wb') == samples.tobytes()
    # the same clip through the streamer directly, the model built the way end2end.main builds it
    opt = TestOptions().parse(['--model', 'geomcgt_ifw_test', '--netG', 'resnet_9blocks_rcatland32_full_ifw', '--netg_resb_div', '3',
                               '--netg_resb_disp', '3', '--output_nc', '1', '--dataset_mode', 'synthetic', '--blendbg', '1', '--gpu_ids',
                               '0'] + model_args)
    torch.manual_seed(7)
    model = create_model(opt)
    prepare(model)
    model.setup(opt)
    model.eval()
    frames = stream.ClipStreamer(model, batch=2).run(end2end.load_photo(str(tmp_path / 'photo.png'), 256), lm0.numpy(), seq.numpy(),
                                                     matte=end2end.load_matte(str(tmp_path / 'matte.png'), 256))
    assert frames.shape == (5, 1, 256, 256)
    want = _u8(dev, frames, 1)
    assert want.std() > 1.0
    for k in range(5):
        figures = jf.check_file(video[k], want[k], 90)                # 1-channel frames: greyscale files by default
        print('frame %d: %d bytes; PSNR %.3f dB, max error %d; PIL\'s file %.3f dB, %d' % ((k, len(video[k])) + figures))
