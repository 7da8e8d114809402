"""apd_png_encode on the MI355X: every file is read back by the independent decoder of tests/png_fixture.py and by PIL and
must give the bytes of apd_frames_to_u8 exactly; every call writes into slots pre-filled with 0xA5 between sentinel guards,
which must stay intact, as must every byte past sizes[n]."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_fixture as pf          # noqa: E402
import testset_fixture as tf      # noqa: E402

pytestmark = pytest.mark.gpu
GUARD, FILL, SENTINEL = 4096, 0xA5, 0x3C
IMAGES = pf.images()


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    return torch.device('cuda:0')


def _ptr(t, offset=0):
    return ctypes.c_void_p(t.data_ptr() + offset)


def _encode_guarded(dev, frames, channels, where='device'):
    """apd_png_encode through ctypes -> (rc, [file bytes], slots (N, slot) uint8 array).  where: 'device', 'pinned' or
    'pageable' memory for the slots and the sizes.  Asserts the guards and the bytes past sizes[n] on success."""
    from animateportrait_amd import _dataapi as D
    lib = D.lib()
    frames = torch.as_tensor(frames, dtype=torch.float32).to(dev).contiguous()
    n, c, h, w = frames.shape
    slot, ws_bytes = lib.apd_png_bound(h, w, channels), lib.apd_png_workspace_bytes(n, h, w, channels)
    assert slot > 0 and ws_bytes > 0

    def make(count, dtype, fill, guard):
        t = torch.full((count + 2 * guard,), SENTINEL, dtype=dtype)
        t[guard:guard + count] = fill
        return t.to(dev) if where == 'device' else t.pin_memory() if where == 'pinned' else t
    buf, sizes = make(n * slot, torch.uint8, FILL, GUARD), make(n, torch.int32, -7, 16)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    rc = lib.apd_png_encode(_ptr(frames), n, c, h, w, channels, _ptr(buf, GUARD), slot, _ptr(sizes, 64), _ptr(ws), ws_bytes,
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
        assert 66 < size <= slot, (i, size, slot)
        assert (slots[i, size:] == FILL).all(), 'frame %d: bytes past sizes[n] were written' % i
        files.append(slots[i, :size].tobytes())
    return rc, files, slots


def _u8(dev, frames, channels):
    """the pixels the files must hold: apd_frames_to_u8's, the first channel alone for greyscale files"""
    from animateportrait_amd.data import visuals
    want = visuals.frames_to_u8(torch.as_tensor(frames, dtype=torch.float32).to(dev), out='device').cpu().numpy()
    return want if channels == 3 else want[..., :1]


@pytest.mark.parametrize('name', sorted(IMAGES))
def test_files_decode_to_frames_to_u8(dev, name):
    im = IMAGES[name]
    channels = im.shape[2]
    frames = pf.to_frames(im)
    want = _u8(dev, frames, channels)
    assert np.array_equal(want[0], im)                               # the frames do carry the image
    rc, files, _ = _encode_guarded(dev, frames, channels)
    assert rc == 0
    pf.check_both(files[0], want[0])
    print('%s: %d bytes, raw %d' % (name, len(files[0]), im.size))
    if name == 'white256_rgb':
        assert len(files[0]) * 20 <= 196608
    if name == 'lines256_rgb':
        assert len(files[0]) * 3 <= 196608


@pytest.mark.parametrize('c,channels', [(1, 1), (1, 3), (3, 3)])
def test_three_frames_in_one_call(dev, c, channels):
    """N = 3, 37 x 53: grey to grey, grey tiled to RGB, RGB; with NaN, infinities and values beyond [-1, 1], which clamp"""
    rng = np.random.RandomState(c * 10 + channels)
    frames = rng.uniform(-1, 1, (3, c, 37, 53)).astype(np.float32)
    frames[1, 0, 0, :12] = [np.nan, -1.5, 3.0, 1e30, -1e30, np.inf, -np.inf, 1.0000001, -1.0000001, 0.0, 1.0, -1.0]
    frames[2, :, 5:30] = 1.0                                         # rows of white: runs across rows and bands
    want = _u8(dev, frames, channels)
    assert want[1, 0, :12, 0].tolist() == [0, 0, 255, 255, 0, 255, 0, 255, 0, 127, 255, 0]
    rc, files, _ = _encode_guarded(dev, frames, channels)
    assert rc == 0 and len(files) == 3
    for i in range(3):
        pf.check_both(files[i], want[i])
    assert len(files[2]) < len(files[0])                             # and the white rows did shrink


def test_same_bytes_again_and_in_pinned_memory(dev):
    frames = np.concatenate([pf.to_frames(IMAGES['noise37x53_rgb']), pf.to_frames(pf.line_drawing(64, seed=2)[:37, :53]),
                             pf.to_frames(IMAGES['noise37x53_rgb'][::-1])])
    rc, first, _ = _encode_guarded(dev, frames, 3)
    rc2, second, _ = _encode_guarded(dev, frames, 3)
    rc3, pinned, _ = _encode_guarded(dev, frames, 3, where='pinned')
    assert rc == 0 and rc2 == 0 and rc3 == 0
    assert first == second and first == pinned
    assert first[0] != first[2]


def test_pageable_memory_is_refused(dev):
    from animateportrait_amd import _dataapi as D
    rc, _, slots = _encode_guarded(dev, pf.to_frames(IMAGES['noise37x53_grey']), 1, where='pageable')
    assert rc < 0 and 'neither device memory nor pinned' in D.last_error() and (slots == FILL).all()


def test_sink_device_equals_host(dev, tmp_path):
    """save_png_batch with both encoders: a 3-visual dict at N = 3 (grey, RGB, a line drawing); the files decode to equal arrays"""
    from PIL import Image
    from animateportrait_amd.data import visuals
    rng = np.random.RandomState(3)
    drawing = np.stack([pf.to_frames(pf.line_drawing(64, seed=s))[0] for s in (1, 2, 3)])
    shown = {'grey': torch.from_numpy(rng.uniform(-1, 1, (3, 1, 37, 53)).astype(np.float32)).to(dev),
             'rgb': torch.from_numpy(rng.uniform(-1.2, 1.2, (3, 3, 40, 24)).astype(np.float32)).to(dev),
             'lines': torch.from_numpy(drawing).to(dev)}
    names = {e: {l: [str(tmp_path / ('%s_%d_%s.png' % (e, i, l))) for i in range(3)] for l in shown} for e in ('host', 'device')}
    assert visuals.save_png_batch(shown, names['host']) == 9                       # the default is the host encoder
    assert visuals.save_png_batch(shown, names['device'], encoder='device') == 9
    for label, t in shown.items():
        want = _u8(dev, t, 3)
        for i in range(3):
            host = np.asarray(Image.open(names['host'][label][i]))
            data = open(names['device'][label][i], 'rb').read()
            pf.check_both(data, host)
            assert np.array_equal(host, want[i])
    buf, sizes = visuals.encode_png_batch(shown['grey'], channels=1)
    again, _ = visuals.encode_png_batch(shown['grey'], channels=1)
    torch.cuda.synchronize(dev)
    assert buf.is_pinned() and sizes.is_pinned() and again.data_ptr() == buf.data_ptr()         # one buffer per shape, reused
    pf.check_both(buf.numpy()[1, :int(sizes[1])].tobytes(), _u8(dev, shown['grey'], 1)[1])


def test_entry_point_device_encoder_equals_host(dev, tmp_path):
    """test.py --save_format png on the fixture tree with both encoders: the same names, files that decode to equal arrays"""
    from PIL import Image
    from animateportrait_amd import standins, test as entry
    work = tmp_path / 'tree'
    tf.write_test_tree(str(work / 'root'), str(work / 'lists'))

    def prepare(model):
        torch.manual_seed(0)
        model.aux['netF'] = standins.StandinFlowNet().to(dev)
        model.aux['modnet'] = standins.StandinMatteNet().to(dev)
    out = {}
    for encoder in ('host', 'device'):
        torch.manual_seed(7)                                          # --allow_random_init: the same weights in both runs
        argv = ['--model', 'geomcgt_ifw_test', '--netG', 'resnet_9blocks_rcatland32_full_ifw', '--netg_resb_div', '3',
                '--netg_resb_disp', '3', '--output_nc', '1', '--ngf', '8', '--dataset_mode', 'umlvdfw_test', '--dataroot', tf.NAME,
                '--list_dir', str(work / 'lists'), '--draw_op', '1', '--lmark_lookup', tf.LOOKUP, '--batch_size', '2', '--gpu_ids', '0',
                '--allow_random_init', '--name', 'run', '--checkpoints_dir', str(tmp_path / 'ck'),
                '--results_dir', str(tmp_path / encoder), '--save_format', 'png', '--png_encoder', encoder]
        entry.main(argv, prepare_model=prepare)
        out[encoder] = tmp_path / encoder / 'run' / 'test_latest' / 'images'
    listed = sorted(os.listdir(out['host']))
    assert len(listed) == 27 and sorted(os.listdir(out['device'])) == listed
    for name in listed:
        host = np.asarray(Image.open(out['host'] / name))
        pf.check_both(open(out['device'] / name, 'rb').read(), host)
