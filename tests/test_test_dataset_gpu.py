"""umlvdfw_test on the MI355X: apd_landmark_map against draw2 restated on oracle/cv_raster and against the reference's golden
maps, apd_landmark_marks against the host get_lmvis it replaces, apd_frames_to_u8 against end2end.tensor2im, a device-prepared
batch against the reference's golden items, and test.py writing PNGs end to end."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import testset_fixture as tf          # noqa: E402
from conftest import linf             # noqa: E402

pytestmark = pytest.mark.gpu
GUARD, SENTINEL = 4096, -7777.0
CASES = tf.raster_cases()


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    work = tmp_path_factory.mktemp('umlvdfw_gpu')
    root, lists = str(work / 'tree'), str(work / 'lists')
    tf.write_test_tree(root, lists)
    return root, lists


def _ptr(t, offset=0):
    return ctypes.c_void_p(t.data_ptr() + offset)


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


# ------------------------------------------------------------------------------------------------ apd_landmark_map
def _map_guarded(dev, lm, seg, h, w, radius, thickness, op):
    """apd_landmark_map through ctypes into a NaN-filled window between sentinel guards: (rc, maps (N, h, w), guards intact)"""
    from animateportrait_amd import _dataapi as D
    lm = torch.as_tensor(lm, dtype=torch.float32).to(dev).contiguous()
    n, p, _ = lm.shape
    seg = np.ascontiguousarray(seg, np.int32)
    s = len(seg)
    seg_dev = torch.from_numpy(seg).to(dev) if s else None
    count = n * h * w
    buf = torch.full((count + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    buf[GUARD:GUARD + count] = float('nan')
    rc = D.lib().apd_landmark_map(_ptr(lm), _ptr(seg_dev) if s else None, seg.ctypes.data_as(ctypes.c_void_p) if s else None, n, p, s,
                                  h, w, radius, thickness, op, -1.0, 1.0, _ptr(buf, 4 * GUARD), _stream(dev))
    torch.cuda.synchronize(dev)
    guards = bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + count:] == SENTINEL).all())
    return rc, buf[GUARD:GUARD + count].view(n, h, w).cpu(), guards


def test_discs_equal_ap_landmark_discs(dev):
    from animateportrait_amd import losses
    from animateportrait_amd.data import visuals
    g = torch.Generator().manual_seed(4)
    lm = torch.rand((3, 68, 2), generator=g) * 300 - 20               # some points outside the 256 x 256 image
    lm[0, :4] = torch.tensor([[10.5, 11.5], [12.5, 13.5], [0.0, 0.0], [255.0, 255.0]])
    lm = lm.to(dev)
    for radius in (3, 5, 0, 31):
        want = losses.landmark_discs(lm, 256, 256, radius=radius)
        got = visuals.landmark_map(lm, np.load(tf.LOOKUP), 256, 256, radius, 2, op=0)          # op 0: the table is not read
        assert got.shape == (3, 1, 256, 256) and torch.equal(got, want), radius
    assert torch.equal(visuals.landmark_map(lm, None, 256, 256, 3, 2, op=0, lo=0.0, hi=0.5), losses.landmark_discs(lm, 256, 256, 3, 0.0, 0.5))


@pytest.mark.parametrize('name', sorted(CASES))
def test_contour_map_equals_cv_raster(dev, name):
    """op 1 == fill_circle + thick_line in numpy, bit for bit; a second sample (the same points moved) shares the launch"""
    h, w, lm, seg, radius, thickness = CASES[name]
    batch = np.stack([lm, lm + np.array([3.0, -2.0], np.float32)])
    rc, got, guards = _map_guarded(dev, batch, seg, h, w, radius, thickness, 1)
    assert rc == 0 and guards
    for i in range(2):
        want = tf.draw2_reference(batch[i], seg, h, w, radius, thickness, 1)
        assert set(np.unique(got[i].numpy()).tolist()) <= {-1.0, 1.0}
        diff = int(((got[i].numpy() > 0) != (want > 0)).sum())
        assert diff == 0, (name, i, diff)
    if name.startswith('ragged'):
        lands = np.round(lm).astype(int)
        assert lands[0].tolist() == [2, 4] and lands[1].tolist() == [12, 12]           # the ties went to even
        outside = tf.draw2_reference(lm[[5, 6]], [(0, 1)], h, w, radius, thickness, 1)
        assert not outside.any()                                                           # the segment wholly outside draws nothing
        rc, only, guards = _map_guarded(dev, lm[None, [5, 6]], [(0, 1)], h, w, radius, thickness, 1)
        assert rc == 0 and guards and bool((only == -1.0).all())


def test_refused_map_writes_nothing(dev):
    from animateportrait_amd import _dataapi as D
    h, w, lm, seg, radius, thickness = CASES['square32_t2']
    for kw in (dict(radius=32), dict(thickness=17), dict(seg=np.array([(0, 6)], np.int32)), dict(seg=np.zeros((129, 2), np.int32))):
        args = dict(seg=seg, radius=radius, thickness=thickness)
        args.update(kw)
        rc, win, guards = _map_guarded(dev, lm[None], args['seg'], h, w, args['radius'], args['thickness'], 1)
        assert rc < 0 and guards and bool(torch.isnan(win).all()) and 'landmark_map' in D.last_error(), kw


def test_table_maps_equal_the_reference_items(dev, golden):
    """256 x 256 with the 64-segment table: the A_lm / tB_lm the reference's draw2 produced for the golden items"""
    from animateportrait_amd.data import visuals
    gd = golden('test_dataset.npz')
    seg = np.load(tf.LOOKUP)
    for s, (_, draw_op, _, _) in enumerate(tf.ITEMS):
        lm = torch.stack([gd['A_lm_68_%d' % s], gd['tB_lm_68_%d' % s]]).to(dev)
        got = visuals.landmark_map(lm, seg, 256, 256, 3, 2, op=draw_op).cpu()
        for i, k in enumerate(('A_lm', 'tB_lm')):
            want = torch.from_numpy(gd['%s_u8_%d' % (k, s)]).float() / 255. * 2 - 1
            assert torch.equal(got[i], want), (s, k, int((got[i] != want).sum()))
        assert np.array_equal(gd['B_lm_u8_%d' % s], gd['tB_lm_u8_%d' % s])


# ------------------------------------------------------------------------------------------------ apd_landmark_marks
def _host_lmvis(tensor_im, lm, win, hradius=3):
    """get_lmvis as the model ran it on the host before apd_landmark_marks (sample 0's marks on every sample)"""
    vis = tensor_im.detach().clone()
    if vis.shape[1] == 1:
        vis = vis.repeat(1, 3, 1, 1)
    pts = lm.detach().cpu().numpy()
    win = win.cpu().numpy() if torch.is_tensor(win) else win

    def mark(y0, y1, x0, x1):
        vis[:, 0, y0:y1, x0:x1] = 1
        vis[:, 1:, y0:y1, x0:x1] = -1
    for k in range(lm.shape[1]):
        x, y = int(round(float(pts[0, k, 0]))), int(round(float(pts[0, k, 1])))
        mark(y - hradius, y + hradius, x - hradius, x + hradius)
    x1, x2, y1, y2 = (int(win[0][i]) for i in range(4))
    mark(y1 - hradius, y1 + hradius, x1 - hradius, x2 + hradius)
    mark(y2 - hradius, y2 + hradius, x1 - hradius, x2 + hradius)
    mark(y1 - hradius, y2 + hradius, x1 - hradius, x1 + hradius)
    mark(y1 - hradius, y2 + hradius, x2 - hradius, x2 + hradius)
    return vis


def _marks_inputs(n, c, h=48, w=40, p=10, seed=0):
    g = torch.Generator().manual_seed(seed)
    frames = torch.rand((n, c, h, w), generator=g) * 1.6 - 0.8
    lm = torch.stack([torch.rand((n, p), generator=g) * (w - 7) + 3, torch.rand((n, p), generator=g) * (h - 7) + 3], 2)
    lm[:, 0] = torch.tensor([4.5, 5.5])                                   # ties: 4.5 -> 4, 5.5 -> 6
    win = torch.tensor([[8 + i, 30 + i, 10 + 2 * i, 40 + i] for i in range(n)], dtype=torch.int32)
    return frames, lm, win


@pytest.mark.parametrize('c', [1, 3])
def test_marks_equal_the_host_get_lmvis(dev, c):
    from animateportrait_amd.data import visuals
    frames, lm, win = _marks_inputs(3, c)
    batch = visuals.landmark_marks(frames.to(dev), lm.to(dev), win).cpu()
    assert batch.shape == (3, 3, 48, 40)
    for i in range(3):
        one = visuals.landmark_marks(frames[i:i + 1].to(dev), lm[i:i + 1].to(dev), win[i:i + 1]).cpu()
        assert torch.equal(one, _host_lmvis(frames[i:i + 1], lm[i:i + 1], win[i:i + 1])), i      # N = 1: the old tensor
        assert torch.equal(batch[i], one[0]), i                                                  # every sample its own marks
    assert not torch.equal(batch[1], _host_lmvis(frames, lm, win)[1])                            # (the old loop reused sample 0's)


def test_marks_are_clipped_at_the_corners(dev):
    from animateportrait_amd import _dataapi as D
    h, w, p = 48, 40, 4
    frames = torch.zeros((1, 1, h, w)).uniform_(-0.5, 0.5)
    lm = torch.tensor([[[0.0, 0.0], [39.6, 47.2], [-5.0, 20.0], [100.0, 100.0]]])
    win = torch.tensor([[-2, 41, -1, 50]], dtype=torch.int32)
    count = 3 * h * w
    buf = torch.full((3 * count,), SENTINEL, dtype=torch.float32, device=dev)      # a guard frame before and after the output
    f, l, wn = frames.to(dev), lm.to(dev), win.to(dev)
    rc = D.lib().apd_landmark_marks(_ptr(f), _ptr(l), _ptr(wn), 1, 1, p, h, w, 3, _ptr(buf, 4 * count), _stream(dev))
    torch.cuda.synchronize(dev)
    assert rc == 0 and bool((buf[:count] == SENTINEL).all()) and bool((buf[2 * count:] == SENTINEL).all())
    hit = np.zeros((h, w), bool)

    def mark(y0, y1, x0, x1):
        hit[max(y0, 0):max(min(y1, h), 0), max(x0, 0):max(min(x1, w), 0)] = True
    for x, y in np.round(lm[0].numpy()).astype(int):
        mark(y - 3, y + 3, x - 3, x + 3)
    x1, x2, y1, y2 = win[0].tolist()
    mark(y1 - 3, y1 + 3, x1 - 3, x2 + 3)
    mark(y2 - 3, y2 + 3, x1 - 3, x2 + 3)
    mark(y1 - 3, y2 + 3, x1 - 3, x1 + 3)
    mark(y1 - 3, y2 + 3, x2 - 3, x2 + 3)
    want = frames[0].repeat(3, 1, 1).clone()
    want[0][torch.from_numpy(hit)] = 1
    want[1:, torch.from_numpy(hit)] = -1
    assert hit[:3, :3].all() and hit[44:, 37:].all() and not hit[10:40, 10:30].any()
    assert torch.equal(buf[count:2 * count].view(3, h, w).cpu(), want)


# ------------------------------------------------------------------------------------------------ apd_frames_to_u8
def _edge_values():
    """-1, 1 and, for every k in 0..255, the float32 values just below, at and just above where (x + 1) / 2 * 255 crosses k"""
    x = (np.arange(256, dtype=np.float64) * 2 / 255 - 1).astype(np.float32)
    lo, hi = np.nextafter(x, np.float32(-2)), np.nextafter(x, np.float32(2))
    return np.clip(np.concatenate([np.array([-1, 1], np.float32), lo, x, hi, np.nextafter(lo, np.float32(-2)), np.nextafter(hi, np.float32(2))]),
                   -1, 1).astype(np.float32)


def _frames(shape, seed):
    rng = np.random.RandomState(seed)
    a = rng.uniform(-1, 1, shape).astype(np.float32)
    edge = _edge_values()
    flat = a.reshape(-1)
    k = min(flat.size, edge.size)
    flat[:k] = rng.permutation(edge)[:k]
    return torch.from_numpy(a)


@pytest.mark.parametrize('shape', [(2, 1, 5, 7), (3, 3, 16, 67), (1, 1, 256, 256)])
def test_frames_to_u8_equals_tensor2im(dev, shape):
    from animateportrait_amd import end2end
    from animateportrait_amd.data import visuals
    frames = _frames(shape, seed=shape[3])
    want = np.stack([end2end.tensor2im(f) for f in frames])
    on_device = visuals.frames_to_u8(frames.to(dev), out='device')
    pinned = visuals.frames_to_u8(frames.to(dev))
    torch.cuda.synchronize(dev)
    assert on_device.is_cuda and pinned.is_pinned() and not pinned.is_cuda
    assert on_device.shape == want.shape and np.array_equal(on_device.cpu().numpy(), want)
    assert np.array_equal(pinned.numpy(), want)
    assert visuals.frames_to_u8(frames.to(dev)).data_ptr() == pinned.data_ptr()         # one buffer per (shape, device), reused
    if shape[3] == 256:
        assert len(np.unique(want)) == 256                                              # every byte value occurs


def test_frames_to_u8_clamps_and_refuses(dev):
    from animateportrait_amd import _dataapi as D
    from animateportrait_amd.data import visuals
    x = torch.tensor([-1.5, 3.0, 1e30, -1e30, float('inf'), float('-inf'), float('nan'), 1.0000001, -1.0000001, 0.0, 1.0, -1.0])
    got = visuals.frames_to_u8(x.view(1, 1, 2, 6).to(dev), out='device').cpu().view(12, 3)
    assert got[:, 0].tolist() == [0, 255, 255, 0, 255, 0, 0, 255, 0, 127, 255, 0] and bool((got == got[:, :1]).all())
    pageable = torch.zeros((1, 2, 6, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match='pinned'):
        visuals.frames_to_u8(x.view(1, 1, 2, 6).to(dev), out=pageable)
    src = x.view(1, 1, 2, 6).to(dev)
    rc = D.lib().apd_frames_to_u8(_ptr(src), 1, 1, 2, 6, _ptr(pageable), _stream(dev))   # the library asks the runtime itself
    assert rc < 0 and 'neither device memory nor pinned' in D.last_error() and not pageable.any()


# ------------------------------------------------------------------------------------------------ the batch
def test_device_batch_equals_the_reference_items(dev, tree, golden):
    """Each golden item was made under its own options (draw_op, --serial_batches, --no_flip), so each sits in a B = 3 batch
    of a dataset with those options, at position s, beside two other items.  A and both landmark maps exact; landmarks and
    window exact; the motion grid to the 2e-5 of tests/test_dataset_gpu.py; the static warp against an fp64 evaluation of
    grid_sample on the same inputs within 4 e_ref + 1e-6, and against the reference's recorded warp within what the 2e-5
    between the two motion maps can move a bilinear sample (the far bar of tests/test_dataset_gpu.py)."""
    from animateportrait_amd.data import find_dataset_using_name, image_prep
    gd = golden('test_dataset.npz')
    lut = image_prep.lut('image')
    step = int(gd['step'])
    for s, (index, draw_op, serial, seed) in enumerate(tf.ITEMS):
        ds = find_dataset_using_name('umlvdfw_test')(tf.options(tree[1], draw_op=draw_op, serial_batches=bool(serial), no_flip=bool(serial)))
        plans = [None] * 3
        for pos in range(3):
            if pos != s:
                plans[pos] = ds.plan_item((index + 1 + pos) % 3)
        random.seed(seed)
        torch.manual_seed(seed)
        plans[s] = ds.plan_item(index)
        item = ds.make_batch(plans, mode='device')
        torch.cuda.synchronize(dev)
        assert set(item) == {'A', 'A_lm', 'B_lm', 'tB_lm', 'A_lm_68', 'tB_lm_68', 'winB', 'realA_static_warp', 'warp_motion', 'A_paths',
                             'B_paths', 'image_paths'}
        for k in ('A', 'A_lm', 'B_lm', 'tB_lm'):
            want = lut[torch.from_numpy(gd['%s_u8_%d' % (k, s)]).long()]
            assert item[k].is_cuda and item[k].shape[0] == 3 and torch.equal(item[k][s].cpu(), want), (s, k)
        for k in ('A_lm_68', 'tB_lm_68'):
            assert torch.equal(item[k][s].cpu(), gd['%s_%d' % (k, s)]), (s, k)
        assert item['winB'][s].tolist() == gd['winB_%d' % s].tolist()
        assert item['image_paths'][s] == str(gd['image_paths_%d' % s])
        err = linf(item['warp_motion'][s][::step, ::step], gd['warp_motion_%d' % s])
        print('item %d warp_motion: |device - reference| = %.3e' % (s, err))
        assert item['warp_motion'].shape == (3, 256, 256, 2) and err < 2e-5, (s, err)
        a, grid = item['A'].cpu(), item['warp_motion'].cpu()
        ref64 = torch.nn.functional.grid_sample(a.double(), grid.double(), align_corners=True)
        ref32 = torch.nn.functional.grid_sample(a, grid, align_corners=True)
        e_ref = float((ref32.double() - ref64).abs().max())
        kerr = float((item['realA_static_warp'].cpu().double() - ref64).abs().max())
        far = linf(item['realA_static_warp'][s][:, ::step, ::step], gd['realA_static_warp_%d' % s])
        step_max = max(float((a[..., 1:, :] - a[..., :-1, :]).abs().max()), float((a[..., :, 1:] - a[..., :, :-1]).abs().max()))
        far_bar = 2 * (2e-5 * 127.5) * step_max + (4 * e_ref + 1e-6) + e_ref
        print('item %d realA_static_warp: e_ref = %.3e  |kernel - ref64| = %.3e  |kernel - reference item| = %.3e, bar %.3e'
              % (s, e_ref, kerr, far, far_bar))
        assert item['realA_static_warp'].shape == (3, 3, 256, 256) and kerr <= 4 * e_ref + 1e-6, (s, kerr, e_ref)
        assert far <= far_bar, (s, far, far_bar)
        if s == 2:                                                     # --data_prep host: the same bits, every key
            host = ds.make_batch(plans, mode='host')
            for k, v in item.items():
                assert (torch.equal(host[k], v) if torch.is_tensor(v) else host[k] == v), k


def test_batches_cover_the_dataset_with_a_short_last_batch(dev, tree):
    from animateportrait_amd.data import create_dataset
    ds = create_dataset(tf.options(tree[1], dataset_mode='umlvdfw_test', batch_size=2, draw_op=1))
    sizes = [(b['A'].shape[0], b['image_paths']) for b in ds]
    assert [n for n, _ in sizes] == [2, 1] and [p for _, ps in sizes for p in ps] == ['p0->p1.png', 'p1->d0.png', 'p2->d1.png']


# ------------------------------------------------------------------------------------------------ end to end
def test_entry_point_writes_the_reference_named_pngs(dev, tree, tmp_path):
    from PIL import Image
    from animateportrait_amd import end2end, standins, test as entry
    kept = []

    def prepare(model):
        model.aux['netF'] = standins.StandinFlowNet().to(dev)
        model.aux['modnet'] = standins.StandinMatteNet().to(dev)
        run = model.test

        def test_and_keep():
            run()
            kept.append((list(model.get_image_paths()), model.fake_B.detach().clone(), list(model.get_current_visuals())))
        model.test = test_and_keep
    argv = ['--model', 'geomcgt_ifw_test', '--netG', 'resnet_9blocks_rcatland32_full_ifw', '--netg_resb_div', '3', '--netg_resb_disp',
            '3', '--output_nc', '1', '--ngf', '8', '--dataset_mode', 'umlvdfw_test', '--dataroot', tf.NAME, '--list_dir', tree[1],
            '--draw_op', '1', '--lmark_lookup', tf.LOOKUP, '--batch_size', '2', '--gpu_ids', '0', '--allow_random_init', '--name', 'run',
            '--checkpoints_dir', str(tmp_path / 'ck'), '--results_dir', str(tmp_path / 'res')]
    entry.main(argv + ['--save_format', 'png'], prepare_model=prepare)
    out = tmp_path / 'res' / 'run' / 'test_latest' / 'images'
    labels = kept[0][2]
    assert labels == ['real_A', 'real_A_lm', 'target_B_lm', 'fake_B', 'fake_B_vis', 'fg_mask', 'fakeB_static', 'fake_B_fore', 'fg_mask1']
    stems = [os.path.splitext(p)[0] for paths, _, _ in kept for p in paths]
    assert stems == ['p0->p1', 'p1->d0', 'p2->d1']
    assert sorted(os.listdir(out)) == sorted('%s_%s.png' % (s, l) for s in stems for l in labels)
    frames = torch.cat([f for _, f, _ in kept])
    for i, s in enumerate(stems):
        png = np.asarray(Image.open(out / ('%s_fake_B.png' % s)))
        assert png.shape == (256, 256, 3) and np.array_equal(png, end2end.tensor2im(frames[i])), s
        vis = np.asarray(Image.open(out / ('%s_fake_B_vis.png' % s)))
        assert (vis != png).any() and ((vis == png).all(2) | (vis == np.array([255, 0, 0], np.uint8)).all(2)).all()
    # the default format: the .npy files of before, and no PNG
    del kept[:]
    entry.main(argv + ['--results_dir', str(tmp_path / 'res_npy')], prepare_model=prepare)
    out = tmp_path / 'res_npy' / 'run' / 'test_latest' / 'images'
    assert sorted(os.listdir(out)) == sorted('%s.png_fake_B.npy' % s for s in stems)
    again = torch.cat([f for _, f, _ in kept])
    for i, s in enumerate(stems):
        assert np.array_equal(np.load(out / ('%s.png_fake_B.npy' % s)), again[i].cpu().numpy())


def test_missing_aux_networks_are_named(dev, tree):
    from animateportrait_amd.data import create_dataset
    from animateportrait_amd.models import create_model
    from animateportrait_amd import standins, test as entry
    opt = entry.parse(['--model', 'geomcgt_ifw_test', '--netG', 'resnet_9blocks_rcatland32_full_ifw', '--output_nc', '1', '--ngf', '8',
                       '--dataroot', tf.NAME, '--list_dir', tree[1], '--batch_size', '1', '--gpu_ids', '0'])
    opt.serial_batches = opt.no_flip = True
    batch = next(iter(create_dataset(opt)))
    model = create_model(opt)
    with pytest.raises(RuntimeError, match='netF'):
        model.set_input(batch)
    model.aux['netF'] = standins.StandinFlowNet().to(dev)
    with pytest.raises(RuntimeError, match='MODNet'):
        model.set_input(batch)
