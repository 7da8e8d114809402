"""The umlvd_ifw data layer on the MI355X: apd_image_prep_u8 bit-exact against the PIL restatement (pil_reference.py, held
against PIL itself in test_dataset_cpu.py), a device-prepared batch against the reference's golden items, and one training
step fed by the dataset."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dataset_fixture as fx          # noqa: E402
import pil_reference as pr            # noqa: E402
from conftest import linf             # noqa: E402
from test_dataset_cpu import hard_image, IMAGE_KEYS, MASK_KEYS      # noqa: E402

pytestmark = pytest.mark.gpu
GUARD, SENTINEL = 4096, -7777.0


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    return torch.device('cuda:0')


def _launch(dev, src, params, load_h, load_w, crop, gray, kind, spoil=None):
    """apd_image_prep_u8 through ctypes into a NaN-filled window between sentinel guards: (rc, window, guards intact)"""
    from animateportrait_amd import _dataapi as D
    from animateportrait_amd.data import image_prep
    n, hs, ws, c = src.shape
    oc = 3 if (c == 3 and not gray) else 1
    params = np.asarray(params, dtype=np.int32).reshape(n, 3)
    d = image_prep.describe(n, hs, ws, c, load_w, load_h, crop, gray, int(params[:, 0].max()), int(params[:, 1].max()))
    for k, v in (spoil or {}).items():
        setattr(d, k, v)
    count = n * oc * crop * crop
    buf = torch.full((count + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    buf[GUARD:GUARD + count] = float('nan')
    th, tv = image_prep._table_on(dev, ws, load_w), image_prep._table_on(dev, hs, load_h)
    keep = [torch.from_numpy(src).to(dev).contiguous(), torch.from_numpy(params).to(dev), image_prep._lut_on(dev, kind)]

    def p(t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None else None
    rc = D.lib().apd_image_prep_u8(ctypes.byref(d), p(keep[0]), p(keep[1]), p(th[0] if th else None), p(th[1] if th else None),
                                   p(tv[0] if tv else None), p(tv[1] if tv else None), p(keep[2]),
                                   ctypes.c_void_p(buf.data_ptr() + 4 * GUARD),
                                   ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize(dev)
    guards = bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + count:] == SENTINEL).all())
    return rc, buf[GUARD:GUARD + count].view(n, oc, crop, crop), guards


def _expected(src, params, load_h, load_w, crop, gray, kind):
    from animateportrait_amd.data import image_prep
    u8 = np.stack([pr.transform_u8(a, int(q[0]), int(q[1]), int(q[2]), load_h, load_w, crop, gray) for a, q in zip(src, params)])
    return image_prep.lut(kind)[torch.from_numpy(u8).long()]


# Hs, Ws, C, load_h, load_w, crop, [(x, y, flip) per image], to_gray, lut
CASES = {
    'down2_512_full': (512, 512, 3, 256, 256, 256, [(0, 0, 0)], False, 'image'),
    'crop64_offsets_flipmix': (80, 96, 3, 72, 72, 64, [(0, 0, 0), (8, 8, 1), (3, 5, 0), (8, 0, 1), (0, 8, 0)], False, 'image'),
    'crop64_c1_mask': (80, 96, 1, 72, 72, 64, [(0, 0, 1), (8, 8, 0), (3, 5, 1)], False, 'mask'),
    'crop64_gray': (80, 96, 3, 72, 72, 64, [(3, 5, 0), (8, 8, 1)], True, 'image'),
    'up_286_crop_at_both_edges': (50, 70, 1, 286, 286, 256, [(30, 30, 0), (30, 30, 1)], False, 'image'),
    'same_size_no_pass': (64, 64, 3, 64, 64, 64, [(0, 0, 0), (0, 0, 1)], False, 'image'),
    'vertical_pass_skipped': (64, 96, 3, 64, 64, 61, [(3, 2, 0), (0, 3, 1)], False, 'image'),
    'horizontal_pass_skipped': (96, 64, 1, 64, 64, 64, [(0, 0, 1)], True, 'mask'),
    'crop67_ragged': (80, 96, 3, 72, 72, 67, [(5, 5, 0), (0, 3, 1)], False, 'image'),
    'load_not_square': (97, 33, 3, 40, 56, 40, [(16, 0, 1), (0, 0, 0)], True, 'image'),
    'dataset_size_300x280': (300, 280, 3, 286, 286, 256, [(17, 30, 1)], False, 'image'),
}


@pytest.mark.parametrize('name', sorted(CASES))
def test_image_prep_is_bit_exact(dev, name):
    hs, ws, c, load_h, load_w, crop, params, gray, kind = CASES[name]
    rng = np.random.RandomState(len(name) * 31 + hs)
    src = np.stack([hard_image(rng, hs, ws, c) for _ in params])
    want = _expected(src if c == 3 else src[..., 0], params, load_h, load_w, crop, gray, kind)
    rc, got, guards = _launch(dev, src, params, load_h, load_w, crop, gray, kind)
    assert rc == 0 and guards
    assert got.shape == want.shape and torch.equal(got.cpu(), want), float((got.cpu() - want).abs().max())
    if (hs, ws) != (load_h, load_w) and name != 'down2_512_full':          # (halving averages the checker away)
        assert float(want.min()) == float(_lut(kind)[0]) and float(want.max()) == float(_lut(kind)[255])    # both clip points occur


def _lut(kind):
    from animateportrait_amd.data import image_prep
    return image_prep.lut(kind)


def test_refused_shapes_write_nothing(dev):
    from animateportrait_amd import _dataapi as D
    src = np.stack([hard_image(np.random.RandomState(1), 80, 96, 3)])
    for spoil in (dict(crop=73), dict(max_x=9), dict(kh=0), dict(kv=9), dict(C=2), dict(load_w=0)):
        rc, win, guards = _launch(dev, src, [(0, 0, 0)], 72, 72, 64, False, 'image', spoil)
        assert rc < 0 and guards and bool(torch.isnan(win).all()), spoil
        assert 'image_prep' in D.last_error()


def test_prep_device_wrapper_equals_host(dev):
    """the product's two legs on the same decoded arrays: prep_device (one launch) == prep_host (PIL)"""
    from animateportrait_amd.data import image_prep
    rng = np.random.RandomState(9)
    arrs = [hard_image(rng, 120, 100, 3) for _ in range(4)]
    params = [(0, 30, 0), (30, 0, 1), (11, 7, 1), (2, 3, 0)]
    for gray, kind in ((False, 'image'), (True, 'mask')):
        got = image_prep.prep_device(torch.from_numpy(np.stack(arrs)).to(dev), params, 286, 256, gray, kind)
        assert torch.equal(got.cpu(), image_prep.prep_host(arrs, params, 286, 256, gray, kind))


# ------------------------------------------------------------------------------------------------ a batch against the golden
@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    work = tmp_path_factory.mktemp('umlvd_gpu')
    root, lists = str(work / 'tree'), str(work / 'lists')
    fx.write_tree(root, lists)
    return root, lists


def test_device_batch_equals_the_reference_items(dev, tree, golden):
    """Images and the drawn target exact; landmarks and windows exact; motion grids to the bar of the motion-grid golden test
    (2e-5, test_delaunay_gpu.py); the static warps against an fp64 evaluation of grid_sample on the same inputs, within
    4 e_ref + 1e-6 where e_ref is the distance of the fp32 evaluation from it, and against the reference's recorded warps within
    what the 2e-5 between the two motion maps can move a bilinear sample."""
    from animateportrait_amd.data import find_dataset_using_name, image_prep
    gd = golden('dataset.npz')
    ds = find_dataset_using_name('umlvd_ifw')(fx.options(tree[1]))
    plans = []
    for s in range(3):
        random.seed(int(gd['seeds'][s]))
        torch.manual_seed(int(gd['seeds'][s]))
        plans.append(ds.plan_sample(int(gd['indices'][s])))
    item = ds.make_batch(plans, mode='device')
    torch.cuda.synchronize(dev)
    luts = {'image': image_prep.lut('image'), 'mask': image_prep.lut('mask')}
    step = int(gd['step'])
    for s in range(3):
        for kind, keys in (('image', IMAGE_KEYS + ('tB2_lm',)), ('mask', MASK_KEYS)):
            for k in keys:
                want = luts[kind][torch.from_numpy(gd['%s_u8_%d' % (k, s)]).long()]
                assert item[k].is_cuda and torch.equal(item[k][s].cpu(), want), (s, k)
        for k in ('A_lm_68', 'B_lm_68', 'tA_lm_68', 'tB_lm_68', 'tB2_lm_68', 'B1_lm_68', 'B2_lm_68'):
            assert torch.equal(item[k][s].cpu(), gd['%s_%d' % (k, s)]), (s, k)
        for k in ('winA', 'winBr', 'winB', 'winB2', 'winBr1', 'winBr2'):
            assert item[k][s].tolist() == gd['%s_%d' % (k, s)].tolist(), (s, k)
        for k in ('warp_motion', 'warp_motion2'):
            err = linf(item[k][s][::step, ::step], gd['%s_%d' % (k, s)])
            print('sample %d %s: |device - reference| = %.3e' % (s, k, err))
            assert item[k].shape == (3, 256, 256, 2) and err < 2e-5, (s, k, err)
    a = item['A'].cpu()
    for k, m in (('realA_static_warp', 'warp_motion'), ('realA_static_warp2', 'warp_motion2')):
        grid = item[m].cpu()
        ref64 = torch.nn.functional.grid_sample(a.double(), grid.double(), align_corners=True)
        ref32 = torch.nn.functional.grid_sample(a, grid, align_corners=True)
        e_ref = float((ref32.double() - ref64).abs().max())
        err = float((item[k].cpu().double() - ref64).abs().max())
        far = max(linf(item[k][s][:, ::step, ::step], gd['%s_%d' % (k, s)]) for s in range(3))
        # the reference's item samples the same image through its own griddata map.  The maps agree within 2e-5 (asserted above
        # at these pixels), that is 2e-5 * 127.5 pixels per axis; a bilinear sample moves by at most the largest difference of
        # neighbouring pixels per pixel of displacement and axis; and the reference's own fp32 sampling is e_ref from exact.
        step_max = max(float((a[..., 1:, :] - a[..., :-1, :]).abs().max()), float((a[..., :, 1:] - a[..., :, :-1]).abs().max()))
        far_bar = 2 * (2e-5 * 127.5) * step_max + (4 * e_ref + 1e-6) + e_ref
        print('%s: e_ref = %.3e  |kernel - ref64| = %.3e  |kernel - reference item| (its own griddata map) = %.3e, bar %.3e'
              % (k, e_ref, err, far, far_bar))
        assert item[k].shape == (3, 3, 256, 256) and err <= 4 * e_ref + 1e-6, (k, err, e_ref)
        assert far <= far_bar, (k, far, far_bar)
    assert item['A_paths'] == [p['A_path'] for p in plans] and len(item['image_paths']) == 3


def test_one_training_step_fed_by_the_dataset(dev, tree):
    from animateportrait_amd import networks as N, standins
    from animateportrait_amd.data import create_dataset
    from animateportrait_amd.models import create_model
    from animateportrait_amd.options.base_options import TrainOptions
    argv = ['--model', 'geomgm_ifw_fore', '--netG', 'resnet_9blocks_rcatland32_full_ifw', '--dataset_mode', 'umlvd_ifw',
            '--dataroot', fx.NAME, '--list_dir', tree[1], '--output_nc', '1', '--ngf', '8', '--ndf', '8', '--netg_resb_div', '3',
            '--netg_resb_disp', '3', '--batch_size', '2', '--gpu_ids', '0']
    opt = TrainOptions().parse(argv)
    assert opt.data_prep == 'device'
    random.seed(2)               # first batch: one target drawn from landmarks, one taken from a clip
    torch.manual_seed(2)
    batch = next(iter(create_dataset(opt)))
    model = create_model(opt)
    model.aux['landmarks'] = standins.StandinLandmarkNet().to(dev)
    model.aux['faceloss'] = N.FaceLoss(standins.StandinFaceNet().to(dev))
    model.aux['netF'] = standins.StandinFlowNet().to(dev)
    model.aux['modnet'] = standins.StandinMatteNet().to(dev)
    before = [p.detach().clone() for p in model.netG_A.parameters()] + [p.detach().clone() for p in model.netD_A.parameters()]
    model.set_input(batch)
    model.optimize_parameters()
    torch.cuda.synchronize(dev)
    losses = model.get_current_losses()
    assert losses and all(np.isfinite(float(v)) for v in losses.values()), losses
    after = list(model.netG_A.parameters()) + list(model.netD_A.parameters())
    assert all(bool(torch.isfinite(p).all()) for p in after)
    assert sum(int(not torch.equal(b, p.detach())) for b, p in zip(before, after)) > len(before) // 2
