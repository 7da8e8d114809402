"""The umlvd_ifw dataset without a device: registry, the PIL restatement against PIL, the coefficient tables, the random
decisions and landmarks against the reference's golden items (tests/golden/make_dataset_golden.py), the host image path,
and the refusals of libapdata.so."""
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

SHAPES = [(80, 96, 72, 72), (512, 512, 256, 256), (64, 64, 64, 64), (50, 70, 286, 286), (97, 33, 40, 56), (512, 512, 286, 286)]
IMAGE_KEYS = ('A', 'B', 'A_lm', 'B_lm', 'tA_lm', 'tB_lm', 'B1', 'B2', 'B3', 'B4', 'fakeB_static')
MASK_KEYS = tuple(p + '_mask' + s for p in ('A', 'Br', 'B', 'B2') for s in ('', 'e', 'l'))


def hard_image(rng, h, w, c):
    """noise plus a 0/255 checkerboard: the negative lobes of the kernel reach both clip points"""
    a = rng.randint(0, 256, (h, w, c)).astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    cb = (((yy // 3 + xx // 3) % 2) * 255).astype(np.uint8)
    a[h // 4:h // 2] = cb[h // 4:h // 2, :, None]
    return a


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    work = tmp_path_factory.mktemp('umlvd')
    root, lists = str(work / 'tree'), str(work / 'lists')
    fx.write_tree(root, lists)
    return root, lists


@pytest.fixture(scope='module')
def planned(tree, golden):
    """the dataset on the fixture tree and the plans of the three golden samples"""
    from animateportrait_amd.data import find_dataset_using_name
    root, lists = tree
    gd = golden('dataset.npz')
    ds = find_dataset_using_name('umlvd_ifw')(fx.options(lists))
    plans = []
    for s in range(3):
        random.seed(int(gd['seeds'][s]))
        torch.manual_seed(int(gd['seeds'][s]))
        plans.append(ds.plan_sample(int(gd['indices'][s])))
    return ds, plans, root


def test_registry_knows_umlvd_ifw():
    from animateportrait_amd import data
    cls = data.find_dataset_using_name('umlvd_ifw')
    assert cls.__name__ == 'UMLVDIFWDataset'
    import argparse
    p = data.get_option_setter('umlvd_ifw')(argparse.ArgumentParser(), True)
    o = p.parse_args([])
    assert o.data_prep in ('device', 'host') and o.list_dir == 'datasets/list' and o.cache_decoded is False
    with pytest.raises(NotImplementedError):
        data.find_dataset_using_name('no_such_dataset')


@pytest.mark.parametrize('h,w,oh,ow', SHAPES)
def test_pil_reference_equals_pil(h, w, oh, ow):
    from PIL import Image
    rng = np.random.RandomState(h * 7 + ow)
    for c in (1, 3):
        a = hard_image(rng, h, w, c)
        a = a[..., 0] if c == 1 else a
        ref = np.asarray(Image.fromarray(a).resize((ow, oh), Image.BICUBIC))
        got = pr.resize(a, oh, ow)
        assert np.array_equal(got, ref), int(np.abs(got.astype(int) - ref).max())


def test_gray_rule_equals_pil():
    from PIL import Image
    a = np.random.RandomState(3).randint(0, 256, (64, 96, 3)).astype(np.uint8)
    a[0, :6] = [[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [254, 255, 255]]
    assert np.array_equal(pr.to_gray(a), np.asarray(Image.fromarray(a).convert('L')))


def test_product_tables_equal_the_restatement():
    from animateportrait_amd.data import image_prep
    sizes = {(i, o) for h, w, oh, ow in SHAPES for i, o in ((h, oh), (w, ow))} | {(300, 286), (280, 286), (100, 286), (4000, 286)}
    for i, o in sorted(sizes):
        tab = image_prep.resample_table(i, o)
        if i == o:
            assert tab is None
            continue
        b, w, k = pr.coeffs(i, o)
        assert tab[2] == k and np.array_equal(tab[0], b) and np.array_equal(tab[1], w), (i, o)
        assert tab[0].dtype == np.int32 and tab[1].dtype == np.int32
    lut = image_prep.lut('image')
    v = torch.arange(256, dtype=torch.float32)
    assert torch.equal(lut, (v / 255 - 0.5) / 0.5) and torch.equal(image_prep.lut('mask'), v / 255)


def test_plan_sample_equals_the_reference(planned, golden):
    ds, plans, root = planned
    gd = golden('dataset.npz')
    assert sorted(int(gd['branch_%d' % s]) for s in range(3)) == [0, 1, 2]
    for s, p in enumerate(plans):
        assert [os.path.relpath(p[k], root) for k in ('A_path', 'B_path', 'B1_path', 'B2_path')] == gd['paths_%d' % s].tolist()
        assert p['image_paths'] == str(gd['image_paths_%d' % s])
        got = [(int(q[0]), int(q[1]), int(q[2])) for q in (p['pA'], p['pB'], p['pB1'])]
        assert got == [tuple(r) for r in gd['params_%d' % s].tolist()], s
        assert p['branch'] == int(gd['branch_%d' % s])
        for k in ('A_lm_68', 'B_lm_68', 'B1_lm_68', 'B2_lm_68', 'tB_lm_68', 'tB2_lm_68'):       # tB2 carries the offsets
            assert p[k].dtype == torch.float32 and torch.equal(p[k], gd['%s_%d' % (k, s)]), (s, k)
        for k in ('winA', 'winBr', 'winBr1', 'winBr2', 'winB', 'winB2'):
            assert p[k].tolist() == gd['%s_%d' % (k, s)].tolist(), (s, k)


def test_host_item_images_equal_the_reference(planned, golden):
    from animateportrait_amd.data import image_prep
    ds, plans, _ = planned
    gd = golden('dataset.npz')
    item = ds.image_tensors(plans, mode='host')
    luts = {'image': image_prep.lut('image'), 'mask': image_prep.lut('mask')}
    checked = 0
    for s, p in enumerate(plans):
        for kind, keys in (('image', IMAGE_KEYS + (('tB2_lm',) if p['branch'] == 0 else ())), ('mask', MASK_KEYS)):
            for k in keys:
                want = luts[kind][torch.from_numpy(gd['%s_u8_%d' % (k, s)]).long()]
                assert item[k].dtype == torch.float32 and torch.equal(item[k][s], want), (s, k)
                checked += 1
    assert checked == 3 * (len(IMAGE_KEYS) + len(MASK_KEYS)) + 1
    assert item['A'].shape == (3, 3, 256, 256) and item['B'].shape == (3, 1, 256, 256)


def test_warp_loss_1_is_refused(tree):
    from animateportrait_amd.data import find_dataset_using_name
    with pytest.raises(NotImplementedError, match='warp_loss 1'):
        find_dataset_using_name('umlvd_ifw')(fx.options(tree[1], warp_loss=1))


def test_apd_refuses_without_a_device():
    """null pointers and descriptions outside the served region: refused before anything touches a device"""
    from animateportrait_amd import _dataapi as D
    from animateportrait_amd.data.image_prep import describe
    lib = D.lib()
    assert lib.apd_abi_version() == D.ABI_VERSION == 1
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'animateportrait_data.h')).read()
    assert '#define APD_ABI_VERSION 1' in header and all(name + '(' in header for name in D.SIGNATURES)
    good = describe(2, 80, 96, 3, 72, 72, 64, False, 8, 8)
    assert lib.apd_image_prep_ok(ctypes.byref(good)) == 1
    assert lib.apd_image_prep_ok(None) == 0
    one = ctypes.c_void_p(16)                 # never dereferenced: every call below is refused first
    assert lib.apd_image_prep_u8(None, *([one] * 8), None) < 0
    for hole in range(8):                     # src, params, the four tables, lut, out: each in turn missing
        args = [one] * 8
        args[hole] = None
        assert lib.apd_image_prep_u8(ctypes.byref(good), *args, None) < 0, hole
        assert 'image_prep' in D.last_error() and 'launch' not in D.last_error()
    bad = [dict(C=2), dict(C=4), dict(N=0), dict(N=D.MAX_IMAGES + 1), dict(Hs=0), dict(Ws=D.MAX_SOURCE + 1), dict(load_w=0),
           dict(load_h=D.MAX_LOAD + 1), dict(crop=0), dict(crop=73), dict(max_x=9), dict(max_y=9), dict(max_x=-1),
           dict(kh=0), dict(kv=5), dict(kh=64)]
    for change in bad:
        d = describe(2, 80, 96, 3, 72, 72, 64, False, 8, 8)
        for k, v in change.items():
            setattr(d, k, v)
        assert lib.apd_image_prep_ok(ctypes.byref(d)) == 0, change
        assert lib.apd_image_prep_u8(ctypes.byref(d), *([one] * 8), None) < 0 and 'launch' not in D.last_error(), change
    many = describe(1, 8192, 8192, 1, 100, 100, 64, False)         # 2 * ceil(2 * 81.92) + 1 taps
    assert many.kh > D.MAX_TAPS and lib.apd_image_prep_ok(ctypes.byref(many)) == 0 and 'taps' in D.last_error()


@pytest.mark.parametrize('length,world,batch', [(5, 2, 2), (1025, 8, 16), (3, 2, 2), (7, 3, 1), (64, 4, 4), (9, 1, 4), (3, 3, 16)])
def test_every_rank_runs_the_same_batches_per_epoch(tree, length, world, batch):
    """each training step is a collective: the ranks of a data-parallel run must see the same number of batches, of the same
    sizes, from one shared order, whatever their own ``random`` state; the shards are disjoint"""
    from animateportrait_amd.data.umlvd_ifw_dataset import UMLVDIFWDataset
    per_rank = []
    for rank in range(world):
        ds = UMLVDIFWDataset(fx.options(tree[1], batch_size=batch, rank=rank, world_size=world))
        ds.A_paths, ds.A_size = [ds.A_paths[i % 3] for i in range(length)], length          # an epoch of ``length`` indices
        random.seed(100 + rank)                                                              # the ranks' own states differ
        per_rank.append([ds.batches(epoch=0), ds.batches(epoch=1)])
    for e in range(2):
        shapes = [[len(b) for b in r[e]] for r in per_rank]
        assert all(s == shapes[0] for s in shapes) and shapes[0], (e, shapes)
        seen = [i for r in per_rank for b in r[e] for i in b]
        assert len(seen) == len(set(seen)) and set(seen) <= set(range(length))
        assert len(seen) >= length - (world * batch - 1) or len(seen) == (length // world) * world
    if length > 3:
        assert [r[0] for r in per_rank] != [r[1] for r in per_rank]                          # the epochs differ
    serial = UMLVDIFWDataset(fx.options(tree[1], batch_size=batch, rank=0, world_size=world, serial_batches=True))
    serial.A_paths, serial.A_size = [serial.A_paths[i % 3] for i in range(length)], length
    assert [i for b in serial.batches() for i in b] == sorted(i for b in serial.batches() for i in b)
    with pytest.raises(RuntimeError, match='ranks'):
        UMLVDIFWDataset(fx.options(tree[1], rank=0, world_size=4)).batches()                 # 3 samples, 4 ranks


def test_iterating_advances_the_epoch(tree):
    from animateportrait_amd.data.umlvd_ifw_dataset import UMLVDIFWDataset
    ds = UMLVDIFWDataset(fx.options(tree[1], batch_size=1))
    ds.make_batch = lambda plans, mode=None: [p['index'] for p in plans]                     # no device here
    first, second = [b[0] for b in ds], [b[0] for b in ds]
    assert sorted(first) == sorted(second) == [0, 1, 2] and ds.epoch == 2
    assert first == [b[0] for b in ds.batches(epoch=0)] and second == [b[0] for b in ds.batches(epoch=1)]


def test_max_offset_above_3_moves_the_second_masks(tree):
    """--max_offset 5: the branch with transform_mask, restated here per sample from the reference (umlvd_ifw_dataset.py:
    321-371), including its slip in the photo branch: B2_mask ends as the moved LIP mask, B2_maske / B2_maskl stay unmoved."""
    import torch.nn.functional as F
    from animateportrait_amd.data.umlvd_ifw_dataset import UMLVDIFWDataset
    ds = UMLVDIFWDataset(fx.options(tree[1], max_offset=5))
    plans, seed = {}, 0
    while len(plans) < 3:
        seed += 1
        random.seed(seed)
        torch.manual_seed(seed)
        p = ds.plan_sample(seed % 3)
        plans.setdefault(p['branch'], p)
    plans = [plans[0], plans[1], plans[2]]
    assert plans[0]['dxdy'] is None and all(p['dxdy'] is not None for p in plans[1:])
    for p in plans[1:]:
        off = p['tB2_lm_68'] - p['tB_lm_68']
        assert float((off - off[0]).abs().max()) < 1e-4 and 0 <= float(off.min()) and float(off.max()) <= 5       # one shared offset
        assert float(p['dxdy'][0]) == float(-p['offset'][0, 0] / 256) and float(p['dxdy'][1]) == float(-p['offset'][0, 1] / 256)
    plain = ds.image_tensors(plans, mode='host')
    item = ds.shift_second_masks(dict(plain), plans)

    def moved(mask, p):
        theta = torch.tensor([[1, 0, p['dxdy'][0]], [0, 1, p['dxdy'][1]]], dtype=torch.float)
        grid = F.affine_grid(theta.unsqueeze(0), mask.unsqueeze(0).size(), align_corners=False)
        return F.grid_sample(mask.unsqueeze(0), grid, align_corners=False)[0]
    for suf in ('', 'e', 'l'):
        assert torch.equal(item['B2_mask' + suf][0], plain['B2_mask' + suf][0])                         # clip branch: untouched
        assert torch.equal(item['B2_mask' + suf][1], moved(plain['Br_mask' + suf][1], plans[1]))         # drawing branch
        assert not torch.equal(item['B2_mask' + suf][1], plain['Br_mask' + suf][1])
        assert torch.equal(item['B_mask' + suf], plain['B_mask' + suf])
    assert torch.equal(item['B2_mask'][2], moved(plain['A_maskl'][2], plans[2]))                         # photo branch: the slip
    assert torch.equal(item['B2_maske'][2], plain['A_maske'][2]) and torch.equal(item['B2_maskl'][2], plain['A_maskl'][2])
    assert torch.equal(plain['B2_mask'][2], plain['A_mask'][2])                                          # the input was not changed
