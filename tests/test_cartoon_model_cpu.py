"""Cartoon training without a device: the option surface and name lists of ``geomgm_ifw_cartoon_fore`` against the reference
class's own (tests/golden/cartoon_model.json), the two registries, and the random decisions, landmarks and host-prepared RGB
frames of ``umlvd_ifw_cartoon`` against the reference's items on the tree tests/cartoon_fixture.py writes
(tests/golden/cartoon_dataset.npz; both made by tests/golden/make_cartoon_golden.py).

A model instance needs the MI355X (BaseModel has no CPU path), so here ``create_model``'s resolution step
(``find_model_using_name``, the call that raised NotImplementedError before this model existed), the parser and the name lists
are checked; tests/test_cartoon_train_gpu.py builds the instance."""
import argparse
import json
import os
import random
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cartoon_fixture as cf          # noqa: E402
from conftest import GOLDEN           # noqa: E402


@pytest.fixture(scope='module')
def ref():
    return json.load(open(os.path.join(GOLDEN, 'cartoon_model.json')))


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    work = tmp_path_factory.mktemp('umlvd_cartoon')
    root, lists = str(work / 'tree'), str(work / 'lists')
    cf.write_tree(root, lists)
    return root, lists


@pytest.fixture(scope='module')
def planned(tree, golden):
    from animateportrait_amd.data import create_dataset
    root, lists = tree
    gd = golden('cartoon_dataset.npz')
    ds = create_dataset(cf.options(lists, dataset_mode='umlvd_ifw_cartoon'))
    plans = []
    for s in range(3):
        random.seed(int(gd['seeds'][s]))
        torch.manual_seed(int(gd['seeds'][s]))
        plans.append(ds.plan_sample(int(gd['indices'][s])))
    return ds, plans, root


def test_both_names_resolve():
    from animateportrait_amd import data, models
    from animateportrait_amd.models.geomgm_ifw_fore_model import GeomGMIFWForeModel
    cls = models.find_model_using_name('geomgm_ifw_cartoon_fore')          # what create_model calls first
    assert cls.__name__ == 'GeomGMIFWCartoonForeModel' and issubclass(cls, GeomGMIFWForeModel)
    assert models.get_option_setter('geomgm_ifw_cartoon_fore') == cls.modify_commandline_options
    assert data.find_dataset_using_name('umlvd_ifw_cartoon').__name__ == 'UMLVDIFWCartoonDataset'
    o = data.get_option_setter('umlvd_ifw_cartoon')(argparse.ArgumentParser(), True).parse_args([])
    assert o.data_prep == 'device' and o.list_dir == 'datasets/list'


@pytest.mark.parametrize('phase', ['train', 'test'])
def test_option_defaults_equal_the_reference(ref, phase):
    """every option the reference's modify_commandline_options registers or changes: same names, same defaults; and the
    options it does NOT have (the video-clip ones) are absent here too"""
    from animateportrait_amd.models import get_option_setter
    from animateportrait_amd.options.base_options import TrainOptions, TestOptions
    Options = TrainOptions if phase == 'train' else TestOptions
    base = Options().initialize(argparse.ArgumentParser())
    before = {a.dest for a in base._actions}
    p = get_option_setter('geomgm_ifw_cartoon_fore')(base, phase == 'train')
    want = ref['defaults_' + phase]
    for k, v in want.items():
        assert p.get_default(k) == v, (k, p.get_default(k), v)
    added = {a.dest for a in p._actions} - before
    assert added == set(want) - before, added ^ (set(want) - before)
    for gone in ('select_target12_thre', 'rx', 'ry', 'rs'):
        assert gone not in {a.dest for a in p._actions}
    # the drawing model keeps them
    q = get_option_setter('geomgm_ifw_fore')(TrainOptions().initialize(argparse.ArgumentParser()), True)
    assert q.get_default('select_target12_thre') == 0.2 and q.get_default('rs') == 0.7 and q.get_default('coherent') == 1 \
        and q.get_default('coh_use_more') == 2 and q.get_default('dataset_mode') == 'umlvd_ifw'


@pytest.mark.parametrize('tag', ['readme', 'variant'])
def test_readme_command_parses_and_names_equal_the_reference(ref, tag):
    from animateportrait_amd.models import find_model_using_name
    from animateportrait_amd.options.base_options import TrainOptions
    argv = ref['readme_argv'] + (ref['variant_argv'] if tag == 'variant' else [])
    opt = TrainOptions().parse(argv + ['--list_dir', 'x'])                  # the dataset's own options are registered too
    assert opt.model == 'geomgm_ifw_cartoon_fore' and opt.dataset_mode == 'umlvd_ifw_cartoon' and opt.output_nc == 3
    assert opt.coherent == 0 and opt.coh_use_more == 0 and not hasattr(opt, 'select_target12_thre')
    loss, vis = find_model_using_name(opt.model).reference_names(opt, True)
    assert vis == ref[tag]['visual_names'] and loss == ref[tag]['loss_names']
    assert 'real_A_fore' not in vis and 'fakeB_static_bg' not in vis
    opt = TrainOptions().parse([a if a != 'umlvd_ifw_cartoon' else 'synthetic' for a in argv])   # and on synthetic batches
    assert opt.dataset_mode == 'synthetic' and opt.synthetic_batches > 0


def test_synthetic_batch_follows_output_nc():
    from animateportrait_amd.data.synthetic_dataset import make_train_batch
    one, three = make_train_batch(1, seed=3, size=64), make_train_batch(1, seed=3, size=64, output_nc=3)
    for k in ('B', 'fakeB_static', 'B1', 'B2', 'B3', 'B4'):
        assert one[k].shape == (1, 1, 64, 64) and three[k].shape == (1, 3, 64, 64), k
    assert torch.equal(one['A'], three['A']) and set(one) == set(three)


def test_plan_sample_draws_in_the_reference_order(planned, golden):
    """paths, both get_params2 draws, the branch and the offsets: any extra, missing or reordered call on ``random`` /
    ``torch.rand`` moves every later draw"""
    ds, plans, root = planned
    gd = golden('cartoon_dataset.npz')
    assert sorted(int(gd['branch_%d' % s]) for s in range(3)) == [1, 1, 2]
    for s, p in enumerate(plans):
        assert [os.path.relpath(p[k], root) for k in ('A_path', 'B_path')] == gd['paths_%d' % s].tolist()
        assert '/Cartoon/' in p['B_path'] and p['image_paths'] == str(gd['image_paths_%d' % s])
        got = [(int(q[0]), int(q[1]), int(q[2])) for q in (p['pA'], p['pB'])]
        assert got == [tuple(r) for r in gd['params_%d' % s].tolist()], s
        assert p['branch'] == int(gd['branch_%d' % s])
        for k in ('A_lm_68', 'B_lm_68', 'tB_lm_68', 'tB2_lm_68'):                               # tB2 carries the offsets
            assert p[k].dtype == torch.float32 and torch.equal(p[k], gd['%s_%d' % (k, s)]), (s, k)
        for k in ('winA', 'winBr', 'winB', 'winB2'):
            assert p[k].tolist() == gd['%s_%d' % (k, s)].tolist(), (s, k)
        assert not any(k in p for k in ('B1_path', 'pB1', 'B1_lm_68', 'winBr1', 'B3_path'))
        assert not any(k.startswith(('B1', 'B2_lm', 'B2_path', 'winBr1', 'winBr2', 'B3', 'B4')) for k in gd['keys_%d' % s].tolist())


def test_host_frames_are_rgb_and_equal_the_reference(planned, golden):
    from animateportrait_amd.data import image_prep
    ds, plans, _ = planned
    gd = golden('cartoon_dataset.npz')
    step = int(gd['step'])
    item = ds.image_tensors(plans, mode='host')
    lut = image_prep.lut('image')
    assert item['B'].shape == (3, 3, 256, 256) and item['fakeB_static'].shape == (3, 3, 256, 256) and item['A'].shape == (3, 3, 256, 256)
    assert not any(k in item for k in ('B1', 'B2', 'B3', 'B4'))
    for s in range(3):
        for k in ('B', 'fakeB_static'):
            want = lut[torch.from_numpy(gd['%s_u8_%d' % (k, s)]).long()]
            assert torch.equal(item[k][s][:, ::step, ::step], want), (s, k)


def test_static_picture_is_read_only_when_a_loss_needs_it(tree):
    """umlvd_ifw_cartoon_dataset.py:301: warp_loss == 2 or identity_loss == 2"""
    from animateportrait_amd.data import create_dataset
    _, lists = tree
    for warp, iden, read in ((2, 2, True), (0, 2, True), (2, 0, True), (0, 0, False), (0, 1, False)):
        ds = create_dataset(cf.options(lists, dataset_mode='umlvd_ifw_cartoon', warp_loss=warp, identity_loss=iden, serial_batches=True))
        random.seed(1)
        torch.manual_seed(1)
        jobs = ds._jobs([ds.plan_sample(0)])
        assert any('/fakeB5_static/' in j[0] for j in jobs) == read, (warp, iden)
        assert not any('/fakeB_static/' in j[0] or '/Drawing/' in j[0] for j in jobs)


def test_clip_options_are_refused_by_name(tree):
    from animateportrait_amd.data import create_dataset
    _, lists = tree
    for over in (dict(coherent=1), dict(coh_use_more=2)):
        with pytest.raises(NotImplementedError, match='scanner_frag'):
            create_dataset(cf.options(lists, dataset_mode='umlvd_ifw_cartoon', **over))
