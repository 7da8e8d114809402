"""umlvdfw_test without a device: the registry, the decisions of plan_item against the reference's golden items
(tests/golden/make_test_dataset_golden.py), list / directory discovery, the refusals, the data ABI's new names, and the
--save_format flag of test.py."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import testset_fixture as tf          # noqa: E402

NEW_NAMES = ('apd_landmark_map_ok', 'apd_landmark_map', 'apd_landmark_marks_ok', 'apd_landmark_marks', 'apd_frames_to_u8_ok',
             'apd_frames_to_u8')


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    work = tmp_path_factory.mktemp('umlvdfw_cpu')
    root, lists = str(work / 'tree'), str(work / 'lists')
    tf.write_test_tree(root, lists)
    return root, lists


def test_registry_resolves_umlvdfw_test():
    import argparse
    from animateportrait_amd import data
    cls = data.find_dataset_using_name('umlvdfw_test')
    assert cls.__name__ == 'UMLVDFWTestDataset'
    o = data.get_option_setter('umlvdfw_test')(argparse.ArgumentParser(), False).parse_args([])
    assert o.lmark_lookup == 'faceLmarkLookup.npy' and o.data_prep == 'device' and o.list_dir == 'datasets/list'


def test_plan_item_equals_the_reference(tree, golden):
    from animateportrait_amd.data import find_dataset_using_name
    gd = golden('test_dataset.npz')
    assert gd['items'].tolist() == [list(map(int, i)) for i in tf.ITEMS]
    seen_b = set()
    for s, (index, draw_op, serial, seed) in enumerate(tf.ITEMS):
        ds = find_dataset_using_name('umlvdfw_test')(tf.options(tree[1], draw_op=draw_op, serial_batches=bool(serial),
                                                                 no_flip=bool(serial)))
        assert len(ds) == 3
        random.seed(seed)
        torch.manual_seed(seed)
        p = ds.plan_item(index)
        assert [os.path.relpath(p[k], tree[0]) for k in ('A_path', 'B_path')] == gd['paths_%d' % s].tolist()
        assert p['index_B'] == int(gd['index_B_%d' % s])
        assert [tuple(int(v) for v in p[k]) for k in ('pA', 'pB')] == [tuple(r) for r in gd['params_%d' % s].tolist()]
        for k in ('A_lm_68', 'tB_lm_68'):
            assert p[k].dtype == torch.float32 and torch.equal(p[k], gd['%s_%d' % (k, s)]), (s, k)       # bit-equal
        assert p['winB'].tolist() == gd['winB_%d' % s].tolist()
        assert p['image_paths'] == str(gd['image_paths_%d' % s])
        seen_b.add('Alm' in p['B_path'])
    assert seen_b == {True, False}                                  # both landmark-path rules for B were taken
    # the item drawn without --serial_batches did not land on the serial index: the draw was random.randint's
    index, _, serial, _ = tf.ITEMS[2]
    assert not serial and int(gd['index_B_2']) != index % 3


def test_list_files_and_directory_scan_give_the_same_order(tmp_path, monkeypatch):
    from animateportrait_amd.data import find_dataset_using_name
    cls = find_dataset_using_name('umlvdfw_test')
    root = tmp_path / 'scan'
    rel_a = ['testA/Photo/b.png', 'testA/Photo/a.jpg', 'testA/Photo/sub/c.png']
    rel_b = ['testB/Drawing/real/z.png', 'testB/Alm/MTCNN/a.png', 'testB/Drawing/fake/y.png']
    for rel in rel_a + rel_b + ['testA/Photo/notes.txt']:
        (root / rel).parent.mkdir(parents=True, exist_ok=True)
        (root / rel).write_bytes(b'')
    scanned = cls(tf.options(str(tmp_path / 'no_lists'), dataroot=str(root)))
    lists = tmp_path / 'lists'
    for side, rels in (('A', rel_a), ('B', rel_b)):
        (lists / ('test' + side)).mkdir(parents=True)
        (lists / ('test' + side) / 'named.txt').write_text('\n'.join(str(root / r) for r in rels) + '\n')
    listed = cls(tf.options(str(lists), dataroot='named'))
    assert scanned.A_paths == listed.A_paths == sorted(str(root / r) for r in rel_a)
    assert scanned.B_paths == listed.B_paths == sorted(str(root / r) for r in rel_b)
    with pytest.raises(RuntimeError, match='no images'):
        cls(tf.options(str(tmp_path / 'no_lists'), dataroot=str(tmp_path / 'nowhere')))


def test_refusals(tree, tmp_path):
    from animateportrait_amd.data import find_dataset_using_name
    cls = find_dataset_using_name('umlvdfw_test')
    with pytest.raises(NotImplementedError, match='draw_op 2.*1-channel landmark encoder'):
        cls(tf.options(tree[1], draw_op=2))
    with pytest.raises(FileNotFoundError, match='draw_op 1.*no_such_lookup.npy.*lmark_lookup'):
        cls(tf.options(tree[1], draw_op=1, lmark_lookup=str(tmp_path / 'no_such_lookup.npy')))
    cls(tf.options(tree[1], draw_op=0, lmark_lookup=str(tmp_path / 'no_such_lookup.npy')))       # read only for --draw_op 1
    with pytest.raises(NotImplementedError, match='preprocess scale_width is not served'):
        cls(tf.options(tree[1], preprocess='scale_width'))
    ds = cls(tf.options(tree[1], preprocess='none'))                      # 300 x 280 photos at load 286: not what 'none' means
    with pytest.raises(NotImplementedError, match='preprocess none'):
        ds.plan_item(0)
    assert cls(tf.options(tree[1], draw_op=1)).segments.shape == (64, 2)


def test_lookup_fixture_is_the_table():
    seg = np.load(tf.LOOKUP)
    assert seg.shape == (64, 2) and seg.dtype.kind == 'i' and seg.min() >= 0 and seg.max() <= 67


def test_new_names_are_declared_and_exported():
    from animateportrait_amd import _dataapi as D
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'animateportrait_data.h')).read()
    assert all(n in D.SIGNATURES for n in NEW_NAMES)
    assert all(name + '(' in header for name in D.SIGNATURES)
    assert '#define APD_ABI_VERSION 1' in header and D.ABI_VERSION == 1
    lib = D.lib()
    assert all(hasattr(lib, n) for n in D.SIGNATURES) and lib.apd_abi_version() == 1
    for macro, value in (('APD_MAX_SEGMENTS', D.MAX_SEGMENTS), ('APD_MAX_RADIUS', D.MAX_RADIUS), ('APD_MAX_THICKNESS', D.MAX_THICKNESS),
                         ('APD_MAX_MAP', D.MAX_MAP), ('APD_MAX_POINTS', D.MAX_POINTS)):
        assert '#define %s %d ' % (macro, value) in header


def test_a_stale_library_is_named_by_its_missing_symbol(monkeypatch):
    from animateportrait_amd import _dataapi as D
    monkeypatch.setattr(D, '_lib', None)
    monkeypatch.setitem(D.SIGNATURES, 'apd_not_built_yet', (ctypes.c_int, []))
    with pytest.raises(RuntimeError, match='stale.*apd_not_built_yet'):
        D.lib()


def test_ok_functions_refuse_without_a_device():
    """the pointers are never dereferenced by the *_ok calls (except seg_host, a host table): any non-null value stands in"""
    from animateportrait_amd import _dataapi as D
    lib = D.lib()
    x = ctypes.c_void_p(4096)
    seg = (ctypes.c_int32 * 8)(0, 1, 1, 2, 2, 3, 67, 0)
    sp = ctypes.cast(seg, ctypes.c_void_p)

    def map_ok(lm=x, seg_dev=x, seg_host=sp, out=x, n=2, p=68, s=4, h=256, w=256, radius=3, thickness=2, op=1):
        return lib.apd_landmark_map_ok(lm, seg_dev, seg_host, out, n, p, s, h, w, radius, thickness, op)
    assert map_ok() == 1 and map_ok(s=0, seg_dev=None, seg_host=None) == 1 and map_ok(op=0, seg_dev=None, seg_host=None) == 1
    for bad, word in ((dict(lm=None), 'null'), (dict(out=None), 'null'), (dict(seg_dev=None), 'segment table'),
                      (dict(seg_host=None), 'segment table'), (dict(s=129), 'S = 129'), (dict(p=67), 'names landmark 67 of 67'),
                      (dict(radius=32), 'radius = 32'), (dict(thickness=0), 'thickness'), (dict(thickness=17), 'thickness'),
                      (dict(h=1025), '1025'), (dict(w=0), 'map'), (dict(op=2), 'op = 2'), (dict(n=0), 'N = 0')):
        assert map_ok(**bad) == 0, bad
        assert 'landmark_map' in D.last_error() and word in D.last_error(), (bad, D.last_error())
    big = (ctypes.c_int32 * 258)(*([0] * 258))
    assert map_ok(seg_host=ctypes.cast(big, ctypes.c_void_p), s=128) == 1 and map_ok(seg_host=ctypes.cast(big, ctypes.c_void_p), s=129) == 0
    assert lib.apd_landmark_map(x, x, sp, 2, 68, 4, 256, 256, 32, 2, 1, -1.0, 1.0, x, None) < 0        # refused: nothing launched

    assert lib.apd_landmark_marks_ok(x, x, x, x, 2, 3, 68, 48, 40, 3) == 1
    for args in ((None, x, x, x, 2, 3, 68, 48, 40, 3), (x, None, x, x, 2, 3, 68, 48, 40, 3), (x, x, None, x, 2, 3, 68, 48, 40, 3),
                 (x, x, x, None, 2, 3, 68, 48, 40, 3), (x, x, x, x, 2, 2, 68, 48, 40, 3), (x, x, x, x, 2, 3, 0, 48, 40, 3),
                 (x, x, x, x, 2, 3, 68, 48, 40, -1), (x, x, x, x, 0, 3, 68, 48, 40, 3)):
        assert lib.apd_landmark_marks_ok(*args) == 0 and 'landmark_marks' in D.last_error(), args

    assert lib.apd_frames_to_u8_ok(x, x, 2, 1, 5, 7) == 1
    for args in ((None, x, 2, 1, 5, 7), (x, None, 2, 1, 5, 7), (x, x, 2, 2, 5, 7), (x, x, 0, 1, 5, 7), (x, ctypes.c_void_p(4097), 2, 1, 5, 7),
                 (x, x, 4096, 3, 512, 512)):
        assert lib.apd_frames_to_u8_ok(*args) == 0 and 'frames_to_u8' in D.last_error(), args


def test_save_format_flag():
    from animateportrait_amd import test as entry
    base = ['--model', 'geomcgt_ifw_test', '--dataroot', 'x']
    opt = entry.parse(base)
    assert opt.save_format == 'npy' and opt.dataset_mode == 'umlvdfw_test' and opt.lmark_lookup == 'faceLmarkLookup.npy'
    assert entry.parse(base + ['--save_format', 'png']).save_format == 'png'
    assert entry.parse(base + ['--save_format', 'both', '--draw_op', '1']).draw_op == 1
    with pytest.raises(SystemExit):
        entry.parse(base + ['--save_format', 'jpeg'])
    from animateportrait_amd.data import visuals
    assert visuals.PNG_THREADS <= 16
