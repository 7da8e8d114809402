"""The device PNG encoder without a device: the names the data ABI gained, what apd_png_encode_ok refuses, apd_png_bound,
the entry points' flags, and the encoder's own text (csrc/data/png_deflate.h) compiled for the host under
-fsanitize=address,undefined by tools/png_host_check.py and read back by two decoders (tests/png_fixture.py)."""
import ctypes
import importlib.util
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_fixture as pf          # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ('apd_png_bound', 'apd_png_workspace_bytes', 'apd_png_encode_ok', 'apd_png_encode')
IMAGES = pf.images()


def _tool():
    spec = importlib.util.spec_from_file_location('png_host_check', os.path.join(ROOT, 'tools', 'png_host_check.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope='module')
def host_files(tmp_path_factory):
    """every image of the fixture through the sanitised host program, once: name -> (file bytes, bound)"""
    tool = _tool()
    work = str(tmp_path_factory.mktemp('png_host'))
    exe = tool.build(work)
    names = sorted(IMAGES)
    return dict(zip(names, tool.encode(exe, work, [IMAGES[n] for n in names])))


def test_new_names_are_declared_and_exported():
    from animateportrait_amd import _dataapi as D
    header = open(os.path.join(ROOT, 'include', 'animateportrait_data.h')).read()
    assert all(n in D.SIGNATURES and n + '(' in header for n in NEW_NAMES)
    assert '#define APD_ABI_VERSION 1' in header and D.ABI_VERSION == 1
    assert '#define APD_MAX_PNG_SIDE %d ' % D.MAX_PNG_SIDE in header and D.MAX_PNG_SIDE == 2048
    lib = D.lib()
    assert all(hasattr(lib, n) for n in NEW_NAMES) and lib.apd_abi_version() == 1
    common = open(os.path.join(ROOT, 'animateportrait_amd', 'csrc', 'data', 'apd_common.h')).read()
    frames = open(os.path.join(ROOT, 'animateportrait_amd', 'csrc', 'data', 'frames_u8.hip')).read()
    assert 'unsigned to_byte(float x)' in common and 'unsigned to_byte(float x)' not in frames          # one definition, shared


def test_bound_and_workspace():
    from animateportrait_amd import _dataapi as D
    lib = D.lib()
    for h, w in ((1, 1), (37, 53), (256, 256), (2048, 3), (3, 2048), (2048, 2048), (1, 2048), (2048, 1), (16, 1023)):
        for ch in (1, 3):
            b = lib.apd_png_bound(h, w, ch)
            assert b > 0 and b % 4 == 0 and b <= pf.bound_limit(h, w, ch), (h, w, ch, b)
            assert b >= h * (w * ch + 1) + 66                                  # noise does not shrink
            assert lib.apd_png_workspace_bytes(3, h, w, ch) == 3 * lib.apd_png_workspace_bytes(1, h, w, ch) > 0
    for args in ((0, 5, 3), (5, 0, 3), (2049, 5, 3), (5, 2049, 1), (5, 5, 2), (5, 5, 4)):
        assert lib.apd_png_bound(*args) < 0 and 'png_bound' in D.last_error(), args
    assert lib.apd_png_workspace_bytes(0, 5, 5, 3) < 0 and lib.apd_png_workspace_bytes(1, 5, 5, 2) < 0


def test_ok_refuses_without_a_device():
    """the pointers are never dereferenced by apd_png_encode_ok: any non-null aligned value stands in"""
    from animateportrait_amd import _dataapi as D
    lib = D.lib()
    x = ctypes.c_void_p(4096)

    def ok(src=x, dst=x, sizes=x, ws=x, n=2, c=1, h=37, w=53, ch=3, slot=None, wsb=None):
        slot = lib.apd_png_bound(h, w, ch) if slot is None else slot
        wsb = lib.apd_png_workspace_bytes(n, h, w, ch) if wsb is None else wsb
        return lib.apd_png_encode_ok(src, dst, sizes, ws, n, c, h, w, ch, slot, wsb)
    assert ok() == 1 and ok(c=3) == 1 and ok(ch=1) == 1 and ok(h=2048, w=2048, n=1) == 1 and ok(h=1, w=1) == 1
    bound = lib.apd_png_bound(37, 53, 3)
    assert ok(slot=bound + 4) == 1
    for bad, word in ((dict(src=None), 'null'), (dict(dst=None), 'null'), (dict(sizes=None), 'null'), (dict(ws=None), 'null'),
                      (dict(c=2), 'C = 2'), (dict(c=4), 'C = 4'), (dict(ch=2, slot=bound, wsb=1 << 20), 'channels = 2'),
                      (dict(ch=0, slot=bound, wsb=1 << 20), 'channels = 0'), (dict(c=3, ch=1), 'needs C = 1'),
                      (dict(h=0, slot=bound, wsb=1 << 20), 'sides'), (dict(w=0, slot=bound, wsb=1 << 20), 'sides'),
                      (dict(h=2049, slot=1 << 24, wsb=1 << 30), '2049'), (dict(w=2049, slot=1 << 24, wsb=1 << 30), '2049'),
                      (dict(slot=bound - 4), 'below apd_png_bound'), (dict(slot=bound + 2), 'multiple of 4'),
                      (dict(n=0, slot=bound, wsb=1 << 20), 'N = 0'),
                      (dict(n=2, slot=1 << 30, wsb=1 << 30), '2^31'),
                      (dict(wsb=lib.apd_png_workspace_bytes(2, 37, 53, 3) - 1), 'workspace'),
                      (dict(dst=ctypes.c_void_p(4097)), 'aligned'), (dict(sizes=ctypes.c_void_p(4098)), 'aligned')):
        assert ok(**bad) == 0, bad
        assert 'png_encode' in D.last_error() and word in D.last_error(), (bad, D.last_error())
    # the launching call refuses the same way, before it asks the runtime anything: nothing is launched
    assert lib.apd_png_encode(x, 2, 2, 37, 53, 3, x, bound, x, x, 1 << 20, None) < 0 and 'C = 2' in D.last_error()
    assert lib.apd_png_encode(x, 2, 1, 37, 53, 3, x, bound - 4, x, x, 1 << 20, None) < 0 and 'below apd_png_bound' in D.last_error()


def test_flags():
    from animateportrait_amd import end2end, test as entry
    from animateportrait_amd.data import visuals
    base = ['--model', 'geomcgt_ifw_test', '--dataroot', 'x']
    assert entry.parse(base).png_encoder == 'host' and entry.parse(base).save_format == 'npy'
    assert entry.parse(base + ['--save_format', 'png', '--png_encoder', 'device']).png_encoder == 'device'
    with pytest.raises(SystemExit):
        entry.parse(base + ['--png_encoder', 'zlib'])
    ap = end2end.make_parser()
    a = ap.parse_args(['--photo', 'p.png', '--out', 'o'])
    assert a.png_encoder == 'host' and a.png_channels == 3
    a = ap.parse_args(['--photo', 'p.png', '--out', 'o', '--png_encoder', 'device', '--png_channels', '1'])
    assert a.png_encoder == 'device' and a.png_channels == 1
    with pytest.raises(SystemExit):
        ap.parse_args(['--photo', 'p.png', '--out', 'o', '--png_channels', '2'])
    with pytest.raises(ValueError, match='encoder'):
        visuals.save_png_batch({'a': None}, {'a': []}, encoder='zlib')


def test_decoder_refuses_damage(host_files):
    """the yardstick itself: one flipped byte in a chunk's data, in a CRC or in the Adler-32, or a byte after IEND, is caught"""
    import zlib
    data, _ = host_files['noise37x53_rgb']
    assert np.array_equal(pf.decode(data), IMAGES['noise37x53_rgb'])
    for at in (20, 60, len(data) - 40, len(data) - 27, len(data) - 22, len(data) - 3):       # IHDR, data, a CRC, Adler, CRC, IEND
        broken = bytearray(data)
        broken[at] ^= 0x10
        with pytest.raises((AssertionError, zlib.error)):
            pf.decode(bytes(broken))
    with pytest.raises(AssertionError, match='after IEND'):
        pf.decode(data + b'\x00')


@pytest.mark.parametrize('name', sorted(IMAGES))
def test_host_program_files_decode_to_their_images(host_files, name):
    data, bound = host_files[name]
    im = IMAGES[name]
    pf.check_both(data, im)
    h, w, ch = im.shape
    print('%s: %d bytes, bound %d, raw %d' % (name, len(data), bound, im.size))
    assert len(data) <= bound <= pf.bound_limit(h, w, ch)
    from animateportrait_amd import _dataapi as D
    assert bound == D.lib().apd_png_bound(h, w, ch)                 # the host program and the library state one bound


def test_host_program_sizes(host_files):
    """the issue's size conditions on the layout: all white <= raw / 20, the line drawing <= raw / 3"""
    white, lines = len(host_files['white256_rgb'][0]), len(host_files['lines256_rgb'][0])
    print('white 256 x 256 RGB: %d bytes; line drawing: %d bytes; raw 196608' % (white, lines))
    assert white * 20 <= 196608
    assert lines * 3 <= 196608
