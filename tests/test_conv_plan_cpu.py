"""CPU (-m "not gpu"): the convolution planner's answers, pinned.  tests/golden/conv_plans.json holds what every plan query of the
C ABI answered for a sweep of descriptors at commit e450293 (the parent of the change that split make_plan and conv2d_fwd_impl in
what was then csrc/conv_host.hip into named steps; the planner is csrc/conv_plan.hip now); this test replays the sweep and compares every field for equality.  The plan reads shapes
only, never memory, and without a GPU the planner assumes 256 compute units -- the MI355X's count -- so the table is the same on
both kinds of machine.

The sweep is built here, deterministically; the golden file stores it next to the answers, so a change of the sweep shows up as a
difference too.  To record a new golden after a DELIBERATE planner change: ``python tests/test_conv_plan_cpu.py --record`` and name
the commit above."""
import ctypes
import json
import os
import sys

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'conv_plans.json')
FP32, BF16X3, BF16 = 0, 1, 2
ZERO, REFLECT = 0, 1
OIHW, IOHW = 0, 1
CONFIGS = {'default': {}, 'no_small_tiles': {'APAMD_NO_SMALL_TILES': '1'}, 'no_bf16x3': {'APAMD_NO_BF16X3': '1'}}
CONFIG_ORDER = ('default', 'no_small_tiles', 'no_bf16x3')
COUTS = (1, 2, 4, 8, 16, 32, 48, 64, 96, 128, 256, 512)


def _layer(segs, cout, k, stride=1, pad=0, mode=ZERO, tr=0, op=0, layout=OIHW, flip=0, s2d_k=0, kh=None):
    return (tuple(segs), cout, kh or k, k, stride, pad, mode, tr, op, layout, flip, s2d_k)


def sweep():
    """[(precision, layer, (N, H, W))]: the served shapes of the networks (tests/test_served_shapes_*.py, the generator, the
    PatchGAN, the landmark encoder, the flow regressor and their data gradients) and, around them, both sides of every branch
    of the kernel selection."""
    rows = []
    ALL, F_X3, X3_16 = (FP32, BF16X3, BF16), (FP32, BF16X3), (BF16X3, BF16)

    def add(layers, shapes, precs):
        rows.extend((p, lay, shp) for lay in layers for shp in shapes for p in precs)

    # 3x3 stride 1: every output width; the trunk, ResnetBlock2's concatenations, segments off the 16-channel grid and below 8
    add([_layer((64,), co, 3, 1, 1, REFLECT) for co in COUTS], [(1, 64, 64)], ALL)
    add([_layer((256,), co, 3, 1, 1, REFLECT) for co in (16, 48)], [(1, 64, 64)], ALL)
    segs3 = [(256,), (128,), (32, 32), (256, 16), (48, 16, 32), (128, 16, 16), (16,), (32,), (24,), (3,), (1,), (20,), (6, 2),
             (7, 5, 3), (40, 8), (64, 12), (9,)]
    add([_layer(s, 64, 3, 1, 1, ZERO) for s in segs3], [(2, 32, 32)], F_X3)
    add([_layer(s, 16, 3, 1, 1, REFLECT) for s in ((128,), (112,), (256, 16), (8,), (16,), (12,))], [(2, 64, 64)], F_X3)
    # ... both sides of the tall / short tile rule (128 | 136 tiles of 16 rows; maps no taller than the short tile)
    add([_layer((64,), 64, 3, 1, 1, REFLECT), _layer((256,), 256, 3, 1, 1, REFLECT)],
        [(16, 64, 64), (17, 64, 64), (8, 64, 64), (40, 4, 66), (40, 5, 66), (64, 2, 64), (16, 60, 64), (16, 64, 48),
         (1, 256, 256), (1, 8, 37)], X3_16)
    # the data-gradient forms: full correlation with flipped IOHW weights (the strip operator and its transposed column strip)
    add([_layer((64,), 64, 3, 1, 2, ZERO, 0, 0, IOHW, 1), _layer((256,), 256, 3, 1, 2, ZERO, 0, 0, IOHW, 1),
         _layer((128,), 16, 3, 1, 2, ZERO, 0, 0, IOHW, 1), _layer((64,), 8, 3, 1, 2, ZERO, 0, 0, IOHW, 1),
         _layer((64,), 3, 7, 1, 3, ZERO, 0, 0, IOHW, 1), _layer((64,), 1, 7, 1, 6, ZERO, 0, 0, IOHW, 1),
         _layer((512,), 256, 4, 1, 2, ZERO, 0, 0, IOHW, 1), _layer((16,), 8, 3, 1, 1, ZERO, 0, 0, IOHW, 1)],
        [(2, 64, 64), (2, 2, 64)], (FP32, BF16))
    # 3x3 stride 2 (the encoders) and the narrow layers of the landmark encoder at both strides
    add([_layer((64,), 128, 3, 2, 1), _layer((128,), 256, 3, 2, 1), _layer((128, 128), 256, 3, 2, 1), _layer((32,), 48, 3, 2, 1),
         _layer((1,), 8, 3, 2, 1), _layer((8,), 16, 3, 2, 1), _layer((16,), 16, 3, 2, 1), _layer((16,), 8, 3, 1, 1, REFLECT),
         _layer((17,), 16, 3, 1, 1), _layer((16,), 32, 3, 1, 1), _layer((8, 8), 16, 3, 1, 1), _layer((16,), 16, 3, 1, 1, ZERO, 0, 0, OIHW, 1)],
        [(1, 64, 64), (1, 33, 47)], F_X3)
    # 7x7 'same' layers: stems, the last layer (direct kernel: 1..4 outputs), the row form of a stem
    add([_layer((3,), 64, 7, 1, 3, REFLECT), _layer((1,), 64, 7, 1, 3, REFLECT), _layer((4,), 32, 7, 1, 3, REFLECT),
         _layer((64,), 1, 7, 1, 3, REFLECT), _layer((64,), 3, 7, 1, 3, REFLECT), _layer((64,), 4, 7, 1, 3, ZERO),
         _layer((64,), 2, 7, 1, 3, REFLECT), _layer((32, 32), 1, 7, 1, 3, REFLECT), _layer((30, 3, 1), 3, 7, 1, 3, REFLECT),
         _layer((64,), 8, 7, 1, 3, REFLECT), _layer((64,), 64, 7, 1, 3, REFLECT), _layer((64,), 1, 7, 1, 2, REFLECT),
         _layer((64,), 1, 7, 2, 3, ZERO)], [(2, 64, 48)], F_X3)
    add([_layer((32,), 64, 7, 1, 3, REFLECT, kh=1), _layer((32,), 32, 7, 1, 3, ZERO, kh=1), _layer((32,), 96, 7, 1, 3, REFLECT, kh=1)],
        [(1, 256, 256)], ALL)
    # 4x4: the PatchGAN (stride 2 body, stride 1 tail, the one-channel head on both sides of kHeadMaxW = 31)
    add([_layer((2,), 64, 4, 2, 1), _layer((1,), 64, 4, 2, 1), _layer((64,), 128, 4, 2, 1), _layer((128,), 256, 4, 2, 1),
         _layer((256,), 512, 4, 1, 1), _layer((512,), 1, 4, 1, 1), _layer((64,), 1, 4, 1, 1), _layer((48,), 1, 4, 1, 1),
         _layer((256, 256), 1, 4, 1, 1), _layer((512,), 1, 4, 1, 2), _layer((512,), 1, 4, 1, 1, ZERO, 0, 0, OIHW, 1),
         _layer((512,), 2, 4, 1, 1), _layer((64,), 64, 4, 1, 1, REFLECT)],
        [(2, 31, 31), (2, 32, 32)], F_X3)
    # 2x2: the space-to-depth form of the 4x4 / 3x3 stride-2 layers (s2d_k = 3: 7 of 16 taps skipped); 1x1: channel_mapping
    add([_layer((256,), 128, 2), _layer((512,), 256, 2), _layer((256,), 128, 2, s2d_k=3), _layer((128,), 64, 2, s2d_k=3),
         _layer((512,), 256, 2, s2d_k=3), _layer((256,), 32, 2), _layer((24,), 64, 2), _layer((256,), 128, 2, 1, 1)],
        [(2, 65, 65)], ALL)
    add([_layer((256,), 64, 1), _layer((64,), 256, 1), _layer((48,), 48, 1), _layer((256,), 2, 1), _layer((20,), 64, 1),
         _layer((64,), 64, 1, 1, 1), _layer((64,), 64, 1, 2, 0)], [(1, 33, 17)], F_X3)
    # transposed stride 2: even outputs (all phases in one tile, ph4 = 3 | 4; pad 0: fused phases), odd outputs (four launches),
    # the narrow-output form of the PatchGAN's first-layer data gradient, layouts and flips
    add([_layer((256,), 128, 3, 2, 1, ZERO, 1, 1, IOHW), _layer((128,), 64, 3, 2, 1, ZERO, 1, 1, IOHW),
         _layer((256,), 128, 3, 2, 1, ZERO, 1, 0, IOHW), _layer((256,), 128, 3, 2, 0, ZERO, 1, 1, IOHW),
         _layer((256,), 128, 3, 2, 0, ZERO, 1, 0, IOHW), _layer((128,), 64, 4, 2, 1, ZERO, 1, 0, IOHW),
         _layer((128,), 64, 4, 2, 1, ZERO, 1, 1, IOHW), _layer((128,), 64, 4, 2, 0, ZERO, 1, 0, IOHW),
         _layer((128,), 64, 4, 2, 1, ZERO, 1, 0, OIHW, 1), _layer((256,), 128, 3, 2, 1, ZERO, 1, 1, OIHW, 1),
         _layer((64,), 2, 4, 2, 1, ZERO, 1, 0, IOHW), _layer((64,), 1, 4, 2, 1, ZERO, 1, 0, IOHW), _layer((64,), 3, 4, 2, 1, ZERO, 1, 0, IOHW),
         _layer((64,), 4, 4, 2, 1, ZERO, 1, 0, IOHW), _layer((64,), 2, 4, 2, 1, ZERO, 1, 0, OIHW), _layer((64,), 8, 4, 2, 1, ZERO, 1, 0, IOHW),
         _layer((64,), 2, 4, 2, 1, ZERO, 1, 1, IOHW), _layer((32, 32), 2, 4, 2, 1, ZERO, 1, 0, IOHW),
         _layer((16,), 8, 3, 2, 1, ZERO, 1, 1, IOHW), _layer((24, 8), 64, 3, 2, 1, ZERO, 1, 1, IOHW), _layer((64,), 32, 3, 2, 1, ZERO, 1, 1, IOHW),
         _layer((64,), 64, 1, 2, 0, ZERO, 1, 1, IOHW), _layer((64,), 64, 2, 2, 0, ZERO, 1, 0, IOHW)],
        [(2, 64, 64)], F_X3)
    add([_layer((256,), 128, 3, 2, 1, ZERO, 1, 1, IOHW), _layer((256,), 128, 3, 2, 1, ZERO, 1, 0, IOHW),
         _layer((128,), 64, 4, 2, 1, ZERO, 1, 0, IOHW)], [(1, 16, 31), (1, 1, 1)], (BF16,))
    # descriptors that must be refused
    add([_layer((64,), 64, 5, 1, 2), _layer((64,), 64, 6, 1, 2), _layer((64,), 64, 8, 1, 3), _layer((64,), 64, 5, 1, 1, kh=3),
         _layer((64,), 64, 3, 3, 1), _layer((64,), 64, 3, 1, 1, ZERO, 1, 0, IOHW), _layer((64,), 64, 3, 2, 1, REFLECT, 1, 1, IOHW),
         _layer((64,), 64, 3, 1, 9, REFLECT), _layer((64,), 64, 7, 1, 0), _layer((64, 0), 64, 3, 1, 1), _layer((), 64, 3, 1, 1),
         _layer((64,), 0, 3, 1, 1), _layer((64,), 64, 7, 2, 1, ZERO, 1, 1, IOHW), _layer((64,), 64, 7, 2, 3),
         _layer((16,), 64, 7, 1, 3, REFLECT, kh=1), _layer((32,), 64, 7, 1, 3, REFLECT, 0, 0, IOHW, kh=1),
         _layer((32,), 64, 7, 1, 3, REFLECT, 0, 0, OIHW, 1, kh=1), _layer((32,), 64, 7, 2, 3, REFLECT, kh=1),
         _layer((256,), 128, 2, 1, 0, ZERO, 0, 0, IOHW), _layer((256,), 128, 2, 2, 0)], [(1, 8, 8)], (BF16X3,))
    add([_layer((64,), 64, 3, 1, 1)], [(0, 8, 8), (1, 0, 8)], (FP32,))
    return rows


def _desc(prec, layer, shape):
    from animateportrait_amd import _capi
    segs, cout, kh, kw, stride, pad, mode, tr, op, layout, flip, s2d_k = layer
    d = _capi.ApConvDesc()
    d.N, d.H, d.W = shape
    d.Cout, d.KH, d.KW, d.stride, d.pad, d.pad_mode = cout, kh, kw, stride, pad, mode
    d.transposed, d.output_padding, d.w_layout, d.w_flip, d.s2d_k = tr, op, layout, flip, s2d_k
    d.nsrc, d.precision = len(segs), prec
    for i, c in enumerate(segs):
        d.src[i].C = c
    return d


def answers(lib, prec, layer, shape):
    """What the planner says about one descriptor: [rc, Hout, Wout, packed floats, stat tiles, wants presplit, kernel name (or its
    refusal code), octet ok, bf16out ok]."""
    d = _desc(prec, layer, shape)
    ref = ctypes.byref(d)
    ho, wo = ctypes.c_int32(-1), ctypes.c_int32(-1)
    rc = lib.ap_conv2d_out_size(ref, ctypes.byref(ho), ctypes.byref(wo))
    buf = ctypes.create_string_buffer(96)
    nrc = lib.ap_conv2d_kernel_name(ref, buf, 96)
    return [rc, ho.value, wo.value, lib.ap_conv2d_packed_floats(ref), lib.ap_conv2d_stat_tiles(ref),
            lib.ap_conv2d_wants_presplit(ref), buf.value.decode() if nrc == 0 else nrc, lib.ap_conv2d_octet_ok(ref),
            lib.ap_conv2d_bf16out_ok(ref)]


def _table(lib):
    return [answers(lib, p, lay, shp) for p, lay, shp in sweep()]


def _use(env, setenv, delenv):
    from animateportrait_amd import ops
    for v in ops.plan_switch_names():      # every environment switch a route decision reads: make_plan's and the *_ok predicates' among them
        delenv(v)
    for k, v in env.items():
        setenv(k, v)


@pytest.fixture(scope='module')
def lib():
    from animateportrait_amd import _capi
    return _capi.lib()


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _recorded(golden, config):
    """golden row: [precision, layer, shape, answers by default, answers under each other setting of CONFIGS or null = the same]"""
    col = 3 + CONFIG_ORDER.index(config)
    return [r[col] if r[col] is not None else r[3] for r in golden]


@pytest.mark.parametrize('config', CONFIG_ORDER)
def test_conv_plans_match_the_recorded_table(lib, golden, monkeypatch, config):
    _use(CONFIGS[config], monkeypatch.setenv, lambda v: monkeypatch.delenv(v, raising=False))
    rows = sweep()
    assert [[p, [list(lay[0])] + list(lay[1:]), list(shp)] for p, lay, shp in rows] == [r[:3] for r in golden] and len(rows) >= 300
    got, want = _table(lib), _recorded(golden, config)
    bad = [(r[:3], g, w) for r, g, w in zip(golden, got, want) if g != w]
    assert not bad, '%d of %d plans differ; first (descriptor, got, recorded): %r' % (len(bad), len(got), bad[0])


def test_the_sweep_reaches_every_family_and_refusal(golden):
    """The golden table is only a pin if it exercises the selection: every kernel family, both tile heights, both fused-phase
    forms, every output form and each refusal code appear in it."""
    rows = [a for c in ('default', 'no_small_tiles') for a in _recorded(golden, c)]
    names = {a[6] for a in rows if isinstance(a[6], str)}
    for prefix in ('DirectCfg<7, 1>', 'DirectCfg<7, 4>', 'SmallCfg<1, 8>', 'SmallCfg<2, 16>', 'HeadCfg<4>', 'TSmallCfg<1>',
                   'TSmallCfg<4>', 'ConvCfg<2, ', 'ConvCfg<4, ', 'ConvCfg<8, ', 'Bf3Cfg<1, 3, 1, 2, 4, 4>', 'Bf3Cfg<1, 3, 1, 2, 4, 1>',
                   'Bf3Cfg<2, 3, ', 'Bf3Cfg<1, 4, ', 'Bf3Cfg<1, 7, 1, 1, 4, 2, 0, 1>',       # (the row form always takes its short tile)
                   'Bf3Cfg<1, 0, 1, 2, 4, 4, 4>', 'Bf3Cfg<1, 0, 1, 2, 4, 2, 4>', 'Ph4Cfg<3', 'Ph4Cfg<4'):
        assert any(n.startswith(prefix) for n in names), prefix
    assert any(n.endswith(' bf16') for n in names)
    assert {a[0] for a in rows} == {0, -1, -2}
    for col in (5, 7, 8):                          # wants presplit, octet, bf16 out: answered both ways
        assert {a[col] for a in rows if a[0] == 0} == {0, 1}, col
    # (the 1 x 7 row form exists on the split-bf16 path only and does not read the switch)
    assert all(a[5] == 0 for r, a in zip(golden, _recorded(golden, 'no_bf16x3')) if a[0] == 0 and r[1][2] == r[1][3])


if __name__ == '__main__' and '--record' in sys.argv:
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from animateportrait_amd import _capi
    tables = []
    for name in CONFIG_ORDER:
        _use(CONFIGS[name], os.environ.__setitem__, lambda v: os.environ.pop(v, None))
        tables.append(_table(_capi.lib()))
    rows = [[p, [list(lay[0])] + list(lay[1:]), list(shp), a[0]] + [b if b != a[0] else None for b in a[1:]]
            for (p, lay, shp), a in zip(sweep(), zip(*tables))]
    with open(GOLDEN, 'w') as f:
        f.write('[\n' + ',\n'.join(json.dumps(r, separators=(',', ':')) for r in rows) + '\n]\n')
    print('recorded', len(rows), 'plans in', GOLDEN)
