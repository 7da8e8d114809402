"""CPU (-m "not gpu"): the weight-gradient planner's answers, pinned.  tests/golden/wgrad_plans.json holds what every plan query of
the backward half of the C ABI answered for a sweep of descriptors and shapes at commit 3f2dcd7 (the parent of the change that split
make_wgrad_plan and wgrad_impl in what was then csrc/wgrad_host.hip into per-family steps and moved the edge-layer entry points to
csrc/edge_host.hip; the planner is csrc/wgrad_plan.hip now, the launchers csrc/wgrad_launch.hip and csrc/wgrad_operand.hip); this test replays the sweep and compares every field for equality.  The plan reads shapes and whether pointers
are null, never memory, and without a GPU the planner assumes 256 compute units -- the MI355X's count -- so the table is the same on
both kinds of machine.

Two tables: the descriptor-driven queries (ap_conv2d_wgrad_workspace_floats / _gt_dims / _xs_ok, under every environment switch the
planner reads) and the shape-driven ones of the edge layers (k7, d0, final, head).  A descriptor's fifth answer is the one decision
of the planner no query reports -- may the shifted operand come from the forward pass's split copies (wgrad_xs_route)? -- read off
the argument validation of ap_conv2d_wgrad: a descriptor whose first segment has no data and a mean without rstd is refused as
'null data' where the route is closed and as 'mean/rstd mismatch' where it is open, before anything is launched.

The sweep is built here, deterministically; the golden file stores it next to the answers, so a change of the sweep shows up as a
difference too.  To record a new golden after a DELIBERATE planner change: ``python tests/test_wgrad_plan_cpu.py --record`` and
name the commit above."""
import ctypes
import json
import os
import sys

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'wgrad_plans.json')
FP32, BF16X3, BF16 = 0, 1, 2
ZERO, REFLECT = 0, 1
CONFIGS = {'default': {}, 'no_bf16x3': {'APAMD_NO_BF16X3': '1'}, 'no_s2d': {'APAMD_NO_S2D_WGRAD': '1'},
           'rows': {'APAMD_ROWS_WGRAD': '1'}, 'no_xs_direct': {'APAMD_NO_XS_DIRECT': '1'}, 'no_xs': {'APAMD_NO_XS_WGRAD': '1'},
           'blocks64': {'APAMD_WGRAD_BLOCKS': '64'}}
CONFIG_ORDER = ('default', 'no_bf16x3', 'no_s2d', 'rows', 'no_xs_direct', 'no_xs', 'blocks64')
ALL, F_X3, X3_16 = (FP32, BF16X3, BF16), (FP32, BF16X3), (BF16X3, BF16)
NO_XS = (0, 0, 0)
# (xs_parts, src_xs[] filled, src_xs_s2d filled): the forward pass's split copies as a descriptor can carry them
XS_FORMS = ((0, 1, 0), (1, 1, 0), (2, 1, 0), (3, 1, 0), (2, 0, 0), (2, 0, 1), (2, 1, 1), (1, 0, 1))
SOME_POINTER = 0x1000           # the planner only asks whether a pointer is null


def _layer(segs, m, k, stride=1, pad=None, mode=ZERO, g=0, xs=NO_XS, grid=0, nsrc=None):
    """g = 1: the gradient is a virtual (normalised + activated) tensor; grid: added to GH (a grid that is not the conv output)"""
    return (tuple(segs), m, k, stride, (k - 1) // 2 if pad is None else pad, mode, g, tuple(xs), grid,
            len(segs) if nsrc is None else nsrc)


def sweep():
    """[(precision, layer, (N, H, W))]: the served layers of the generator, the PatchGAN and the landmark encoder at small maps and,
    around them, both sides of every branch of make_wgrad_plan and of the xs predicates."""
    rows = []

    def add(layers, shapes, precs):
        rows.extend((p, lay, shp) for lay in layers for shp in shapes for p in precs)

    # generator: the 7x7 stems (the 30 % tile rule: 64 x 192 against 128 x 256 tiles at Cin = 3), a wide 7x7, the last layer
    add([_layer((3,), m, 7, 1, 3, REFLECT) for m in (32, 64, 128)] + [_layer((1,), 64, 7, 1, 3, REFLECT), _layer((4,), 32, 7, 1, 3, REFLECT)],
        [(2, 32, 32), (1, 33, 47)], ALL)
    add([_layer((64,), 64, 7, 1, 3, REFLECT), _layer((64,), 1, 7, 1, 3, REFLECT), _layer((64,), 3, 7, 1, 3, REFLECT)], [(2, 32, 32)], F_X3)
    # ... the row form of a stem (opt-in, plain bf16): M 23 | 24, 7 Cin <= 64 (Cin 9 | 10), pad 3, one segment
    add([_layer((3,), 23, 7, 1, 3, REFLECT), _layer((3,), 24, 7, 1, 3, REFLECT), _layer((9,), 64, 7, 1, 3, REFLECT),
         _layer((10,), 64, 7, 1, 3, REFLECT), _layer((2, 1), 64, 7, 1, 3, REFLECT), _layer((3,), 64, 7, 1, 3, ZERO, 1)],
        [(2, 32, 32), (1, 34, 70)], (BF16,))
    # ... the stride-2 3x3 encoder: the tile rule (M = 16 / 64 / 128 by Cin = 8 / 16 / 64), the space-to-depth form (Cin 7 | 8, odd
    # H / W, zero pad 1 only), concatenated sources
    add([_layer((c,), m, 3, 2, 1) for m in (16, 64, 128) for c in (8, 16, 64)], [(2, 32, 32)], ALL)
    add([_layer((7,), 64, 3, 2, 1), _layer((8,), 64, 3, 2, 1), _layer((128,), 256, 3, 2, 1), _layer((128, 128), 256, 3, 2, 1),
         _layer((64,), 128, 3, 2, 1, REFLECT), _layer((64,), 128, 3, 2, 1, ZERO, 1), _layer((64,), 47, 3, 2, 1), _layer((64,), 48, 3, 2, 1)],
        [(2, 32, 32), (1, 33, 32), (1, 32, 47)], F_X3)
    # ... the 3x3 stride-1 trunk: M 47 | 48, 127 | 128 | 256 (the 8-wave workgroup), Cin 31 | 32, 1 - 3 segments, a virtual
    # gradient, tile-aligned grids or not (g_direct of the fp32 kernel)
    add([_layer((64,), m, 3, 1, 1, REFLECT) for m in (47, 48, 127, 128, 256)] +
        [_layer((31,), 64, 3, 1, 1, REFLECT), _layer((32,), 64, 3, 1, 1, REFLECT), _layer((256, 16), 256, 3, 1, 1, REFLECT),
         _layer((48, 16, 32), 64, 3, 1, 1), _layer((16, 8, 7), 64, 3, 1, 1), _layer((64,), 64, 3, 1, 1, ZERO, 1),
         _layer((256,), 256, 3, 1, 1, REFLECT, 1)],
        [(2, 32, 32), (1, 33, 47)], ALL)
    # ... P against the number of stages: one-stage maps, many workgroups per tile
    add([_layer((64,), 64, 3, 1, 1), _layer((256,), 256, 3, 1, 1), _layer((512,), 512, 3, 1, 1)],
        [(1, 2, 32), (1, 4, 8), (1, 4, 64), (16, 64, 64)], ALL)
    # PatchGAN: the narrow first layer (1 | 2 channels: the LDS-staged form wants a power-of-two GW = W / 2 and whole row groups),
    # the 4x4 stride-2 body, the stride-1 tail and the one-channel head
    add([_layer((c,), 64, 4, 2, 1, mode, g) for c in (1, 2) for mode, g in ((ZERO, 0), (REFLECT, 0), (ZERO, 1))],
        [(2, 64, 64), (2, 40, 64), (2, 64, 48), (1, 33, 47), (1, 1024, 1024)], (FP32, BF16))
    add([_layer((2,), 20, 4, 2, 1), _layer((1,), 3, 4, 2, 1), _layer((3,), 64, 4, 2, 1), _layer((1, 1), 64, 4, 2, 1), _layer((2,), 64, 4, 2, 0)],
        [(2, 64, 64)], (FP32,))
    add([_layer((64,), 128, 4, 2, 1), _layer((128,), 256, 4, 2, 1), _layer((8,), 48, 4, 2, 1), _layer((4,), 64, 4, 2, 1),
         _layer((256,), 512, 4, 1, 1), _layer((512,), 1, 4, 1, 1), _layer((32,), 64, 4, 1, 1), _layer((16,), 64, 4, 1, 1)],
        [(2, 32, 32), (2, 31, 31)], ALL)
    # landmark encoder: one input channel (narrow 3x3), the 8 -> 16 -> 16 stride-2 layers (64 x 64 tiles), stride-1 layers
    add([_layer((1,), 8, 3, 1, 1), _layer((1,), 8, 3, 1, 1, REFLECT), _layer((1,), 8, 3, 1, 1, ZERO, 1), _layer((1,), 20, 3, 1, 1),
         _layer((2,), 8, 3, 1, 1), _layer((8,), 16, 3, 2, 1), _layer((16,), 16, 3, 2, 1), _layer((16,), 32, 3, 1, 1),
         _layer((1,), 8, 3, 2, 1)],
        [(2, 64, 64), (1, 33, 47), (1, 300, 300)], F_X3)
    # the forward pass's split copies: every form of carrying them, on the layers both xs routes serve and on those they refuse
    # (a segment or M off the octet grid, 4x4 in plain bf16, 7x7, the fp32 kernel)
    xs_layers = [((256,), 256, 3, 1, 1, REFLECT), ((256, 16), 256, 3, 1, 1, REFLECT), ((36,), 64, 3, 1, 1, ZERO), ((40,), 52, 3, 1, 1, ZERO),
                 ((64, 12), 64, 3, 1, 1, ZERO), ((256,), 512, 4, 1, 1, ZERO), ((64,), 128, 3, 2, 1, ZERO), ((64,), 128, 4, 2, 1, ZERO),
                 ((32, 32), 128, 3, 2, 1, ZERO), ((12,), 64, 3, 2, 1, ZERO), ((64,), 52, 3, 2, 1, ZERO)]
    add([_layer(s, m, k, st, p, mode, 0, xs) for s, m, k, st, p, mode in xs_layers for xs in XS_FORMS], [(2, 32, 32)], X3_16)
    add([_layer((64,), 64, 3, 1, 1, REFLECT, 1, (2, 1, 0)), _layer((3,), 64, 7, 1, 3, REFLECT, 0, (2, 1, 0)),
         _layer((16,), 32, 3, 1, 1, ZERO, 0, (2, 1, 0)), _layer((64,), 128, 3, 2, 1, ZERO, 0, (2, 1, 1))], [(2, 32, 32), (1, 33, 47)], ALL)
    # ... both sides of the 32-bit slot index of a split copy: the gradient's, a source's, the space-to-depth view's
    add([_layer((64,), 512, 3, 1, 1, ZERO, 0, (2, 1, 0)), _layer((512,), 64, 3, 1, 1, ZERO, 0, (2, 1, 0))], [(255, 256, 256), (256, 256, 256)],
        (BF16X3,))
    add([_layer((256,), 64, 3, 2, 1, ZERO, 0, (2, 0, 1)), _layer((64,), 1024, 3, 2, 1, ZERO, 0, (2, 0, 1))], [(511, 256, 256), (512, 256, 256)],
        (BF16X3,))
    # descriptors that must be refused: kernel size, stride, the grid, a reflection pad as large as the map, segment counts,
    # a segment without channels, sizes that are not positive
    add([_layer((64,), 64, 5, 1, 2), _layer((64,), 64, 1, 1, 0), _layer((64,), 64, 3, 3, 1), _layer((64,), 64, 7, 2, 3), _layer((64,), 64, 4, 3, 1),
         _layer((64,), 64, 3, 1, 1, ZERO, 0, NO_XS, 1), _layer((64,), 64, 3, 1, 0), _layer((1,), 8, 3, 1, 1, ZERO, 0, NO_XS, -1),
         _layer((64,), 64, 3, 1, 8, REFLECT), _layer((64,), 64, 7, 1, 9, REFLECT), _layer((64,), 64, 5, 1, 9, REFLECT),
         _layer((), 64, 3, 1, 1), _layer((64, 64, 64), 64, 3, 1, 1, ZERO, 0, NO_XS, 0, 4), _layer((64, 0), 64, 3, 1, 1),
         _layer((64, -8), 64, 3, 1, 1), _layer((64,), 0, 3, 1, 1)], [(1, 8, 8)], ALL)
    add([_layer((64,), 64, 3, 1, 1)], [(0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8)], (BF16X3,))
    return rows


def _desc(prec, layer, shape, probe=False):
    from animateportrait_amd import _capi
    segs, m, k, stride, pad, mode, g, (parts, xs_plain, xs_s2d), grid, nsrc = layer
    d = _capi.ApWgradDesc()
    d.N, d.H, d.W = shape
    d.M, d.K, d.stride, d.pad, d.pad_mode, d.nsrc, d.precision = m, k, stride, pad, mode, nsrc, prec
    d.GH, d.GW = (d.H + 2 * pad - k) // stride + 1 + grid, (d.W + 2 * pad - k) // stride + 1
    d.g.data, d.g.C, d.g.act = SOME_POINTER, m, 0
    if g:
        d.g.mean, d.g.rstd, d.g.act = SOME_POINTER, SOME_POINTER, 1
    for i, c in enumerate(segs):
        d.src[i].data, d.src[i].C = SOME_POINTER, c
        if xs_plain:
            d.src_xs[i] = SOME_POINTER
    if xs_s2d:
        d.src_xs_s2d = SOME_POINTER
    d.xs_parts = parts
    if probe:
        d.src[0].data, d.src[0].mean, d.src[0].rstd = None, SOME_POINTER, None
    return d


def answers(lib, prec, layer, shape):
    """What the planner says about one descriptor: [workspace floats (or the refusal code), rc of gt_dims, dims, xs_ok, xs route]"""
    ref = ctypes.byref(_desc(prec, layer, shape))
    dims = (ctypes.c_int32 * 3)(-1, -1, -1)
    ws = lib.ap_conv2d_wgrad_workspace_floats(ref)
    rc = lib.ap_conv2d_wgrad_gt_dims(ref, dims)
    ok = lib.ap_conv2d_wgrad_xs_ok(ref)
    route = None
    if ws >= 0:
        # refused by the argument validation either way: nothing is launched and no pointer is followed
        probe = lib.ap_conv2d_wgrad(ctypes.byref(_desc(prec, layer, shape, probe=True)), SOME_POINTER, SOME_POINTER, None)
        err = lib.ap_last_error()
        assert probe == -1 and (b'null data' in err or b'mean/rstd mismatch' in err), (probe, err)
        route = 0 if b'null data' in err else 1
    return [ws, rc, list(dims), ok, route]


# the shape-driven plan queries of the edge layers
def _shape_sweep():
    def grid(*axes):
        out = [()]
        for a in axes:
            out = [o + (v,) for o in out for v in a]
        return out

    k7 = grid((0, 1, 300), (16, 32, 64), (1, 2, 3), (3, 4, 256), (8, 16, 250, 256, 272), (0, 1))
    d0 = grid((0, 1, 300), (32, 64), (1, 2, 3), (0, 2, 63, 256), (16, 32, 48, 448, 512, 544))
    final = grid((0, 1, 2), (0, 16, 32, 64), (0, 1, 16, 64, 100, 256), (1, 16, 20, 64, 65, 256))
    head = grid((0, 1), (16, 32, 48, 512), (1, 2, 4, 6, 30, 34, 35), (1, 2, 30, 34, 35, 192, 193, 289, 290))
    d0f = grid((0, 1, 2), (1, 2, 3), (32, 64), (0, 2, 3, 64), (4, 8, 10, 64, 256, 260))
    return {'k7': k7, 'd0': d0, 'final_wgrad': final, 'final_dgrad': grid((0, 1, 2), (16, 32, 64), (0, 1, 64), (8, 16, 40, 256, 272)),
            'head_dgrad': head, 'd0_fwd': d0f}


def shape_answers(lib, name, a):
    if name == 'k7':
        return [lib.ap_wgrad_k7_bf16_ok(*a), lib.ap_wgrad_k7_bf16_workspace_floats(*a)]
    if name == 'd0':
        return [lib.ap_wgrad_d0_bf16_ok(*a), lib.ap_wgrad_d0_bf16_workspace_floats(*a)]
    if name == 'final_wgrad':
        return [lib.ap_conv_final_wgrad_workspace_floats(*a)]
    if name == 'final_dgrad':
        return [lib.ap_conv_final_dgrad_bf16_ok(*a), lib.ap_conv_final_dgrad_bf16_workspace_floats(*a)]
    if name == 'head_dgrad':
        return [lib.ap_conv_head_dgrad_bf16_ok(*a)]
    return [lib.ap_conv_d0_fwd_bf16_ok(*a)]


def _table(lib):
    return [answers(lib, p, lay, shp) for p, lay, shp in sweep()]


def _shape_table(lib):
    return {name: [[list(a), shape_answers(lib, name, a)] for a in args] for name, args in _shape_sweep().items()}


def _listed(p, lay, shp):
    return [p, [list(lay[0])] + [list(v) if isinstance(v, tuple) else v for v in lay[1:]], list(shp)]


def _use(env, setenv, delenv):
    from animateportrait_amd import ops
    for v in ops.plan_switch_names():      # every environment switch a route decision reads: make_wgrad_plan's and the xs predicates' among them
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
    return [r[col] if r[col] is not None else r[3] for r in golden['descriptors']]


@pytest.mark.parametrize('config', CONFIG_ORDER)
def test_wgrad_plans_match_the_recorded_table(lib, golden, monkeypatch, config):
    _use(CONFIGS[config], monkeypatch.setenv, lambda v: monkeypatch.delenv(v, raising=False))
    rows = sweep()
    assert [_listed(*r) for r in rows] == [r[:3] for r in golden['descriptors']] and len(rows) >= 250
    got, want = _table(lib), _recorded(golden, config)
    bad = [(r[:3], g, w) for r, g, w in zip(golden['descriptors'], got, want) if g != w]
    assert not bad, '%d of %d plans differ; first (descriptor, got, recorded): %r' % (len(bad), len(got), bad[0])


def test_edge_layer_plans_match_the_recorded_table(lib, golden, monkeypatch):
    _use({}, monkeypatch.setenv, lambda v: monkeypatch.delenv(v, raising=False))
    got = _shape_table(lib)
    assert sorted(got) == sorted(golden['shapes'])
    for name in got:
        assert [r[0] for r in got[name]] == [r[0] for r in golden['shapes'][name]], name
        bad = [(g[0], g[1], w[1]) for g, w in zip(got[name], golden['shapes'][name]) if g != w]
        assert not bad, '%s: %d of %d answers differ; first (arguments, got, recorded): %r' % (name, len(bad), len(got[name]), bad[0])


def test_the_sweep_reaches_every_family_and_refusal(golden):
    """The golden table is only a pin if it exercises the selection: both answers of gt_dims and of the xs predicates, every refusal
    code, both answers of each shape predicate, and an effect of every switch."""
    base = _recorded(golden, 'default')
    assert {a[1] for a in base} >= {0, 1}
    assert {a[3] for a in base} == {0, 1} and {a[4] for a in base} == {0, 1, None}
    assert {a[0] for a in base if a[0] < 0} == {-1, -2} and {a[1] for a in base} == {0, 1, -1, -2}
    assert all((a[0] < 0) == (a[1] < 0) and (a[1] < 0 or a[3] == 0 or a[1] == 1) for a in base)     # (xs_ok only on the bf16 GEMM plan)
    for name in CONFIG_ORDER[1:]:
        assert _recorded(golden, name) != base, name
    # the wide (128-channel tile) and plain forms of the bf16 GEMM, the row form and the space-to-depth form show in the dims
    assert {a[2][2] for a in base if a[1] == 1} >= {64, 128, 256}
    assert any(a[1] == 0 and r[1] == 1 for a, r in zip(base, _recorded(golden, 'rows')))           # (the opt-in row form)
    for name, col in (('k7', 0), ('d0', 0), ('final_dgrad', 0), ('head_dgrad', 0), ('d0_fwd', 0)):
        assert {r[1][col] for r in golden['shapes'][name]} == {0, 1}, name
    for name, col in (('k7', 1), ('d0', 1), ('final_wgrad', 0), ('final_dgrad', 1)):               # workspace sizes and refusals
        vals = [r[1][col] for r in golden['shapes'][name]]
        assert any(v > 0 for v in vals) and any(v < 0 for v in vals), name


if __name__ == '__main__' and '--record' in sys.argv:
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from animateportrait_amd import _capi
    tables = []
    for name in CONFIG_ORDER:
        _use(CONFIGS[name], os.environ.__setitem__, lambda v: os.environ.pop(v, None))
        tables.append(_table(_capi.lib()))
    _use({}, os.environ.__setitem__, lambda v: os.environ.pop(v, None))
    rows = [_listed(p, lay, shp) + [a[0]] + [b if b != a[0] else None for b in a[1:]] for (p, lay, shp), a in zip(sweep(), zip(*tables))]
    shapes = _shape_table(_capi.lib())
    with open(GOLDEN, 'w') as f:
        f.write('{"descriptors": [\n' + ',\n'.join(json.dumps(r, separators=(',', ':')) for r in rows) + '\n],\n"shapes": {\n')
        f.write(',\n'.join('"%s": [\n%s\n]' % (n, ',\n'.join(json.dumps(r, separators=(',', ':')) for r in shapes[n])) for n in shapes))
        f.write('\n}}\n')
    print('recorded', len(rows), 'plans and', sum(len(v) for v in shapes.values()), 'edge-layer answers in', GOLDEN)
