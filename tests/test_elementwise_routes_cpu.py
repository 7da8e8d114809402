"""CPU (-m "not gpu"): which kernel of csrc/instnorm_bwd.hip / csrc/act_bwd.hip a plane geometry takes, as ap_instnorm_bwd_route and
ap_act_bwd_route state it -- the launchers switch on the same selectors.  Every boundary of the dispatch is walked with a shape on
each side of it; tests/test_elementwise_bwd_gpu.py runs the kernels and states, per case, the route named here.  Also checked without
a GPU: the refusals that need no launch, the slice counts of the two-stage bias gradient, that the GPU cases cover every route name,
and that their inputs keep the normalised activation away from the activation's kink while the fp32 formula meets the GPU bars."""
import ctypes

import pytest
import torch

import test_elementwise_bwd_gpu as G

AP_ERR_INVALID, AP_ERR_UNSUPPORTED = -1, -2
BF16 = 0x100

INBWD_NAMES = ['small', 'small<g2>', 'vec<256>', 'vec<256,g2>', 'vec<1024>', 'vec<1024,g2>', 'fold1<256>', 'fold1<256,g2>',
               'fold1<1024>', 'fold1<1024,g2>', 'general<256>', 'general<1024>', 'big', 'big<fold>', 'big<bf16>', 'reduce_apply']
ACT_NAMES = ['act_fold1', 'act_generic']


@pytest.fixture(scope='module')
def lib():
    from animateportrait_amd import _capi
    return _capi.lib()


def _name(fn, *args):
    buf = ctypes.create_string_buffer(64)
    rc = fn(*args, buf, 64)
    return buf.value.decode() if rc == 0 else rc


# ap_instnorm_bwd_route(g1_pad, has_g2, act_bits, H, W): (arguments, name or error code)
INBWD_ROUTES = [
    # unfolded, up to 1024 pixels: whole 16-byte groups or not
    ((0, 0, 0, 1, 1), 'small'),
    ((0, 1, 1, 1, 1), 'small<g2>'),
    ((0, 0, 1, 1, 1023), 'small'),                 # H W = 1023
    ((0, 1, 2, 31, 33), 'small<g2>'),
    ((0, 0, 1, 2, 2), 'vec<256>'),
    ((0, 0, 1, 32, 32), 'vec<256>'),               # 1024
    ((0, 1, 1, 2, 514), 'vec<256,g2>'),            # 1028 with W % 4 = 2: only H W % 4 counts without a fold
    ((0, 0, 1, 25, 41), 'general<256>'),           # 1025: beyond the small kernel, not whole groups
    ((0, 1, 1, 25, 41), 'general<256>'),           # (the general kernels take g2 at run time)
    # 4096 | 4100
    ((0, 0, 0, 63, 65), 'general<256>'),           # 4095
    ((0, 0, 0, 64, 64), 'vec<256>'),               # 4096
    ((0, 1, 0, 1024, 4), 'vec<256,g2>'),
    ((0, 0, 0, 17, 241), 'general<1024>'),         # 4097
    ((0, 0, 0, 41, 100), 'vec<1024>'),             # 4100
    ((0, 1, 0, 41, 100), 'vec<1024,g2>'),
    # 16380 | 16384 | 16388
    ((0, 0, 2, 126, 130), 'vec<1024>'),            # 16380
    ((0, 0, 2, 127, 129), 'general<1024>'),        # 16383
    ((0, 0, 2, 128, 128), 'vec<1024>'),            # 16384
    ((0, 0, 2, 5, 3277), 'reduce_apply'),          # 16385: past the one-workgroup kernels, no 16-byte rows
    ((0, 0, 2, 4097, 4), 'big'),                   # 16388
    ((0, 1, 2, 4097, 4), 'big'),
    ((0, 0, 2, 2, 8194), 'reduce_apply'),          # 16388 with W % 4 = 2
    ((0, 0, 2, 8194, 2), 'reduce_apply'),          # ... with W < 4
    # 65536 | 65540
    ((0, 0, 1, 256, 256), 'big'),                  # 65536
    ((0, 0, 1, 16384, 4), 'big'),
    ((0, 0, 1, 16385, 4), 'reduce_apply'),         # 65540
    ((0, 0, 1, 257, 256), 'reduce_apply'),
    ((0, 1, 1, 300, 300), 'reduce_apply'),
    # the pad-1 fold: W % 4 == 0, W >= 8, H >= 3
    ((1, 0, 1, 3, 8), 'fold1<256>'),
    ((1, 1, 1, 3, 8), 'fold1<256,g2>'),
    ((1, 0, 1, 2, 8), 'general<256>'),             # H = 2
    ((1, 0, 1, 3, 4), 'general<256>'),             # W = 4
    ((1, 0, 1, 2, 4), 'general<256>'),
    ((1, 0, 1, 5, 4), 'general<256>'),
    ((1, 0, 1, 3, 10), 'general<256>'),            # W % 4 = 2
    ((1, 0, 1, 31, 33), 'general<256>'),           # 1023 pixels with a fold: not the small kernel's
    ((1, 0, 1, 30, 30), 'general<256>'),
    ((1, 0, 1, 64, 64), 'fold1<256>'),             # 4096
    ((1, 0, 1, 65, 64), 'fold1<1024>'),            # 4160
    ((1, 1, 1, 128, 128), 'fold1<1024,g2>'),       # 16384
    ((1, 0, 1, 70, 70), 'general<1024>'),
    ((1, 0, 1, 4097, 4), 'big<fold>'),             # 16388 (the big kernel takes W = 4)
    ((1, 0, 1, 132, 128), 'big<fold>'),
    ((1, 1, 1, 256, 256), 'big<fold>'),
    ((1, 0, 1, 130, 127), 'reduce_apply'),
    ((1, 0, 1, 16385, 4), 'reduce_apply'),
    # pads 2 and 3
    ((2, 0, 0, 9, 10), 'general<256>'),
    ((2, 0, 0, 9, 12), 'general<256>'),            # W % 4 == 0 makes no 16-byte route for pad 2
    ((3, 0, 0, 40, 44), 'general<256>'),
    ((3, 0, 0, 4, 8), 'general<256>'),             # pad = H - 1
    ((3, 1, 0, 96, 96), 'general<1024>'),
    ((2, 0, 0, 130, 128), 'big<fold>'),
    ((3, 0, 0, 256, 256), 'big<fold>'),
    ((3, 0, 0, 2100, 8), 'big<fold>'),
    ((3, 0, 0, 130, 127), 'reduce_apply'),
    # dy stored as bf16: the unfolded big-plane kernel only
    ((0, 0, 1 | BF16, 132, 128), 'big<bf16>'),
    ((0, 1, 2 | BF16, 256, 256), 'big<bf16>'),
    ((0, 0, 0 | BF16, 4097, 4), 'big<bf16>'),
    ((0, 0, 1 | BF16, 128, 128), AP_ERR_UNSUPPORTED),      # 16384
    ((0, 0, 1 | BF16, 64, 64), AP_ERR_UNSUPPORTED),
    ((0, 0, 1 | BF16, 31, 31), AP_ERR_UNSUPPORTED),
    ((0, 0, 1 | BF16, 16385, 4), AP_ERR_UNSUPPORTED),      # 65540
    ((0, 0, 1 | BF16, 130, 127), AP_ERR_UNSUPPORTED),      # W % 4
    ((1, 0, 1 | BF16, 132, 128), AP_ERR_UNSUPPORTED),      # with a fold
    ((3, 0, 1 | BF16, 256, 256), AP_ERR_UNSUPPORTED),
    ((0, 0, 3 | BF16, 256, 256), AP_ERR_INVALID),          # the activation is judged first
    # activations
    ((0, 0, 3, 64, 64), AP_ERR_INVALID),
    ((0, 0, 4, 64, 64), AP_ERR_INVALID),
    ((0, 0, 0xff, 64, 64), AP_ERR_INVALID),
    # fold pads
    ((4, 0, 1, 4, 8), AP_ERR_INVALID),             # pad = H
    ((8, 0, 1, 9, 8), AP_ERR_INVALID),             # pad = W
    ((1, 0, 1, 1, 8), AP_ERR_INVALID),
    ((1, 0, 1, 8, 1), AP_ERR_INVALID),
    ((-1, 0, 1, 8, 8), AP_ERR_INVALID),
    ((7, 0, 1, 8, 8), 'general<256>'),
]

# ap_act_bwd_route(g1_pad, H, W)
ACT_ROUTES = [
    ((1, 3, 4), 'act_fold1'),
    ((1, 3, 8), 'act_fold1'),
    ((1, 64, 64), 'act_fold1'),
    ((1, 256, 256), 'act_fold1'),
    ((1, 2, 4), 'act_generic'),                    # H = 2
    ((1, 2, 8), 'act_generic'),
    ((1, 3, 6), 'act_generic'),                    # W % 4 = 2
    ((1, 3, 3), 'act_generic'),
    ((1, 182, 181), 'act_generic'),
    ((0, 3, 4), 'act_generic'),
    ((0, 16, 16), 'act_generic'),
    ((0, 256, 256), 'act_generic'),
    ((2, 9, 10), 'act_generic'),
    ((2, 9, 12), 'act_generic'),
    ((3, 12, 16), 'act_generic'),
    ((3, 4, 8), 'act_generic'),                    # pad = H - 1
    ((4, 4, 8), AP_ERR_INVALID),
    ((8, 9, 8), AP_ERR_INVALID),
    ((1, 1, 4), AP_ERR_INVALID),
    ((-1, 8, 8), AP_ERR_INVALID),
]


def _ids(rows):
    return ['p%d g%d a%x %dx%d' % a if len(a) == 5 else 'p%d %dx%d' % a for a, _ in rows]


@pytest.mark.parametrize('args,expect', INBWD_ROUTES, ids=_ids(INBWD_ROUTES))
def test_instnorm_bwd_route(lib, args, expect):
    assert _name(lib.ap_instnorm_bwd_route, *args) == expect
    if isinstance(expect, int):
        assert lib.ap_last_error()


@pytest.mark.parametrize('args,expect', ACT_ROUTES, ids=_ids(ACT_ROUTES))
def test_act_bwd_route(lib, args, expect):
    assert _name(lib.ap_act_bwd_route, *args) == expect


def test_route_names_need_a_buffer(lib):
    assert lib.ap_instnorm_bwd_route(0, 0, 1, 8, 8, None, 64) == AP_ERR_INVALID
    assert lib.ap_act_bwd_route(0, 8, 8, None, 64) == AP_ERR_INVALID
    buf = ctypes.create_string_buffer(4)
    assert lib.ap_instnorm_bwd_route(0, 0, 1, 300, 300, buf, 4) == 0 and buf.value == b'red'      # truncated, terminated


def test_the_selectors_return_the_listed_names_only(lib):
    """A sweep over plane sizes around every threshold, all pads, both g2 forms and the bf16 bit: the names that come back are the
    ones listed above, all of them."""
    sizes = [1, 2, 3, 4, 5, 8, 12, 31, 32, 33, 41, 64, 65, 100, 127, 128, 129, 130, 132, 256, 257, 300, 1023, 4097, 16385]
    seen_in, seen_act = set(), set()
    for h in sizes:
        for w in sizes:
            if h * w > 1 << 20:
                continue
            for pad in range(4):
                a = _name(lib.ap_act_bwd_route, pad, h, w)
                assert (a == AP_ERR_INVALID) == (pad > 0 and (pad >= h or pad >= w))
                if not isinstance(a, int):
                    seen_act.add(a)
                for g2 in (0, 1):
                    for bits in (1, 1 | BF16):
                        r = _name(lib.ap_instnorm_bwd_route, pad, g2, bits, h, w)
                        if not isinstance(r, int):
                            seen_in.add(r)
    assert seen_in == set(INBWD_NAMES) and seen_act == set(ACT_NAMES)
    assert {e for _, e in INBWD_ROUTES if isinstance(e, str)} == set(INBWD_NAMES)
    assert {e for _, e in ACT_ROUTES if isinstance(e, str)} == set(ACT_NAMES)


def test_every_route_is_the_stated_route_of_a_gpu_case(lib):
    stated = {c[0] for c in G.INBWD_CASES} | {c[0] for c in G.INBWD_BF16_CASES}
    assert stated == set(INBWD_NAMES)
    assert {c[0] for c in G.ACT_CASES} == set(ACT_NAMES)
    # ... and the statements are true (the GPU tests assert the same before they launch)
    for route, h, w, pad, act, two, nc in G.INBWD_CASES:
        assert _name(lib.ap_instnorm_bwd_route, pad, int(two), act, h, w) == route and nc >= 3
    for route, h, w, act, two, nc in G.INBWD_BF16_CASES:
        assert _name(lib.ap_instnorm_bwd_route, 0, int(two), act | BF16, h, w) == route and nc >= 3
    for route, h, w, pad, act, two, nc, _ in G.ACT_CASES:
        assert _name(lib.ap_act_bwd_route, pad, h, w) == route and nc >= 3
    for n, c, h, w, pad, act, two in G.ACT_BIAS_CASES:
        assert _name(lib.ap_act_bwd_route, pad, h, w) == 'act_generic'


_DUMMY = 1 << 20        # never dereferenced: every call below is refused before anything is launched


def test_plane_count_limits_are_refused_before_any_launch(lib):
    """N C is the grid's y (or x) extent: 1 .. 65535"""
    for nc in (0, -1, 65536, 1 << 20):
        assert lib.ap_instnorm_bwd(_DUMMY, 0, None, _DUMMY, _DUMMY, _DUMMY, 1, nc, 8, 8, _DUMMY, _DUMMY, None) == AP_ERR_UNSUPPORTED
        assert lib.ap_act_bwd(_DUMMY, 0, None, _DUMMY, 1, nc, 8, 8, _DUMMY, None) == AP_ERR_UNSUPPORTED
    for n, c in ((0, 3), (3, 0), (256, 256), (65536, 1), (1, 65536)):
        assert lib.ap_act_bwd_bias(_DUMMY, 0, None, _DUMMY, 1, n, c, 8, 8, _DUMMY, _DUMMY, _DUMMY, None) == AP_ERR_UNSUPPORTED
    # what the route functions refuse, the launchers refuse with the same code
    assert lib.ap_instnorm_bwd(_DUMMY, 4, None, _DUMMY, _DUMMY, _DUMMY, 1, 3, 4, 8, _DUMMY, _DUMMY, None) == AP_ERR_INVALID
    assert lib.ap_instnorm_bwd(_DUMMY, 0, None, _DUMMY, _DUMMY, _DUMMY, 3, 3, 4, 8, _DUMMY, _DUMMY, None) == AP_ERR_INVALID
    assert lib.ap_instnorm_bwd(_DUMMY, 0, None, _DUMMY, _DUMMY, _DUMMY, 1 | BF16, 3, 64, 64, _DUMMY, _DUMMY, None) == AP_ERR_UNSUPPORTED
    assert lib.ap_instnorm_bwd(_DUMMY, 1, None, _DUMMY, _DUMMY, _DUMMY, 1 | BF16, 3, 132, 128, _DUMMY, _DUMMY, None) == AP_ERR_UNSUPPORTED
    assert lib.ap_instnorm_bwd(_DUMMY, 0, None, None, _DUMMY, _DUMMY, 1, 3, 4, 8, _DUMMY, _DUMMY, None) == AP_ERR_INVALID
    assert lib.ap_act_bwd(_DUMMY, 4, None, _DUMMY, 1, 3, 4, 8, _DUMMY, None) == AP_ERR_INVALID
    assert lib.ap_act_bwd(_DUMMY, 0, None, _DUMMY, 4, 3, 4, 8, _DUMMY, None) == AP_ERR_INVALID
    assert lib.ap_act_bwd(_DUMMY, 0, None, None, 1, 3, 4, 8, _DUMMY, None) == AP_ERR_INVALID


@pytest.mark.parametrize('case', G.BIAS_WS_CASES, ids=lambda c: 'N%d C%d HW%d split%d' % c)
def test_bias_grad_slice_counts(lib, case):
    n, c, hw, split = case
    assert lib.ap_bias_grad_workspace_floats(n, c, hw) == n * c * split


def test_act_bwd_bias_workspace_is_one_float_per_block(lib):
    for n, c, h, w, _, _, _ in G.ACT_BIAS_CASES:
        assert lib.ap_act_bwd_bias_workspace_floats(n, c, h, w) == n * c * min(32, (h * w + 1023) // 1024)
    assert lib.ap_act_bwd_bias_workspace_floats(2, 3, 256, 256) == 6 * 32 == lib.ap_act_bwd_bias_workspace_floats(2, 3, 300, 300)
    assert lib.ap_act_bwd_bias_workspace_floats(0, 3, 8, 8) < 0


@pytest.mark.parametrize('case', G.INBWD_CASES + [(c[0], c[1], c[2], 0) + c[3:] for c in G.INBWD_BF16_CASES], ids=G.inbwd_id)
def test_gpu_case_inputs_stay_off_the_kink(case):
    """The construction of the GPU cases' inputs: after the move no |x^| is below 1e-3 (2e-3 up to the recomputed statistics), so
    fp32 and fp64 agree on every element's side of ReLU's kink; and the backward formula evaluated in fp32 on the CPU meets the bar
    the GPU test holds the kernel to, per plane -- the bar asks nothing the number format cannot give."""
    route, h, w, pad, act, two, nc = case
    p = G.inbwd_problem(h, w, pad, act, two, nc)
    assert p['y'].dtype == torch.float32 and bool(torch.isfinite(p['ref']).all())
    if h * w == 1:
        assert act == 0 and bool((p['ref'] == 0).all())
        return
    assert G.xhat_min(p['y']) >= 1e-3
    m, s = G.plane_stats(p['y'])
    # every plane kept its own mean and scale
    for i in range(nc):
        if h * w >= 64:
            assert abs(float(m.view(-1)[i]) - G.OFFSETS[i % 3]) < G.SCALES[i % 3] and 0.5 < float(s.view(-1)[i]) / G.SCALES[i % 3] < 1.5
    for e, sc in G.per_plane_errors(G.inbwd_formula_fp32(p, pad, act), p['ref']):
        assert e < 2e-5 * sc, (e, sc)


@pytest.mark.parametrize('case', G.ACT_CASES, ids=G.act_id)
def test_gpu_act_case_references(case):
    """ReLU / LeakyReLU cases hold exact zeros (and a negative zero) in the stored output, every plane both signs."""
    route, h, w, pad, act, two, nc, with_out = case
    p = G.act_problem(1, nc, h, w, pad, act, two, with_out)
    assert (p['out'] is None) == (not with_out) and bool(torch.isfinite(p['ref']).all())
    if act in (1, 2):
        assert bool((p['out'] == 0).any())
    if act != 0 and h * w >= 64:
        for i in range(nc):
            assert bool((p['out'][0, i] > 0).any()) and bool((p['out'][0, i] <= 0).any())
