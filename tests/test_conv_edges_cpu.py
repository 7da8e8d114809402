"""CPU (-m "not gpu"): the reach of tests/test_conv_edges_gpu.py.  Without a device the planner and the launchers assume 256
compute units, the MI355X's count, so ap_conv2d_fwd_route answers here what it answers there: every route a GPU case states must
be the query's answer, and the stated routes together must name every kernel word of ap_conv2d_fwd_route_names -- the fixed
instantiation lists of the small families and the registries of csrc/conv_plan.hip.  A kernel added later without a case fails
here.

Five entries have no case because no descriptor reaches them; test_the_entries_without_a_case_are_unreachable sweeps each rule
through the query, and the day a rule changes it fails and the entry needs its case.
  ConvCfg<4,1,7,2,2,2,2>, ConvCfg<8,1,7,2,2,2,2>, ConvCfg<8,1,7,1,2,4,2>: pick_igemm halves the channel chunk until the LDS tile fits
      72 KB; one 7x7 weight block of 49 x CI x CO_TILE floats alone is 98 KB at CI x CO_TILE = 4 x 128 and 8 x 64, 196 KB at 8 x 128.
  ConvCfg<8,2,4,2,2,2,2>: likewise, 16 x 8 x 128 floats = 64 KB of weights plus the 8-channel activation tile of a stride-2 4x4.
  Bf3Cfg<1,7,1,2,4,4,0,1>: pick_bf3 gives the row form of a stem the SHORTEST row tile, whatever the map."""
import ctypes

import pytest

import test_conv_edges_gpu as T
import test_conv_plan_cpu as P

UNREACHABLE = T.IGEMM_UNREACHABLE | {'Bf3Cfg<1,7,1,2,4,4,0,1>'}


@pytest.fixture
def plan_env(monkeypatch):
    from animateportrait_amd import ops
    for v in ops.plan_switch_names():
        monkeypatch.delenv(v, raising=False)
    return monkeypatch


def _names():
    from animateportrait_amd import _capi
    buf = ctypes.create_string_buffer(8192)
    assert _capi.lib().ap_conv2d_fwd_route_names(buf, len(buf)) == 0
    return buf.value.decode().split()


def _kernel_words(route):
    return {w for w in route.replace(';', ' ').split() if '<' in w or w == 'tapgemm'}


@pytest.mark.parametrize('case', T.CASES, ids=[k.name for k in T.CASES])
def test_stated_route_is_the_querys_answer(plan_env, case):
    assert T.query(case) == (case.refused if case.refused else case.route)


def test_cases_name_every_kernel_word(plan_env):
    names = _names()
    assert len(names) == len(set(names)) == 3 + 6 + 4 + 2 + 1 + 54 + 10 + 2 and UNREACHABLE < set(names)
    routes = [k.route for k in T.CASES if not k.refused]
    named = set().union(*map(_kernel_words, routes))
    assert named <= set(names), named - set(names)
    assert set(names) - named == UNREACHABLE, 'kernel words without a GPU case: %s' % sorted(set(names) - named - UNREACHABLE)
    # both arithmetic modes on every split-bf16 kernel a case names, and every launch-time word
    bf3 = {(g.split()[1], g.split()[3]) for r in routes for g in r.split('; ') if g.startswith('bf3 ')}
    assert {k for k, a in bf3 if a == 'x3'} == {k for k, a in bf3 if a == 'b16'} == {n for n in names if n[:3] in ('Bf3', 'Ph4')} - UNREACHABLE
    words = {w for r in routes for w in r.replace(';', ' ').split()}
    assert {'staged', 'gather', 'ob16', 's2d3=ct', 's2d3=mask', 'phases=ph4', 'phases=fused', 'phases=4launch'} <= words
    assert {T.family(r) for r in routes} == {'tsmall', 'head', 'small', 'direct', 'tapgemm', 'igemm', 'bf3'}
    assert {(k.form, bool(k.refused)) for k in T.CASES} == {(f, r) for f in (T.PLAIN, T.OCTET, T.OB16) for r in (False, True)} - {(T.PLAIN, True)}
    # more tiles than workgroups by default, and the statistics fall-back of the two narrow-output kernels
    assert any(k.stats and k.route.startswith('igemm') and k.cout == 1 and k.k == 4 for k in T.CASES)
    assert any(k.stats and k.route.startswith('igemm') and k.tr and k.cout <= 4 and k.k == 4 for k in T.CASES)


def test_every_split_bf16_case_has_a_ragged_walk(plan_env):
    """item 5 of the GPU test is never a launch compared with itself: every launch of every split-bf16 case has at least three
    tiles, and one workgroup count below them divides none"""
    plan_env.setenv('APAMD_BF3_BLOCKS', '1000000')                  # (the cap: one workgroup per tile)
    walked = set()
    for case in T.CASES:
        if case.refused or T.family(case.route) != 'bf3':
            continue
        tiles = T.workgroups(T.query(case))
        ragged = T.a_ragged_count(tiles[0])
        assert min(tiles) >= 3 and ragged is not None and all(t % ragged for t in tiles), (case.name, tiles)
        walked |= {(g.split()[1], g.split()[3], 's2d3=ct' in g) for g in case.route.split('; ')}
    names = {n for n in _names() if n[:3] in ('Bf3', 'Ph4')} - UNREACHABLE
    assert {(n, a, False) for n in names for a in ('x3', 'b16')} <= walked
    assert {('Bf3Cfg<1,0,1,2,4,2,4>', a, True) for a in ('x3', 'b16')} <= walked        # the compile-time-tap instantiations


def _route(d, stats=0, form=0, n=512):
    from animateportrait_amd import _capi
    buf = ctypes.create_string_buffer(n)
    rc = _capi.lib().ap_conv2d_fwd_route(ctypes.byref(d), stats, form, buf, n)
    return rc, buf.value.decode()


def test_route_query_refusals_and_buffer(plan_env):
    from animateportrait_amd import _capi
    lib = _capi.lib()
    d = P._desc(T.X3, P._layer((64,), 64, 3, 1, 1, T.REFLECT), (2, 32, 32))
    buf = ctypes.create_string_buffer(128)
    assert lib.ap_conv2d_fwd_route(ctypes.byref(d), 0, 0, None, 64) == -1 and lib.ap_conv2d_fwd_route(ctypes.byref(d), 0, 0, buf, 0) == -1
    assert lib.ap_conv2d_fwd_route(None, 0, 0, buf, 128) == -1
    # a split-bf16 layer without prepared sources is refused as the launcher refuses it
    assert _route(d)[0] == -1 and b'presplit' in lib.ap_last_error()
    d.presplit = 1
    assert _route(d) == (0, 'bf3 Bf3Cfg<1,3,1,2,4,1> taps=9 x3 wg=16')
    assert _route(d, n=4) == (0, 'bf3')                                                 # truncated, terminated
    assert _route(d, form=5)[0] == -1 and _route(d, form=-1)[0] == -1 and _route(d, stats=1, form=3)[0] == -1
    # the forms: octet and a window are taken, a bf16 store only in plain-bf16 arithmetic; a window of a multi-launch plan is not
    assert _route(d, form=1)[0] == 0 and _route(d, form=3) == _route(d) and _route(d, form=2)[0] == _route(d, form=4)[0] == -2
    d.precision = T.B16
    assert _route(d, form=2) == _route(d, form=4) == (0, 'bf3 Bf3Cfg<1,3,1,2,4,1> taps=9 b16 ob16 wg=16') and _route(d, form=1)[0] == -2
    t = P._desc(T.X3, P._layer((256,), 128, 3, 2, 1, T.ZERO, 1, 1, T.IOHW), (2, 16, 16))
    t.presplit = 1
    assert _route(t)[0] == 0 and _route(t, form=3)[0] == -2 and b'single-launch' in lib.ap_last_error()
    # presplit on a layer that does not take split sources; mean without rstd; an activation out of range
    f = P._desc(T.FP32, P._layer((64,), 64, 3, 1, 1), (1, 8, 8))
    f.presplit = 1
    assert _route(f)[0] == -1
    f.presplit = 0
    f.src[0].mean = 0x1000
    assert _route(f)[0] == -1 and b'mean and rstd' in lib.ap_last_error()
    f.src[0].rstd = 0x1000
    assert _route(f)[0] == 0
    f.src[0].act = 3
    assert _route(f)[0] == -1
    # the workgroup knob is read as the launcher reads it
    plan_env.setenv('APAMD_BF3_BLOCKS', '5')
    d.precision = T.X3
    assert _route(d)[1].endswith(' wg=5')
    assert lib.ap_conv2d_fwd_route_names(buf, 16) == -1 and lib.ap_conv2d_fwd_route_names(None, 16) == -1


def test_refusal_codes_equal_the_entry_points(plan_env):
    """every descriptor of test_conv_plan_cpu.py's sweep the planner refuses: the query answers the code ap_conv2d_fwd answers (for
    non-null arguments; nothing is launched for a refused descriptor, so this runs without a device)"""
    from animateportrait_amd import _capi
    lib = _capi.lib()
    some = ctypes.cast(ctypes.create_string_buffer(64), ctypes.POINTER(ctypes.c_float))
    refused = 0
    for prec, layer, shape in P.sweep():
        d = P._desc(prec, layer, shape)
        ho, wo = ctypes.c_int32(), ctypes.c_int32()
        rc = lib.ap_conv2d_out_size(ctypes.byref(d), ctypes.byref(ho), ctypes.byref(wo))
        if rc == 0:
            continue
        refused += 1
        for i in range(d.nsrc if 0 < d.nsrc <= 3 else 0):
            d.src[i].data = 0x1000
        assert _route(d)[0] == rc == lib.ap_conv2d_fwd(ctypes.byref(d), some, some, some, None, None), (prec, layer, shape)
        assert _route(d, form=1)[0] == rc == lib.ap_conv2d_fwd_octet(ctypes.byref(d), some, some, some, None, None)
        assert _route(d, form=2)[0] == rc == lib.ap_conv2d_fwd_bf16out(ctypes.byref(d), some, some, some, None, None)
    assert refused >= 20


def test_the_entries_without_a_case_are_unreachable(plan_env):
    picked = set()
    segs = [(c,) for c in list(range(1, 34)) + [40, 48, 64, 96, 128, 256]] + [(8, 8), (8, 8, 8), (4, 4), (16, 8), (5, 3), (64, 64)]
    for k, stride in ((7, 1), (4, 2)):
        for cout in (5, 8, 31, 32, 47, 48, 64, 95, 96, 128, 129, 256):
            for s in segs:
                for shape in ((1, 9, 33), (2, 64, 64)):
                    rc, r = _route(P._desc(T.FP32, P._layer(s, cout, k, stride, (k - 1) // 2), shape))
                    assert rc == 0
                    picked |= _kernel_words(r)
    assert not picked & UNREACHABLE, picked & UNREACHABLE
    assert {'ConvCfg<8,1,7,1,1,4,2>', 'ConvCfg<4,1,7,1,2,4,2>', 'ConvCfg<2,1,7,2,2,2,2>', 'ConvCfg<4,2,4,2,2,2,2>', 'ConvCfg<8,2,4,1,2,4,2>'} <= picked
    rows = set()
    for prec in (T.X3, T.B16):
        for cout in (32, 64, 96, 256):
            for shape in ((1, 4, 16), (1, 9, 33), (1, 256, 256), (16, 256, 256), (64, 64, 64)):
                for mode in (T.ZERO, T.REFLECT):
                    d = P._desc(prec, P._layer((32,), cout, 7, 1, 3, mode, kh=1), shape)
                    d.presplit = 1
                    rc, r = _route(d)
                    assert rc == 0
                    rows |= _kernel_words(r)
    assert rows == {'Bf3Cfg<1,7,1,1,4,2,0,1>'}, rows
