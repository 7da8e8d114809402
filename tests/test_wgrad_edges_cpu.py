"""CPU (-m "not gpu"): the reach of tests/test_wgrad_edges_gpu.py.  Without a device the planner assumes 256 compute units, the
MI355X's count, so ap_conv2d_wgrad_route answers here what it answers there: every route a GPU case states must be the planner's
answer, and the stated routes together must name every entry of the four kernel tables of csrc/wgrad_launch.hip (kWgradKernels,
kWgradBf3Kernels, kWgradNarrowKernels, kWgradXsKernels) and every operand form, as ap_conv2d_wgrad_route_names lists them.  A
kernel added later without a case fails here.

Two entries have no case because no descriptor reaches them.  bf16gemm<7,split>+rows: bf16_gemm_view opens the row form of a stem
for AP_PRECISION_BF16 only, which runs the head-only instantiation.  igemm<2,3,64,256,1>: pick_igemm_tile walks the table in order and moves
to a later entry only if its padded M x Q grid is 30 % smaller than the pick's; the 64 x 64 entry stands before the 64 x 256 one
and its padded grid is never larger (same M tile, finer Q tile).  test_the_entries_without_a_case_are_unreachable sweeps both rules
through the query; the day a rule or the table order changes it fails and the entry needs its case."""
import ctypes

import pytest

import test_wgrad_edges_gpu as T

UNREACHABLE = {'igemm<2,3,64,256,1>', 'bf16gemm<7,split>+rows'}
SPLIT_T_FORMS = {'general', 'vec', 'pad_rows', 's2d_rows'}


@pytest.fixture
def plan_env(monkeypatch):
    from animateportrait_amd import ops
    for v in ops.plan_switch_names():
        monkeypatch.delenv(v, raising=False)
    return monkeypatch


def _names():
    from animateportrait_amd import _capi
    buf = ctypes.create_string_buffer(4096)
    assert _capi.lib().ap_conv2d_wgrad_route_names(buf, len(buf)) == 0
    names = buf.value.decode().split()
    return {n for n in names if '<' in n}, {n for n in names if '<' not in n}


@pytest.mark.parametrize('case', T.CASES, ids=[k.name for k in T.CASES])
def test_stated_route_is_the_planners_answer(plan_env, case):
    for k, v in case.env.items():
        plan_env.setenv(k, v)
    assert T.query(case) == case.route


def test_cases_name_every_kernel_table_entry_and_operand_form():
    kernels, forms = _names()
    assert len(kernels) == 8 + 10 + 5 + 6 and UNREACHABLE < kernels and SPLIT_T_FORMS < forms
    words = [w for k in T.CASES for w in k.route.split()]
    named = {w for w in words if '<' in w}
    assert named <= kernels, named - kernels
    assert kernels - named == UNREACHABLE, 'kernel table entries without a GPU case: %s' % sorted(kernels - named - UNREACHABLE)
    seen = {w.split('=', 1)[1] for w in words if w[:2] in ('g=', 'a=')}
    assert seen == forms, 'operand forms without a GPU case: %s' % sorted(forms ^ seen)
    # each of the four operand-preparation kernels on the operand it can serve: the gradient is never padded, so only the shifted
    # operand takes the two row forms
    assert {w[2:] for w in words if w[:2] == 'a='} >= SPLIT_T_FORMS - {'vec'} and {w[2:] for w in words if w[:2] == 'g='} >= {'vec', 'general'}
    # both arithmetic forms and the 8-wave workgroup on every view they exist for; every family under the three stage splits
    assert {T.family(k.route) for k in T.CASES} == {'narrow', 'bf16gemm', 'igemm', 'final'}
    assert {k.via for k in T.CASES} == {'wgrad', 'pre', 'xs', 'final', 'few'}


def test_route_query_refusals_and_buffer(plan_env):
    from animateportrait_amd import _capi, ops
    lib = _capi.lib()
    buf = ctypes.create_string_buffer(128)
    case = T.CASES[1]
    g, forms = T.expected_form(case, 'g'), [T.expected_form(case, 0)]
    d = ops._wgrad_plan_desc(case.k, case.stride, case.pad, case.mode, g.shape, forms, case.prec)
    d.g.data = 0x1000
    assert lib.ap_conv2d_wgrad_route(ctypes.byref(d), None, 64) == -1 and lib.ap_conv2d_wgrad_route(ctypes.byref(d), buf, 0) == -1
    assert lib.ap_conv2d_wgrad_route(ctypes.byref(d), buf, 9) == 0 and buf.value == b'bf16gemm'        # truncated, terminated
    assert lib.ap_conv2d_wgrad_route(None, buf, 128) == -1
    d.K = 5                                                                                            # the launcher's refusal
    assert lib.ap_conv2d_wgrad_route(ctypes.byref(d), buf, 128) == lib.ap_conv2d_wgrad_workspace_floats(ctypes.byref(d)) == -2
    d.K = case.k
    # a bf16-stored source is read by the padded-row kernel only: W = 47 is refused as the launcher refuses it
    d.src[0].act |= 0x100
    assert lib.ap_conv2d_wgrad_route(ctypes.byref(d), buf, 128) == 0 and b'a=pad_rows' in buf.value
    d.W, d.GW = 47, 47
    assert lib.ap_conv2d_wgrad_route(ctypes.byref(d), buf, 128) == -2 and b'padded-row form' in lib.ap_last_error()
    assert lib.ap_conv2d_wgrad_route_names(buf, 16) == -1 and lib.ap_conv2d_wgrad_route_names(None, 16) == -1


def test_the_entries_without_a_case_are_unreachable(plan_env):
    from animateportrait_amd import ops
    import torch
    picked = set()
    for m in (1, 8, 16, 47, 48, 63, 64, 65, 96, 127, 128, 129, 192, 256, 512):
        for cin in list(range(1, 41)) + [48, 56, 57, 64, 85, 86, 96, 114, 128, 256, 512]:
            for prec in (T.FP32, T.X3):
                g = ops.Form((1, m, 8, 8), torch.float32, False, 0, False, False, False, False)
                f = ops.Form((1, cin, 15, 16), torch.float32, False, 0, False, False, False, False)      # (odd H: no space-to-depth view)
                picked.add(ops.wgrad_kernel_route(3, 2, 1, T.ZERO, g, [f], prec).split()[0])
    assert picked == {'igemm<2,3,128,256,1>', 'igemm<2,3,64,64,1>'}, picked
    plan_env.setenv('APAMD_ROWS_WGRAD', '1')
    rows = {}
    for prec in (T.FP32, T.X3, T.B16):
        for m in (24, 32, 64, 128):
            for cin in (1, 3, 4, 9):
                g = ops.Form((1, m, 16, 32), torch.float32, False, 0, False, False, False, False)
                f = ops.Form((1, cin, 16, 32), torch.float32, False, 0, False, False, False, False)
                rows.setdefault(prec, set()).add(ops.wgrad_kernel_route(7, 1, 3, T.REFLECT, g, [f], prec).split()[0])
    assert rows[T.B16] == {'bf16gemm<7,heads>+rows'} and not any('bf16gemm' in r for r in rows[T.FP32] | rows[T.X3]), rows
