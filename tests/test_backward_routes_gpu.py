"""GPU (-m gpu): which launches the train step's backward schedule issues, pinned.  tests/golden/backward_routes.json holds every call
of the C ABI that one gradient pass of geomgm_ifw_fore made (set_input, forward, the G backward and the five D backwards:
test_train_gpu._backward_both) at commit b096b60 -- the parent of the change that gave autograd.conv_backward one cached plan per
layer (autograd._backward_plan) and ops.wgrad a route chosen before anything is launched (ops.wgrad_route).  Each call is one
line: the entry point's name and those of its arguments that are plain integers (sizes, pads, activations, flags; pointers,
descriptors, floats and streams are left out).  The plan queries of QUERIES are not recorded: a schedule may ask them less often.

The library object the package calls through (animateportrait_amd._capi._lib) is replaced by a recording proxy for the duration
of a pass.  Every case runs twice in one process: the second pass finds the per-layer plans cached and must issue the same
launches.  It packs no weights (the packed images are cached per weight version; an untouched parameter is not packed again), so
the two passes are compared without the weight packer's calls; the golden holds the first pass with them.

The last case flips APAMD_NO_S2D_WGRAD between two passes over one model: the second must issue what a FRESH process under that
switch issues -- a plan cached under the other setting would not (at b096b60 itself the second pass does not get that far:
the layer plan still hands the weight gradient a split copy, and ops.wgrad refuses it).

The golden stores each distinct line once (``lines``) and a case as indices into that table, a run of one index as
[index, count].  To record it after a DELIBERATE change of the schedule: ``python tests/test_backward_routes_gpu.py --record``
(one fresh process per case) and name the commit above."""
import fnmatch
import json
import os
import subprocess
import sys

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'backward_routes.json')
QUERIES = ('*_ok', '*_workspace_floats', '*_gt_dims', 'ap_conv2d_out_size', 'ap_conv2d_wants_presplit', 'ap_last_error', 'ap_abi_version')
PACKER = 'ap_conv2d_pack*'
# (precision, ngf = ndf, batch): the drawing width, and the full width, whose layers are the ones the split, xs, strip, k7, d0 and
# head routes serve (B = 1 is the smallest batch that reaches them)
CASES = [(p, w, b) for w, b in ((8, 2), (64, 1)) for p in ('fp32', 'bf16x3', 'bf16')]
SWITCHED = ('bf16x3', 64, 1)
SWITCH = 'APAMD_NO_S2D_WGRAD'


def _name(case, switched=False):
    return '%s-ngf%d-b%d' % case + ('-no_s2d_wgrad' if switched else '')


class Recorder:
    """Stands in for the ctypes library: every entry point called through it leaves one line in ``lines``."""

    def __init__(self, lib):
        self._lib, self.lines = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if any(fnmatch.fnmatchcase(name, q) for q in QUERIES):
            return fn

        def call(*args):
            self.lines.append(' '.join([name] + [str(int(a)) for a in args if isinstance(a, int)]))
            return fn(*args)
        return call


def _one_pass(model, batch):
    from animateportrait_amd import _capi
    from test_train_gpu import _backward_both
    real = _capi.lib()
    rec = Recorder(real)
    _capi._lib = rec
    try:
        _backward_both(model, batch)
        torch.cuda.synchronize()
    finally:
        _capi._lib = real
    return rec.lines


def _model_and_batch(case, set_precision):
    from animateportrait_amd import ops
    from animateportrait_amd.data.synthetic_dataset import make_train_batch
    from test_train_gpu import _make_model
    precision, width, nb = case
    set_precision(ops.PRECISION_BY_NAME[precision])
    torch.manual_seed(0)
    model, _ = _make_model(torch.device('cuda:0'), width, width)
    return model, make_train_batch(nb, seed=5)


def _launches(lines):
    return [ln for ln in lines if not fnmatch.fnmatchcase(ln.split(' ', 1)[0], PACKER)]


def _pack(lines, table):
    out = []
    for ln in lines:
        i = table.setdefault(ln, len(table))
        if out and (out[-1] == i or (isinstance(out[-1], list) and out[-1][0] == i)):
            out[-1] = [i, out[-1][1] + 1] if isinstance(out[-1], list) else [i, 2]
        else:
            out.append(i)
    return out


def _unpack(golden, name):
    lines = golden['lines']
    out = []
    for e in golden['cases'][name]:
        out.extend([lines[e[0]]] * e[1] if isinstance(e, list) else [lines[e]])
    return out


def _same(got, want, what):
    if got != want:
        at = next((i for i, (g, w) in enumerate(zip(got, want)) if g != w), min(len(got), len(want)))
        raise AssertionError('%s: %d calls against %d; first difference at call %d:\n  got      %s\n  recorded %s' % (
            what, len(got), len(want), at, got[at - 2:at + 3], want[at - 2:at + 3]))


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture
def clean_env(monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    monkeypatch.delenv(SWITCH, raising=False)
    return monkeypatch


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES, ids=[_name(c) for c in CASES])
def test_backward_launches_match_the_recorded_schedule(clean_env, golden, case):
    from animateportrait_amd import ops
    model, batch = _model_and_batch(case, lambda p: clean_env.setattr(ops, 'DEFAULT_PRECISION', p))
    first = _one_pass(model, batch)
    second = _one_pass(model, batch)
    _same(first, _unpack(golden, _name(case)), 'first pass')
    _same(_launches(second), _launches(first), 'second pass (plans cached) against the first')
    assert len(_launches(first)) > 500 and any(ln.startswith('ap_conv2d_wgrad') for ln in first)


@pytest.mark.gpu
def test_a_switch_flipped_between_two_passes_reaches_the_layer_plans(clean_env, golden):
    from animateportrait_amd import ops
    model, batch = _model_and_batch(SWITCHED, lambda p: clean_env.setattr(ops, 'DEFAULT_PRECISION', p))
    first = _one_pass(model, batch)
    _same(first, _unpack(golden, _name(SWITCHED)), 'pass before the switch')
    clean_env.setenv(SWITCH, '1')
    second = _one_pass(model, batch)
    want = _launches(_unpack(golden, _name(SWITCHED, True)))
    assert want != _launches(first)                     # (the switch does change the schedule: the case is not vacuous)
    _same(_launches(second), want, 'pass under %s=1 against a fresh process under it' % SWITCH)


def _trace_in_this_process(case, switched, path):
    from animateportrait_amd import ops
    model, batch = _model_and_batch(case, lambda p: setattr(ops, 'DEFAULT_PRECISION', p))
    with open(path, 'w') as f:
        json.dump(_one_pass(model, batch), f)


if __name__ == '__main__' and len(sys.argv) > 1:
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if sys.argv[1] == '--trace':            # child of --record: one case, one pass, a fresh process
        _trace_in_this_process((sys.argv[2], int(sys.argv[3]), int(sys.argv[4])), sys.argv[5] == '1', sys.argv[6])
    elif sys.argv[1] == '--record':
        table, cases = {}, {}
        for case, switched in [(c, False) for c in CASES] + [(SWITCHED, True)]:
            env = {k: v for k, v in os.environ.items() if k != SWITCH}
            if switched:
                env[SWITCH] = '1'
            tmp = GOLDEN + '.tmp'
            subprocess.run([sys.executable, os.path.abspath(__file__), '--trace'] + [str(v) for v in case] + ['1' if switched else '0', tmp],
                           env=env, check=True, timeout=300)
            with open(tmp) as f:
                cases[_name(case, switched)] = _pack(json.load(f), table)
            os.remove(tmp)
        with open(GOLDEN, 'w') as f:
            f.write('{"lines": [\n' + ',\n'.join(json.dumps(ln) for ln in table) + '\n],\n"cases": {\n')
            f.write(',\n'.join('"%s": %s' % (n, json.dumps(v, separators=(',', ':'))) for n, v in cases.items()))
            f.write('\n}}\n')
        print('recorded', {n: len(v) for n, v in cases.items()}, 'in', GOLDEN, os.path.getsize(GOLDEN), 'bytes')
