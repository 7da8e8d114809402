"""CPU (-m "not gpu"): the APAMD_* environment switches are stated once per side of the C ABI -- the table of csrc/switches.h with
its reader sw(), and the table of ops.py with its reader _switch() -- and both sides parse a value by one rule: unset, empty, not a
number or 0 is the default, any other integer is that value.

  scans      nothing else in the core library calls getenv, nothing else in ops.py touches os.environ (APAMD_PRECISION, a name and
             no switch, apart); every switch a source reads is a row, every row is read, ap_switch_names reports the rows;
  Appendix A DESIGN.md's table documents every switch of both tables and names no variable that nothing reads: the tables, the
             package and bench.py are searched as the issue says, and tests/, where APAMD_TEST_DUMP is read;
  parity     the same value list through a C-side plan query and through ops._switch / s2d_eligible;
  cache key  every name of ops.plan_switch_names() is part of ops.backward_switches(), with X=0 and unset as one entry;
  xs halves  ops.XS_WGRAD / XS_DIRECT (what the descriptor carries) against APAMD_NO_XS_WGRAD / _DIRECT (what the planner accepts):
             the answers of tests/golden/xs_switch_answers.json, recorded at the commit before the tables existed."""
import ast
import ctypes
import glob
import json
import os
import re

import pytest
import torch

from animateportrait_amd import _capi, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'animateportrait_amd', 'csrc')
VALUES = (None, '', '0', '1', '2', '-1', 'x')
ROUTE, TUNING, BUILD_ONLY = 0, 1, 2
NAME = re.compile(r'APAMD_[A-Z0-9_]+')


def _read(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def _core_sources():
    """{file name: text} of csrc/*.hip and csrc/*.h"""
    return {os.path.basename(p): _read(p) for ext in ('hip', 'h') for p in glob.glob(os.path.join(CSRC, '*.' + ext))}


def table_rows():
    """{id: (variable, kind)} of every X(...) row of switches.h, the experiment builds' rows included"""
    rows = re.findall(r'\bX\((\w+), "(APAMD_[A-Z0-9_]+)", [^,]+, (ROUTE|TUNING|BUILD_ONLY), "', _read(CSRC, 'switches.h'))
    assert len(rows) == len({r[0] for r in rows}) == len({r[1] for r in rows}) >= 20
    return {i: (name, kind) for i, name, kind in rows}


def ops_switches():
    """every variable ops.py hands to _switch"""
    return set(re.findall(r"_switch\('(APAMD_[A-Z0-9_]+)'", _read('animateportrait_amd', 'ops.py'))) | set(ops._PER_CALL_SWITCHES)


def _set(monkeypatch, name, value):
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, value)


@pytest.fixture
def clean_env(monkeypatch):
    for v in ops.plan_switch_names():
        monkeypatch.delenv(v, raising=False)
    return monkeypatch


def test_only_switches_h_reads_the_environment():
    for name, text in _core_sources().items():
        if name != 'switches.h':
            assert 'getenv' not in text, name
    assert _read(CSRC, 'switches.h').count('getenv(') == 1


def test_only_switch_reads_the_environment_in_ops():
    text = _read('animateportrait_amd', 'ops.py')
    fn = next(n for n in ast.parse(text).body if isinstance(n, ast.FunctionDef) and n.name == '_switch')
    for i, line in enumerate(text.splitlines(), 1):
        if 'os.environ' in line or 'getenv' in line:
            assert fn.lineno <= i <= fn.end_lineno or "os.environ.get('APAMD_PRECISION'" in line, (i, line)


def test_every_switch_read_is_a_row_and_every_row_is_read():
    rows = table_rows()
    used = set()
    for name, text in _core_sources().items():
        if name == 'switches.h':
            continue
        # (quoted APAMD_* names outside comments would be reads that bypass the table: there is no such string left)
        code = re.sub(r'//.*', '', text)
        assert not re.findall(r'"APAMD_[A-Z0-9_]+"', code), name
        used |= set(re.findall(r'\bsw(?:_text|_is)?\(SW_(\w+)', code))
    assert used == set(rows)
    reported = {k: set(_names(k)) for k in (ROUTE, TUNING, BUILD_ONLY)}
    assert reported[ROUTE] == {n for n, k in rows.values() if k == 'ROUTE'}
    assert reported[TUNING] == {n for n, k in rows.values() if k == 'TUNING'}
    assert reported[BUILD_ONLY] == set()          # the product library has none of the experiment builds' rows
    assert set(ops.plan_switch_names()) == reported[ROUTE] | reported[TUNING] | set(ops._PER_CALL_SWITCHES)
    assert {'APAMD_BF3_BLOCKS', 'APAMD_WGRAD_BLOCKS', 'APAMD_CONV_COTILE', 'APAMD_CONV_CI', 'APAMD_CONV_LDS_TARGET',
            'APAMD_WARP_TILE'} == reported[TUNING]


def _names(kind):
    lib = _capi.lib()
    need = lib.ap_switch_names(kind, None, 0)
    assert need >= 1
    buf = ctypes.create_string_buffer(need)
    assert lib.ap_switch_names(kind, buf, need - 1) == need and buf.raw == b'\0' * need       # too small: nothing written
    assert lib.ap_switch_names(kind, buf, need) == need
    return buf.value.decode().split()


def test_switch_names_refuses_an_unknown_kind():
    assert _capi.lib().ap_switch_names(3, None, 0) < 0 and _capi.lib().ap_switch_names(-1, None, 0) < 0


def appendix_a_faults(design):
    """(switches of the two tables without a row in Appendix A, variables Appendix A names that nothing reads)"""
    appendix = design[design.index('## Appendix A. Environment switches'):]
    documented = set()
    for line in appendix.splitlines():
        if line.startswith('| `APAMD_'):
            documented |= set(NAME.findall(line.split('|')[1]))
    tables = {n for n, _ in table_rows().values()} | ops_switches()
    read = set(tables)
    files = glob.glob(os.path.join(ROOT, 'animateportrait_amd', '**', '*.*'), recursive=True) + [os.path.join(ROOT, 'bench.py')]
    files += [p for p in glob.glob(os.path.join(ROOT, 'tests', '*.py')) if os.path.abspath(p) != os.path.abspath(__file__)]
    for p in files:
        if p.endswith(('.py', '.hip', '.h')):
            with open(p, errors='replace') as f:
                read |= set(NAME.findall(f.read()))
    # (`APAMD_CFG_A/B/C` is one name and two letters)
    return sorted(tables - documented), sorted(n for n in documented if n not in read)


def test_appendix_a_documents_every_switch_and_nothing_else():
    assert appendix_a_faults(_read('DESIGN.md')) == ([], [])


def _presplit_desc():
    spec = ops.ConvSpec([256], 256, 3, 1, 1, ops.PAD_REFLECT)
    spec.precision = ops.PRECISION_BF16X3
    return spec.desc(1, 64, 64)


@pytest.mark.parametrize('value', VALUES, ids=repr)
def test_both_sides_parse_a_value_alike(clean_env, value):
    _set(clean_env, 'APAMD_NO_BF16X3', value)
    expect = {None: 0, '': 0, '0': 0, '1': 1, '2': 2, '-1': -1, 'x': 0}[value]
    assert ops._switch('APAMD_NO_BF16X3') == expect
    assert ops._switch('APAMD_NO_BF16X3', 7) == (expect or 7)
    assert _capi.lib().ap_conv2d_wants_presplit(ctypes.byref(_presplit_desc())) == (0 if expect else 1)


@pytest.mark.parametrize('value', VALUES, ids=repr)
def test_s2d_eligible_parses_its_switches_by_the_same_rule(clean_env, value):
    k4 = ops.ConvSpec([64], 128, 4, 2, 1, ops.PAD_ZERO)
    k3 = ops.ConvSpec([64], 128, 3, 2, 1, ops.PAD_ZERO)
    k4.precision = k3.precision = ops.PRECISION_BF16X3
    assert ops.s2d_eligible(k4, 32, 32) and ops.s2d_eligible(k3, 32, 32)
    off = value in ('1', '2', '-1')
    _set(clean_env, 'APAMD_NO_S2D3', value)
    assert ops.s2d_eligible(k4, 32, 32) and ops.s2d_eligible(k3, 32, 32) == (not off)
    _set(clean_env, 'APAMD_NO_S2D3', None)
    _set(clean_env, 'APAMD_NO_S2D', value)
    assert ops.s2d_eligible(k4, 32, 32) == ops.s2d_eligible(k3, 32, 32) == (not off)


def test_every_plan_switch_is_in_the_cache_key(clean_env):
    base = ops.backward_switches()
    names = ops.plan_switch_names()
    assert len(base) == 6 + len(names) and len(set(names)) == len(names) >= 18
    for name in names:
        clean_env.setenv(name, '1')
        assert ops.backward_switches() != base, name
        clean_env.setenv(name, '3')                   # (APAMD_WARP_GATHER is a word: any text is a value of its own)
        assert ops.backward_switches() != base, name
        for same in ('0', ''):
            clean_env.setenv(name, same)
            assert ops.backward_switches() == base, name
        clean_env.delenv(name)
    clean_env.setenv('APAMD_WARP_GATHER', 'quad')
    assert ops.backward_switches() != base


def test_xs_globals_and_xs_variables_answer_as_before(clean_env):
    """The Python global decides what the descriptor carries, the C switch what the planner accepts: the four combinations of each
    pair answer as they did at the recorded commit."""
    golden = json.loads(_read('tests', 'golden', 'xs_switch_answers.json'))
    clean_env.setattr(ops, '_require_device', lambda *a, **k: None)
    clean_env.setattr(ops, 'DEFAULT_PRECISION', ops.PRECISION_BF16X3)
    n, c, h, w = 1, 256, 16, 16
    src = ops.Feat(torch.zeros(n, c, h, w))
    src.xs = torch.zeros(16, dtype=torch.uint8)        # the forward pass's split copy (its pointer is all the plan reads)
    geom = (3, 1, 1, ops.PAD_REFLECT, (n, c, h, w))
    assert len(golden['rows']) == 8
    for row in golden['rows']:
        clean_env.setattr(ops, 'XS_WGRAD', True)
        clean_env.setattr(ops, 'XS_DIRECT', True)
        clean_env.setattr(ops, row['global'], row['value'])
        clean_env.setattr(ops, '_WGRAD_XS_OK', {})
        _set(clean_env, row['variable'], row['env'])
        d = ops._wgrad_desc(*geom, None, [src], None)
        got = dict(row, wgrad_xs_ok=ops.wgrad_xs_ok(*geom, [src], None),
                   ap_conv2d_wgrad_xs_ok=_capi.lib().ap_conv2d_wgrad_xs_ok(ctypes.byref(d)))
        assert got == row
        clean_env.delenv(row['variable'], raising=False)
