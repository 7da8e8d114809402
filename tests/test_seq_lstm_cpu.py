"""CPU (-m "not gpu"): libapseq.so, the batched LSTM forward of Module1's landmark networks -- its C ABI against the header and
the binding, the host-only argument check of apq_lstm_layer_fwd, the Python predicates around it and the backend switch of
module1 / end2end.  Nothing here launches a kernel."""
import inspect
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import ROOT

H = 256
A = 0x10000          # a stand-in address, aligned to everything the kernel asks for


def test_seq_abi_header_binding_and_library_agree():
    from animateportrait_amd import _seqapi, _capi, _dataapi, _styleapi, _faceapi
    hdr = open(os.path.join(ROOT, 'include', 'animateportrait_seq.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    declared = set(re.findall(r'\b(apq_[a-z0-9_]+)\s*\(', code))
    assert declared and declared == set(_seqapi.SIGNATURES)
    lib = _seqapi.lib()
    for name in sorted(declared):
        assert name.startswith('apq_') and hasattr(lib, name), name
    assert int(re.search(r'#define\s+APQ_ABI_VERSION\s+(\d+)', hdr).group(1)) == 1
    assert lib.apq_abi_version() == 1 == _seqapi.ABI_VERSION
    for other in (_capi, _dataapi, _styleapi, _faceapi):
        assert not [n for n in other.SIGNATURES if n.startswith('apq_')], other.__name__
    # the binding's constants are the header's
    for macro, value in (('APQ_LSTM_H', _seqapi.LSTM_H), ('APQ_MAX_B', _seqapi.MAX_B), ('APQ_MAX_T', _seqapi.MAX_T),
                         ('APQ_MAX_I', _seqapi.MAX_I), ('APQ_ALIGN_WIDE', _seqapi.ALIGN_WIDE), ('APQ_ALIGN_ELEM', _seqapi.ALIGN_ELEM)):
        assert int(re.search(r'#define\s+%s\s+(\d+)' % macro, hdr).group(1)) == value, macro


def _ok(x=A, w_ih=A, w_hh=A, b_ih=A, b_hh=A, out=A, B=17, T=18, I=161, h=H, last_only=0):
    from animateportrait_amd import _seqapi
    return _seqapi.lib().apq_lstm_layer_fwd_ok(x, w_ih, w_hh, b_ih, b_hh, out, B, T, I, h, last_only)


@pytest.mark.parametrize('bti', [(1, 1, 80), (17, 18, 161), (512, 18, 256)])
@pytest.mark.parametrize('last_only', [0, 1])
def test_lstm_layer_fwd_ok_accepts_the_served_shapes(bti, last_only):
    b, t, i = bti
    assert _ok(B=b, T=t, I=i, last_only=last_only) == 1


@pytest.mark.parametrize('kw,names', [
    (dict(h=255), 'H = 255'), (dict(h=512), 'H = 512'), (dict(B=0), 'B = 0'), (dict(T=0), 'T = 0'), (dict(I=0), 'I = 0'),
    (dict(w_hh=None), 'null w_hh'), (dict(x=A + 2), 'x is not'),
    # the limits and alignments include/animateportrait_seq.h states
    (dict(I=513), 'I = 513'), (dict(B=1048577), 'B = 1048577'), (dict(T=65537), 'T = 65537'),
    (dict(B=1048576, T=16, I=1), 'out of B T H'), (dict(B=1048576, T=16, I=512), 'x of B T I'), (dict(w_hh=A + 8), 'w_hh is not'), (dict(out=A + 4), 'out is not'),
    (dict(x=None), 'null x'), (dict(out=None), 'null out'),
])
def test_lstm_layer_fwd_ok_refuses_and_names_the_reason(kw, names):
    from animateportrait_amd import _seqapi
    assert _ok() == 1
    assert _ok(**kw) == 0
    assert names in _seqapi.last_error(), _seqapi.last_error()


def test_lstm_layer_fwd_refuses_without_launching():
    """The launching call applies the same checks first: an unsupported size is the unsupported code, a null pointer the
    invalid code, and neither touches a device (there is none here)."""
    from animateportrait_amd import _seqapi
    lib = _seqapi.lib()
    assert lib.apq_lstm_layer_fwd(A, A, A, A, A, A, 17, 18, 161, 512, 0, None) == _seqapi.ERR_UNSUPPORTED
    assert lib.apq_lstm_layer_fwd(A, A, A + 8, A, A, A, 17, 18, 161, H, 0, None) == _seqapi.ERR_UNSUPPORTED
    assert lib.apq_lstm_layer_fwd(A, A, None, A, A, A, 17, 18, 161, H, 0, None) == _seqapi.ERR_INVALID
    with pytest.raises(RuntimeError, match='w_hh'):
        _seqapi.check(lib.apq_lstm_layer_fwd(A, A, None, A, A, A, 17, 18, 161, H, 0, None), 'lstm_layer_fwd')


def test_supported_batched_is_false_off_the_kernels_ground():
    from animateportrait_amd import lstm_hip
    x = torch.randn(6, 18, 80)
    lstm = torch.nn.LSTM(80, H, 3, batch_first=True).eval()
    with torch.no_grad():
        assert not lstm_hip.supported_batched(lstm, x)                                           # a CPU tensor
        assert not lstm_hip.supported_batched(torch.nn.LSTM(80, H, 3, batch_first=True).train(), x)
        assert not lstm_hip.supported_batched(torch.nn.LSTM(80, H, 1, batch_first=True, bidirectional=True).eval(), x)
        assert not lstm_hip.supported_batched(torch.nn.LSTM(80, H, 1, batch_first=True, proj_size=64).eval(), x)
        assert not lstm_hip.supported_batched(torch.nn.LSTM(80, 128, 1, batch_first=True).eval(), x)
    assert not lstm_hip.supported_batched(lstm, x)                                               # grad enabled
    # ... and the predicate itself names each condition (a CPU tensor alone would make all of the above False)
    src = inspect.getsource(lstm_hip.supported_batched)
    for cond in ('x.is_cuda', 'not lstm.training', 'not torch.is_grad_enabled()', 'not lstm.bidirectional', "'proj_size', 0) == 0",
                 'lstm.hidden_size == Q.LSTM_H', 'apq_lstm_layer_fwd_ok'):
        assert cond in src, cond
    # the fallback is the module itself
    with torch.no_grad():
        ref = lstm(x)[0]
        assert torch.equal(lstm_hip.lstm_forward_batched(lstm, x), ref)
        assert torch.equal(lstm_hip.lstm_forward_batched(lstm, x, last_only=True), ref[:, -1, :])


def test_batch1_predicate_is_untouched():
    """lstm_hip.supported on the four configurations of test_module1_gpu.py's kernel test: False on the CPU, and the size
    clause reads as it did."""
    from animateportrait_amd import lstm_hip
    for i, h, layers, bi, t in [(512, 16, 2, True, 96), (545, 512, 3, False, 96), (80, 256, 1, False, 40), (40, 48, 2, True, 33)]:
        lstm = torch.nn.LSTM(i, h, layers, batch_first=True, bidirectional=bi).eval()
        with torch.no_grad():
            assert lstm_hip.supported(lstm, torch.randn(1, t, i)) is False
    src = inspect.getsource(lstm_hip.supported)
    assert '(h <= 64 or (h in (256, 512) and x.shape[0] == 1))' in src and 'apq_' not in src and 'Q.' not in src
    assert 'apq_' not in inspect.getsource(lstm_hip.lstm_forward)


def _seeded_nets():
    from animateportrait_amd import module1 as m1
    torch.manual_seed(11)
    netc = m1.Audio2LandmarkContent(use_prior_net=True, drop_out=0.5).eval()
    netg = m1.Audio2LandmarkPos(drop_out=0.5).eval()
    return netc, netg


def test_set_lstm_backend_and_cpu_fallback_is_bit_identical():
    from animateportrait_amd import module1 as m1
    before = m1.get_lstm_backend()
    with pytest.raises(ValueError):
        m1.set_lstm_backend('nope')
    assert m1.get_lstm_backend() == before
    netc, netg = _seeded_nets()
    g = torch.Generator().manual_seed(12)
    au, emb = torch.randn(6, 18, 80, generator=g), torch.randn(6, 256, generator=g)
    fid, z = torch.randn(1, 204, generator=g) * 0.1, torch.zeros(6, 128)
    out = {}
    try:
        for name in ('library', 'hip'):
            m1.set_lstm_backend(name)
            assert m1.get_lstm_backend() == name
            with torch.no_grad():
                out[name] = (netc(au, fid)[0], netg(au, emb, fid.repeat(6, 1), None, z)[0])
    finally:
        m1.set_lstm_backend(before)
    assert m1.get_lstm_backend() == before
    for a, b in zip(out['library'], out['hip']):
        assert a.shape == (6, 204) and torch.equal(a, b)


@pytest.mark.parametrize('value,want', [('hip', 'hip'), ('library', 'library'), (None, 'library')])
def test_environment_switch_selects_the_backend(value, want):
    env = {k: v for k, v in os.environ.items() if k != 'APAMD_MODULE1_LSTM'}
    if value is not None:
        env['APAMD_MODULE1_LSTM'] = value
    got = subprocess.run([sys.executable, '-c', 'from animateportrait_amd import module1; print(module1.get_lstm_backend())'],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert got.returncode == 0, got.stderr
    assert got.stdout.split()[-1] == want


def test_end2end_parser_takes_the_backend():
    from animateportrait_amd import end2end
    ap = end2end.make_parser()
    base = ['--photo', 'p.png', '--out', 'o']
    assert ap.parse_args(base + ['--module1_lstm', 'hip']).module1_lstm == 'hip'
    assert ap.parse_args(base + ['--module1_lstm', 'library']).module1_lstm == 'library'
    assert ap.parse_args(base).module1_lstm in (None, 'library')          # the default does not select the kernel
    with pytest.raises(SystemExit):
        ap.parse_args(base + ['--module1_lstm', 'miopen'])
