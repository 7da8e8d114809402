"""CPU (-m "not gpu"): the pose network's self-attention encoder on libapseq.so -- its float64 statement (tests/encoder_reference.py)
against ``module1.Encoder`` in torch float64, the C ABI against the header and the binding, the host-only argument checks of
apq_enc_qkv / apq_enc_attn_ff, the backend switch of module1 / end2end and the opt-in mel normalisation (--au_mean_std).  Nothing
here launches a kernel."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, GOLDEN

import encoder_reference as er

A = 0x10000          # a stand-in address, aligned to everything the kernels ask for
IN_SIZE = 512
# (B, T): the single key, the 16-row tile's boundary and its tails, a batch of sequences, the example clip's second segment, the
# maximum
SHAPES = [(1, 1), (1, 15), (1, 16), (1, 17), (1, 33), (3, 17), (1, 113), (1, 512)]
TABLE = os.path.join(GOLDEN, 'MEAN_STD_AUTOVC_RETRAIN_MEL_AU.txt')
WAV = os.path.join(GOLDEN, 'female12.wav')


def make_encoder(d_ff=2048, seed=5):
    """``module1.Encoder(64, 2, 2, 512)`` in fp32 on the CPU with seeded Xavier-style weights; the Norms' alpha / bias and the linear
    biases are drawn too, so that none of them is a no-op"""
    from animateportrait_amd import module1 as m1
    enc = m1.Encoder(64, 2, 2, IN_SIZE)
    if d_ff != 2048:
        for layer in enc.layers:
            layer.ff = m1.FeedForward(64, d_ff)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in enc.named_parameters():
            if p.dim() > 1:
                bound = (6.0 / (p.shape[0] + p.shape[1])) ** 0.5
                p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * bound)
            elif name.endswith('alpha'):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    return enc.eval()


def make_x(b, t, seed=0):
    return torch.randn(b, t, IN_SIZE, generator=torch.Generator().manual_seed(1000 * b + t + seed))


@pytest.mark.parametrize('bt', SHAPES)
def test_statement_is_the_module_in_float64(bt):
    """tests/golden/module1.npz pins module1's networks to the reference's own classes; this pins the statement to the module."""
    import copy
    enc = make_encoder()
    x = make_x(*bt)
    with torch.no_grad():
        want = copy.deepcopy(enc).double()(x.double()).numpy()
    got = er.encoder_forward(x.numpy(), er.params_of(enc))
    assert got.shape == want.shape == bt + (64,) and got.dtype == np.float64
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_statement_takes_another_d_ff():
    import copy
    enc = make_encoder(d_ff=256, seed=6)
    x = make_x(1, 33)
    with torch.no_grad():
        want = copy.deepcopy(enc).double()(x.double()).numpy()
    got = er.encoder_forward(x.numpy(), er.params_of(enc))
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_encoder_symbols_and_constants_in_header_and_binding():
    from animateportrait_amd import _seqapi
    hdr = open(os.path.join(ROOT, 'include', 'animateportrait_seq.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    declared = set(re.findall(r'\b(apq_[a-z0-9_]+)\s*\(', code))
    lib = _seqapi.lib()
    for name in ('apq_enc_qkv_ok', 'apq_enc_qkv', 'apq_enc_attn_ff_ok', 'apq_enc_attn_ff'):
        assert name in declared and name in _seqapi.SIGNATURES and hasattr(lib, name), name
    for macro, value in (('APQ_ENC_D', _seqapi.ENC_D), ('APQ_ENC_HEADS', _seqapi.ENC_HEADS), ('APQ_ENC_ROWS', _seqapi.ENC_ROWS),
                         ('APQ_ENC_MAX_T', _seqapi.ENC_MAX_T), ('APQ_ENC_FF_CHUNK', _seqapi.ENC_FF_CHUNK),
                         ('APQ_ENC_MAX_FF', _seqapi.ENC_MAX_FF)):
        assert int(re.search(r'#define\s+%s\s+(\d+)' % macro, hdr).group(1)) == value, macro
    assert (_seqapi.ENC_D, _seqapi.ENC_HEADS, _seqapi.ENC_MAX_T) == (64, 2, 512)
    assert 2048 % _seqapi.ENC_FF_CHUNK == 0 and _seqapi.ENC_MAX_FF >= 2048
    assert int(re.search(r'#define\s+APQ_ABI_VERSION\s+(\d+)', hdr).group(1)) == 1 == lib.apq_abi_version()


QKV_PTRS = ('x', 'alpha', 'bias', 'wq', 'bq', 'wk', 'bk', 'wv', 'bv', 'q', 'k', 'v')
ATTN_PTRS = ('x', 'q', 'k', 'v', 'wo', 'bo', 'alpha2', 'bias2', 'w1', 'b1', 'w2', 'b2', 'alpha_f', 'bias_f', 'y')


def _qkv_args(B=1, T=113, d_model=64, **ptr):
    p = {n: ptr.get(n, A) for n in QKV_PTRS}
    return [p['x'], p['alpha'], p['bias'], 1e-6] + [p[n] for n in QKV_PTRS[3:]] + [B, T, d_model]


def _attn_args(B=1, T=113, d_model=64, heads=2, d_ff=2048, **ptr):
    p = {n: ptr.get(n, A) for n in ATTN_PTRS}
    return ([p[n] for n in ATTN_PTRS[:8]] + [1e-6] + [p[n] for n in ATTN_PTRS[8:12]] + [p['alpha_f'], p['bias_f'], 1e-6, p['y']] +
            [B, T, d_model, heads, d_ff])


def _qkv_ok(**kw):
    from animateportrait_amd import _seqapi
    return _seqapi.lib().apq_enc_qkv_ok(*_qkv_args(**kw))


def _attn_ok(**kw):
    from animateportrait_amd import _seqapi
    return _seqapi.lib().apq_enc_attn_ff_ok(*_attn_args(**kw))


@pytest.mark.parametrize('bt', SHAPES + [(4096, 512)])
def test_ok_twins_accept_the_served_shapes(bt):
    assert _qkv_ok(B=bt[0], T=bt[1]) == 1
    for d_ff in (256, 2048, 8192):
        assert _attn_ok(B=bt[0], T=bt[1], d_ff=d_ff) == 1
    assert _attn_ok(B=bt[0], T=bt[1], alpha_f=None, bias_f=None) == 1          # every layer but the last: no closing Norm


@pytest.mark.parametrize('kw,names', [
    (dict(T=513), 'T = 513'), (dict(T=0), 'T = 0'), (dict(B=0), 'B = 0'), (dict(d_model=32), 'd_model = 32'), (dict(d_model=128), 'd_model = 128'),
    (dict(d_model=0), 'd_model = 0'), (dict(B=1048577), 'B = 1048577'), (dict(B=65537, T=512), 'elements'),
    (dict(x=A + 4), 'x is not 16-byte aligned'), (dict(wk=A + 8), 'wk is not'), (dict(v=A + 4), 'v is not'), (dict(bias=A + 2), 'bias is not'),
] + [({n: None}, 'null ' + n) for n in QKV_PTRS])
def test_enc_qkv_ok_refuses_and_names_the_reason(kw, names):
    from animateportrait_amd import _seqapi
    assert _qkv_ok() == 1
    assert _qkv_ok(**kw) == 0
    msg = _seqapi.last_error()
    assert msg.startswith('enc_qkv: ') and names in msg, msg


@pytest.mark.parametrize('kw,names', [
    (dict(T=513), 'T = 513'), (dict(T=0), 'T = 0'), (dict(B=0), 'B = 0'), (dict(heads=4), 'heads = 4'), (dict(heads=1), 'heads = 1'),
    (dict(heads=0), 'heads = 0'), (dict(d_model=32), 'd_model = 32'), (dict(d_ff=0), 'd_ff = 0'), (dict(d_ff=2000), 'd_ff = 2000'),
    (dict(d_ff=128), 'd_ff = 128'), (dict(d_ff=8448), 'd_ff = 8448'), (dict(B=1048577), 'B = 1048577'), (dict(B=65537, T=512), 'elements'),
    (dict(q=A + 4), 'q is not 16-byte aligned'), (dict(w2=A + 8), 'w2 is not'), (dict(y=A + 4), 'y is not'), (dict(alpha_f=A + 4), 'alpha_f is not'),
    (dict(alpha_f=None), 'both or neither'), (dict(bias_f=None), 'both or neither'),
] + [({n: None}, 'null ' + n) for n in ATTN_PTRS if not n.endswith('_f')])
def test_enc_attn_ff_ok_refuses_and_names_the_reason(kw, names):
    from animateportrait_amd import _seqapi
    assert _attn_ok() == 1
    assert _attn_ok(**kw) == 0
    msg = _seqapi.last_error()
    assert msg.startswith('enc_attn_ff: ') and names in msg, msg


def test_launching_calls_refuse_without_launching():
    """The launching calls apply the same checks first: unsupported sizes give the unsupported code, null pointers the invalid
    code, and neither touches a device (there is none here)."""
    from animateportrait_amd import _seqapi
    lib = _seqapi.lib()
    assert lib.apq_enc_qkv(*_qkv_args(T=513), None) == _seqapi.ERR_UNSUPPORTED
    assert lib.apq_enc_qkv(*_qkv_args(d_model=32), None) == _seqapi.ERR_UNSUPPORTED
    assert lib.apq_enc_qkv(*_qkv_args(wq=None), None) == _seqapi.ERR_INVALID
    assert lib.apq_enc_attn_ff(*_attn_args(heads=4), None) == _seqapi.ERR_UNSUPPORTED
    assert lib.apq_enc_attn_ff(*_attn_args(y=A + 4), None) == _seqapi.ERR_UNSUPPORTED
    assert lib.apq_enc_attn_ff(*_attn_args(w1=None), None) == _seqapi.ERR_INVALID
    with pytest.raises(RuntimeError, match='null w1'):
        _seqapi.check(lib.apq_enc_attn_ff(*_attn_args(w1=None), None), 'enc_attn_ff')


def test_set_encoder_backend_rejects_unknown_names_and_returns_the_previous():
    from animateportrait_amd import module1 as m1
    assert m1.ENCODER_BACKENDS == ('library', 'hip')
    before = m1.get_encoder_backend()
    with pytest.raises(ValueError):
        m1.set_encoder_backend('flash')
    assert m1.get_encoder_backend() == before
    try:
        assert m1.set_encoder_backend('hip') == before and m1.get_encoder_backend() == 'hip'
        assert m1.set_encoder_backend('library') == 'hip' and m1.get_encoder_backend() == 'library'
    finally:
        m1.set_encoder_backend(before)


@pytest.mark.parametrize('value,want', [('hip', 'hip'), ('library', 'library'), (None, 'library')])
def test_environment_variable_is_read_at_import(value, want):
    env = {k: v for k, v in os.environ.items() if k != 'APAMD_MODULE1_ENCODER'}
    if value is not None:
        env['APAMD_MODULE1_ENCODER'] = value
    got = subprocess.run([sys.executable, '-c', 'from animateportrait_amd import module1; print(module1.get_encoder_backend())'],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert got.returncode == 0, got.stderr
    assert got.stdout.split()[-1] == want


def test_end2end_parser_knows_the_two_options():
    from animateportrait_amd import end2end
    ap = end2end.make_parser()
    base = ['--photo', 'p.png', '--out', 'o']
    assert ap.parse_args(base + ['--module1_encoder', 'hip']).module1_encoder == 'hip'
    assert ap.parse_args(base + ['--module1_encoder', 'library']).module1_encoder == 'library'
    assert ap.parse_args(base).module1_encoder in (None, 'library')       # the default does not select the kernels
    with pytest.raises(SystemExit):
        ap.parse_args(base + ['--module1_encoder', 'flash'])
    assert ap.parse_args(base).au_mean_std is None
    assert ap.parse_args(base + ['--au_mean_std', TABLE]).au_mean_std == TABLE


class _OnDevice:
    """stands for a CUDA tensor in front of the eligibility test: there is no device here"""
    is_cuda = True


def test_encoder_forward_keeps_cpu_tensors_masks_and_training_on_the_torch_path(monkeypatch):
    from animateportrait_amd import encoder_hip, module1 as m1

    def boom(*a, **k):
        raise AssertionError('the kernel binding was called')
    enc = make_encoder(d_ff=256)
    x = make_x(2, 17)
    with torch.no_grad():
        want = enc(x)
    prev = m1.set_encoder_backend('hip')
    try:
        monkeypatch.setattr(encoder_hip, 'encoder_forward', boom)
        monkeypatch.setattr(encoder_hip.Q, 'lib', boom)
        # a CPU tensor: eval without gradients, with a mask, training with gradients
        with torch.no_grad():
            assert torch.equal(enc(x), want)
            masked = enc(x, torch.ones(2, 17, 17))
        assert torch.equal(masked, want)
        enc.train()
        for m in enc.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.0
        out = enc(x)
        assert out.requires_grad and torch.equal(out.detach(), want)
        enc.eval()
        # the same three on a device tensor: only the mask and training with gradients keep it off the kernels
        monkeypatch.setattr(encoder_hip, 'supported', lambda e, t: True)
        dev_x = _OnDevice()
        with torch.no_grad():
            assert m1._encoder_on_kernels(enc, dev_x, None) is True
            assert m1._encoder_on_kernels(enc, dev_x, torch.ones(2, 17, 17)) is False
            assert m1._encoder_on_kernels(enc, x, None) is False
        assert m1._encoder_on_kernels(enc, dev_x, None) is True               # eval mode, gradients enabled
        enc.train()
        assert m1._encoder_on_kernels(enc, dev_x, None) is False              # training with gradients
        with torch.no_grad():
            assert m1._encoder_on_kernels(enc, dev_x, None) is True           # training mode, gradients disabled
        enc.eval()
        monkeypatch.setattr(encoder_hip, 'supported', lambda e, t: False)
        with torch.no_grad():
            assert m1._encoder_on_kernels(enc, dev_x, None) is False          # shapes the library does not serve
        m1.set_encoder_backend('library')
        monkeypatch.setattr(encoder_hip, 'supported', boom)
        with torch.no_grad():
            assert m1._encoder_on_kernels(enc, dev_x, None) is False          # the default backend never asks
    finally:
        m1.set_encoder_backend(prev)


def test_supported_is_false_for_a_cpu_tensor():
    from animateportrait_amd import encoder_hip
    assert encoder_hip.supported(make_encoder(d_ff=256), make_x(1, 17)) is False


# ------------------------------------------------------------------------------------------------ --au_mean_std
def test_fixture_table_is_80_means_then_80_standard_deviations():
    from animateportrait_amd import audio
    mean, std = audio.load_mean_std(TABLE)
    assert mean.shape == std.shape == (80,) and mean.dtype == np.float64
    assert np.isfinite(mean).all() and bool((std > 0).all())
    raw = np.loadtxt(TABLE)
    assert raw.size == 160 and np.array_equal(mean, raw[:80]) and np.array_equal(std, raw[80:])


def test_mean_std_table_reproduces_the_float64_normalisation():
    from animateportrait_amd import audio
    mel = np.random.RandomState(3).rand(40, 80).astype(np.float32)
    raw = np.loadtxt(TABLE)
    want = (mel.astype(np.float64) - raw[:80]) / raw[80:]
    got = audio.normalize_mel(mel, TABLE)
    assert got.dtype == np.float32 and got.shape == (40, 80)
    assert np.array_equal(got, want.astype(np.float32))
    t = audio.normalize_mel(torch.from_numpy(mel), audio.load_mean_std(TABLE))          # a tensor takes the same arithmetic
    assert t.dtype == torch.float32 and np.array_equal(t.numpy(), got)
    assert audio.normalize_mel(mel, None) is mel
    with pytest.raises(ValueError):
        audio.normalize_mel(mel[:, :40], TABLE)


def test_clip_features_with_and_without_the_table():
    """With no table the windows are today's bits; with it they are the windows of the normalised mel (after the converter)."""
    from animateportrait_amd import audio
    conv = lambda m: m * 0.5                                                             # noqa: E731
    base = audio.clip_audio_features(WAV, max_frames=30, converter=conv)
    assert np.array_equal(audio.clip_audio_features(WAV, max_frames=30, converter=conv, au_mean_std=None), base)
    x, sr = audio.read_wav(WAV)
    mel = audio.mel_spectrogram(audio.normalize_loudness(audio.resample_to_16k(x, sr))).astype(np.float32) * np.float32(0.5)
    assert np.array_equal(audio.window_frames(mel)[:30], base)
    raw = np.loadtxt(TABLE)
    want = audio.window_frames(((mel.astype(np.float64) - raw[:80]) / raw[80:]).astype(np.float32))[:30]
    got = audio.clip_audio_features(WAV, max_frames=30, converter=conv, au_mean_std=TABLE)
    assert got.dtype == np.float32 and np.array_equal(got, want) and not np.array_equal(got, base)
    # a CPU-only call of the device front end computes on the host and takes the table too
    assert np.array_equal(audio.clip_audio_features(WAV, max_frames=30, converter=conv, au_mean_std=TABLE, backend='device'), got)


def test_module1_train_shares_the_table_reader():
    from animateportrait_amd import audio, module1_train
    assert module1_train.load_mean_std is audio.load_mean_std
