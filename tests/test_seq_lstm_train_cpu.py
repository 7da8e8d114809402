"""CPU (-m "not gpu"): training Module1's content branch -- the C ABI of the two training calls of libapseq.so against the
header and the binding, their host-only argument checks, and the dataset, loss, optimiser step, checkpoint and command line of
animateportrait_amd/module1_train.py against the reference-made golden (tests/golden/module1_train.npz) in float64.  Nothing
here launches a kernel."""
import argparse
import os
import pickle
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, GOLDEN

sys.path.insert(0, GOLDEN)

H = 256
A = 0x10000          # a stand-in address, aligned to everything the kernels ask for
# a bias in front of a BatchNorm1d in training mode: the batch mean takes it out again, its gradient is identically zero
BIAS_UNDER_BATCHNORM = ('fc_prior.0.bias', 'fc.0.bias', 'fc.3.bias')
NAMES = ('apq_lstm_layer_fwd_train_ok', 'apq_lstm_layer_fwd_train', 'apq_lstm_layer_bwd_ok', 'apq_lstm_layer_bwd')


def test_training_symbols_in_header_binding_and_library_with_equal_signatures():
    import ctypes
    from animateportrait_amd import _seqapi
    hdr = open(os.path.join(ROOT, 'include', 'animateportrait_seq.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    ctype = {'int32_t': ctypes.c_int32, 'int': ctypes.c_int, 'void*': ctypes.c_void_p, 'float*': ctypes.c_void_p,
             'const float*': ctypes.c_void_p}
    lib = _seqapi.lib()
    for name in NAMES:
        m = re.search(r'(\w+)\s+%s\s*\(([^)]*)\)\s*;' % name, code)
        assert m, name
        args = [re.sub(r'\s*\w+$', '', a.strip()) for a in m.group(2).split(',')]
        res, argtypes = _seqapi.SIGNATURES[name]
        assert res is ctype[m.group(1)], name
        assert argtypes == [ctype[a] for a in args], name
        assert hasattr(lib, name)
    # a launching call is its twin with writable outputs and the stream
    assert _seqapi.SIGNATURES['apq_lstm_layer_fwd_train'][1] == _seqapi.SIGNATURES['apq_lstm_layer_fwd_train_ok'][1] + [ctypes.c_void_p]
    assert _seqapi.SIGNATURES['apq_lstm_layer_bwd'][1] == _seqapi.SIGNATURES['apq_lstm_layer_bwd_ok'][1] + [ctypes.c_void_p]
    assert int(re.search(r'#define\s+APQ_ABI_VERSION\s+(\d+)', hdr).group(1)) == 1 == lib.apq_abi_version()


def _fwd_ok(x=A, w_ih=A, w_hh=A, b_ih=A, b_hh=A, out=A, gates=A, cell=A, B=17, T=18, I=161, h=H):
    from animateportrait_amd import _seqapi
    return _seqapi.lib().apq_lstm_layer_fwd_train_ok(x, w_ih, w_hh, b_ih, b_hh, out, gates, cell, B, T, I, h)


def _bwd_ok(dout=A, gates=A, cell=A, w_hh_t=A, dgates=A, B=17, T=18, h=H, last_only=0):
    from animateportrait_amd import _seqapi
    return _seqapi.lib().apq_lstm_layer_bwd_ok(dout, gates, cell, w_hh_t, dgates, B, T, h, last_only)


@pytest.mark.parametrize('bti', [(1, 1, 1), (1048576, 1, 1)])
def test_ok_twins_serve_the_corners(bti):
    b, t, i = bti
    assert _fwd_ok(B=b, T=t, I=i) == 1
    assert _bwd_ok(B=b, T=t, last_only=0) == 1 and _bwd_ok(B=b, T=t, last_only=1) == 1


@pytest.mark.parametrize('fn,kw,reason', [
    (_fwd_ok, dict(h=128), 'H = 128'), (_bwd_ok, dict(h=128), 'H = 128'),
    (_fwd_ok, dict(T=0), 'T = 0'), (_bwd_ok, dict(T=0), 'T = 0'),
    (_fwd_ok, dict(I=513), 'I = 513'),
    (_fwd_ok, dict(gates=None), 'null gates'), (_fwd_ok, dict(cell=None), 'null cell'), (_fwd_ok, dict(x=None), 'null x'),
    (_bwd_ok, dict(dout=None), 'null dout'), (_bwd_ok, dict(w_hh_t=None), 'null w_hh_t'), (_bwd_ok, dict(dgates=None), 'null dgates'),
    (_bwd_ok, dict(w_hh_t=A + 4), 'w_hh_t is not'), (_fwd_ok, dict(gates=A + 4), 'gates is not'),
    (_bwd_ok, dict(B=1048576, T=2), 'dgates of B T 4H'),
])
def test_ok_twins_refuse_and_name_the_reason(fn, kw, reason):
    from animateportrait_amd import _seqapi
    assert fn() == 1
    assert fn(**kw) == 0
    assert reason in _seqapi.last_error(), _seqapi.last_error()


def test_launching_calls_refuse_without_launching():
    from animateportrait_amd import _seqapi
    lib = _seqapi.lib()
    assert lib.apq_lstm_layer_fwd_train(A, A, A, A, A, A, A, A, 17, 18, 161, 128, None) == _seqapi.ERR_UNSUPPORTED
    assert lib.apq_lstm_layer_fwd_train(A, A, A, A, A, A, None, A, 17, 18, 161, H, None) == _seqapi.ERR_INVALID
    assert lib.apq_lstm_layer_bwd(A, A, A, A, A, 17, 18, 128, 0, None) == _seqapi.ERR_UNSUPPORTED
    assert lib.apq_lstm_layer_bwd(A, A, A, A + 4, A, 17, 18, H, 0, None) == _seqapi.ERR_UNSUPPORTED
    assert lib.apq_lstm_layer_bwd(A, A, A, A, A, 17, 0, H, 1, None) == _seqapi.ERR_INVALID


def test_train_backend_switch_and_cpu_fallback():
    from animateportrait_amd import lstm_hip, module1 as m1
    before = m1.get_lstm_train_backend()
    with pytest.raises(ValueError):
        m1.set_lstm_train_backend('nope')
    assert m1.get_lstm_train_backend() == before
    torch.manual_seed(5)
    lstm = torch.nn.LSTM(80, H, 2, batch_first=True).train()
    x = torch.randn(3, 4, 80)
    assert not lstm_hip.supported_train_batched(lstm, x)                             # a CPU tensor
    assert torch.equal(lstm_hip.lstm_train_batched(lstm, x, last_only=True), lstm(x)[0][:, -1, :])
    net = m1.Audio2LandmarkContent().train()
    au, fid = torch.randn(4, 18, 80), torch.randn(1, 204)
    inference = m1.get_lstm_backend()
    outs = {}
    try:
        for name in ('library', 'hip'):
            m1.set_lstm_train_backend(name)
            assert m1.get_lstm_train_backend() == name and m1.get_lstm_backend() == inference
            torch.manual_seed(6)
            outs[name] = net(au, fid)[0]
            assert outs[name].requires_grad
    finally:
        m1.set_lstm_train_backend(before)
    assert torch.equal(outs['library'], outs['hip'])


# ------------------------------------------------------------------------------------------------- dataset and trainer
def _write_dump(dump_dir, n_frames=(60, 60), seed=0):
    """a synthetic dump in the layout main_end2end_module2.py:230-251 writes: per status an au and an fl pickle"""
    rng = np.random.RandomState(seed)
    os.makedirs(dump_dir, exist_ok=True)
    for status in ('train', 'test'):
        au, fl = [], []
        for k, t in enumerate(n_frames):
            info = (k, 'clip%d.wav' % k, np.zeros(256))
            face = rng.randn(1, 204) * 0.3
            au.append((rng.randn(t, 80), info))
            fl.append((np.cumsum(rng.randn(t, 204) * 0.02, 0) + face, info))
        for kind, data in (('au', au), ('fl', fl)):
            with open(os.path.join(dump_dir, 'autovc_retrain_mel_%s_%s.pickle' % (status, kind)), 'wb') as fp:
                pickle.dump(data, fp)


def test_dataset_windows_equal_the_reference_collate(golden, tmp_path):
    from animateportrait_amd import module1_train as mt
    gd = golden('module1_train.npz')
    want = gd['win_index']
    assert want.shape == (42, 18)                                                    # range(0, 60 - 18): the last window is dropped
    assert mt.window_starts(60, 18, 1) == want[:, 0].tolist()
    frames = np.arange(60, dtype=np.float64).reshape(60, 1)
    d = str(tmp_path / 'dump')
    os.makedirs(d)
    for status in ('train', 'test'):
        for kind, width in (('au', 80), ('fl', 204)):
            with open(os.path.join(d, 'autovc_retrain_mel_%s_%s.pickle' % (status, kind)), 'wb') as fp:
                pickle.dump([(frames * np.ones((1, width)), (0, 'a.wav'))], fp)
    ds = mt.ContentDataset(d, status='train')
    fls, aus = ds.windows(0, torch.float64)
    assert fls.shape == (42, 18, 204) and aus.shape == (42, 18, 80)
    assert np.array_equal(fls[:, :, 0].numpy().astype(np.int64), want) and np.array_equal(aus[:, :, 79].numpy().astype(np.int64), want)


def _opt(**kw):
    from animateportrait_amd import module1_train as mt
    o = mt.make_parser().parse_args(['--dump_dir', 'unused', '--ckpt_dir', 'unused', '--nepoch', '1'])
    for k, v in kw.items():
        setattr(o, k, v)
    return o


@pytest.mark.parametrize('lip,motion', [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_loss_gradients_and_adam_step_match_the_reference_in_float64(golden, tmp_path, lip, motion):
    """The trainer's own step (ContentTrainer.train_content, 'library' backend) on the golden's segment: loss, gradient samples
    and norms, parameter samples and norms after the step, to 1e-9 relative -- same expressions, same precision."""
    from animateportrait_amd import module1 as m1, module1_train as mt
    from make_module1_golden import seeded_state
    from make_module1_train_golden import sample_index
    gd = golden('module1_train.npz')
    d = str(tmp_path / 'dump')
    _write_dump(d)
    prev = m1.set_lstm_train_backend('library')
    try:
        tr = mt.ContentTrainer(_opt(dump_dir=d, ckpt_dir=str(tmp_path / 'ck'), use_prior_net=1, use_lip_weight=lip, use_motion_loss=motion,
                                    lr=1e-3, reg_lr=1e-6, lambda_laplacian_smooth_loss=1.0), device='cpu', dtype=torch.float64)
        ks = [(k, tuple(v.shape), str(v.dtype).replace('float64', 'float32')) for k, v in tr.C.state_dict().items()]
        tr.C.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in seeded_state(ks, seed=int(gd['seed'])).items()},
                             strict=True)
        tr.C.train()
        names = [k for k, _ in tr.C.named_parameters()]
        assert names == gd['param_names'].tolist()
        _, loss = tr.train_content(gd['fls'], gd['aus'], gd['face_id'], True)
    finally:
        m1.set_lstm_train_backend(prev)
    tag = 'lip%d_motion%d_' % (lip, motion)
    want = float(gd[tag + 'loss'])
    print('%s loss %.12f (reference %.12f)' % (tag, float(loss), want))
    assert abs(float(loss) - want) <= 1e-9 * abs(want)
    for kind, get in (('grad', lambda p: p.grad), ('adam', lambda p: p.detach())):
        norms, samples = gd[tag + kind + '_norm'].numpy(), gd[tag + kind + '_samples'].numpy()
        for j, (k, p) in enumerate(tr.C.named_parameters()):
            t = get(p)
            if kind == 'grad' and k in BIAS_UNDER_BATCHNORM:
                # exactly zero in exact arithmetic: both sides hold rounding noise, which has no digits to compare
                scale = float(gd[tag + 'grad_norm'][names.index(k.replace('bias', 'weight'))])
                assert float(t.norm()) <= 1e-12 * scale and norms[j] <= 1e-12 * scale, (kind, k)
                continue
            assert abs(float(t.norm()) - norms[j]) <= 1e-9 * norms[j], (kind, k)
            got = t.reshape(-1)[sample_index(t.numel())].numpy()
            assert np.abs(got - samples[j]).max() <= 1e-9 * np.abs(samples[j]).max(), (kind, k)


def test_checkpoint_has_the_reference_keys_and_loads_through_load_module1(tmp_path, golden):
    from animateportrait_amd import module1 as m1, module1_train as mt
    d, ck = str(tmp_path / 'dump'), str(tmp_path / 'ck')
    _write_dump(d)
    for prior in (1, 0):
        tr = mt.ContentTrainer(_opt(dump_dir=d, ckpt_dir=ck, use_prior_net=prior, seed=3), device='cpu')
        (train_loss, eval_loss), = tr.train()
        assert np.isfinite(train_loss) and np.isfinite(eval_loss)
        assert sorted(os.listdir(ck)) == ['ckpt_e_0.pth', 'ckpt_last_epoch.pth']
        saved = torch.load(os.path.join(ck, 'ckpt_last_epoch.pth'), map_location='cpu')
        assert sorted(saved) == ['epoch', 'model_g_face_id'] and saved['epoch'] == 0
        gd = golden('module1.npz')
        assert list(saved['model_g_face_id']) == gd['c_keys'].tolist()                 # the reference network's keys, in its order
        torch.manual_seed(1)
        spk = str(tmp_path / 'g.pth')
        torch.save({'G': m1.Audio2LandmarkPos(drop_out=0.5).state_dict()}, spk)
        _, net_c = m1.load_module1(spk, os.path.join(ck, 'ckpt_last_epoch.pth'))
        assert net_c.use_prior_net == bool(prior) and not net_c.training
        for k, v in net_c.state_dict().items():
            assert torch.equal(v, saved['model_g_face_id'][k]), k
        # ... and a trainer continues from it
        mt.ContentTrainer(_opt(dump_dir=d, ckpt_dir=ck, use_prior_net=prior, load_a2l_C_name=os.path.join(ck, 'ckpt_e_0.pth')), device='cpu')


def test_cli_refuses_use_reg_as_std(tmp_path):
    from animateportrait_amd import module1_train as mt
    with pytest.raises(SystemExit, match='use_reg_as_std'):
        mt.main(['--dump_dir', str(tmp_path), '--ckpt_dir', str(tmp_path), '--nepoch', '1', '--use_reg_as_std'])
    with pytest.raises(NotImplementedError, match='use_reg_as_std'):
        mt.ContentTrainer(argparse.Namespace(use_reg_as_std=True))
    ap = mt.make_parser()
    base = ['--dump_dir', 'd', '--ckpt_dir', 'c', '--nepoch', '2']
    o = ap.parse_args(base)
    assert (o.lr, o.reg_lr, o.lambda_laplacian_smooth_loss) == (1e-3, 1e-6, 1.0)
    assert (o.num_window_frames, o.num_window_step, o.use_lip_weight, o.use_motion_loss, o.in_batch_nepoch) == (18, 1, 1, 0, 1)
    assert (o.hidden_size, o.in_size, o.drop_out, o.use_prior_net, o.lstm) == (256, 80, 0.0, 0, None)
    assert ap.parse_args(base + ['--lstm', 'hip']).lstm == 'hip'
    with pytest.raises(SystemExit):
        ap.parse_args(base + ['--lstm', 'miopen'])


def test_trainer_leaves_the_process_switch_alone_and_main_restores_it(tmp_path):
    from animateportrait_amd import module1 as m1, module1_train as mt
    d, ck = str(tmp_path / 'dump'), str(tmp_path / 'ck')
    _write_dump(d)
    before = m1.get_lstm_train_backend()
    other = 'hip' if before == 'library' else 'library'
    mt.ContentTrainer(_opt(dump_dir=d, ckpt_dir=ck, lstm=other), device='cpu')
    assert m1.get_lstm_train_backend() == before
    assert mt.main(['--dump_dir', d, '--ckpt_dir', ck, '--nepoch', '1', '--lstm', other, '--device', 'cpu', '--seed', '2']) == 0
    assert m1.get_lstm_train_backend() == before and os.path.exists(os.path.join(ck, 'ckpt_last_epoch.pth'))


def test_load_module1_names_a_checkpoint_it_cannot_read(tmp_path):
    from animateportrait_amd import module1 as m1
    torch.manual_seed(1)
    spk, bad = str(tmp_path / 'g.pth'), str(tmp_path / 'c.pth')
    torch.save({'G': m1.Audio2LandmarkPos(drop_out=0.5).state_dict()}, spk)
    sd = m1.Audio2LandmarkContent(use_prior_net=True).state_dict()
    torch.save({'model_g_face_id': {k: v for k, v in sd.items() if not k.startswith('fc_prior')}}, bad)
    with pytest.raises(KeyError, match='fc_prior.0.weight'):
        m1.load_module1(spk, bad)
    sd['bilstm.weight_ih_l0'] = torch.zeros(1024, 100)
    torch.save({'model_g_face_id': sd}, bad)
    with pytest.raises(ValueError, match='width of 100'):
        m1.load_module1(spk, bad)
