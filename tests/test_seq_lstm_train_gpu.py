"""GPU (-m gpu): the training kernel pair of libapseq.so (csrc/seq/seq_lstm_train.hip) -- apq_lstm_layer_fwd_train against
apq_lstm_layer_fwd (bit-equal output) and a float64 restatement (gates, cell), apq_lstm_layer_bwd and the autograd function
around it against the float64 CPU autograd of nn.LSTM, and the content-branch trainer (module1_train.py) on that path.

The bar of every gradient check is measured, not chosen: the error of PyTorch-ROCm's own fp32 nn.LSTM backward on the device
against the same float64 reference.  The kernel route passes at 4 x that error (a different summation order over K = 1024 and
T steps), with a floor of 1e-6 of the tensor's range.  Both errors are printed per tensor (``ERR ...`` lines).

dG, which nn.LSTM does not expose, is read off its autograd like this: the layer gets 4H more input features e = 0 whose
weights are the identity, so that gates_t = W_ih x_t + e_t + ..., and d loss / d e_t is dG_t."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

H = 256
SHAPES = [(1, 1, 80), (17, 3, 161), (16, 18, 256), (33, 2, 5)]
FWD_BAR = 2e-5        # L-inf on values bounded by 1: the bar of the forward kernel's own test (test_seq_lstm_gpu.py)
_REF = {}


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


def _grads_via_autograd(lstm_sd, x, dout, last_only, device, dtype):
    """One-layer nn.LSTM with the identity-extended input (see the module docstring) on ``device`` in ``dtype``:
    {'dG', 'dx', 'dW_ih', 'dW_hh', 'db_ih', 'db_hh'} for loss = sum(out * dout), or sum(out[:, -1] * dout) with last_only."""
    b, t, i = x.shape
    lstm = torch.nn.LSTM(i + 4 * H, H, 1, batch_first=True).to(device=device, dtype=dtype)
    with torch.no_grad():
        lstm.weight_ih_l0.copy_(torch.cat([lstm_sd['weight_ih_l0'].to(dtype), torch.eye(4 * H, dtype=dtype)], 1))
        for n in ('weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0'):
            getattr(lstm, n).copy_(lstm_sd[n].to(dtype))
    xe = torch.cat([x.to(dtype), torch.zeros(b, t, 4 * H, dtype=dtype)], 2).to(device).requires_grad_(True)
    out = lstm(xe)[0]
    d = dout.to(device=device, dtype=dtype)
    ((out[:, -1, :] if last_only else out) * d).sum().backward()
    return {'dG': xe.grad[:, :, i:], 'dx': xe.grad[:, :, :i], 'dW_ih': lstm.weight_ih_l0.grad[:, :i], 'dW_hh': lstm.weight_hh_l0.grad,
            'db_ih': lstm.bias_ih_l0.grad, 'db_hh': lstm.bias_hh_l0.grad}


def _restate64(sd, x):
    """(out, gates, cell) of the layer in float64: the formulas of include/animateportrait_seq.h, step by step"""
    w_ih, w_hh, b_ih, b_hh = (sd[n + '_l0'].double() for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh'))
    b, t, _ = x.shape
    h, c = torch.zeros(b, H, dtype=torch.float64), torch.zeros(b, H, dtype=torch.float64)
    outs, gates, cells = [], [], []
    for s in range(t):
        pre = x[:, s].double() @ w_ih.t() + b_ih + h @ w_hh.t() + b_hh
        gi, gf, gg, go = torch.sigmoid(pre[:, :H]), torch.sigmoid(pre[:, H:2 * H]), torch.tanh(pre[:, 2 * H:3 * H]), torch.sigmoid(pre[:, 3 * H:])
        c = gf * c + gi * gg
        h = go * torch.tanh(c)
        outs.append(h)
        gates.append(torch.cat([gi, gf, gg, go], 1))
        cells.append(c)
    return torch.stack(outs, 1), torch.stack(gates, 1), torch.stack(cells, 1)


def _case(b, t, i):
    """(state dict of a one-layer nn.LSTM in fp32, x, dout (B, T, H), float64 references) -- computed once per shape, never modified"""
    key = (b, t, i)
    if key not in _REF:
        torch.manual_seed(1000 * i + 10 * b + t)
        sd = {k: v.detach().clone() for k, v in torch.nn.LSTM(i, H, 1, batch_first=True).state_dict().items()}
        x, dout = torch.randn(b, t, i), torch.randn(b, t, H)
        ref = {lo: {k: v.detach() for k, v in _grads_via_autograd(sd, x, dout[:, -1] if lo else dout, lo, 'cpu', torch.float64).items()}
               for lo in (0, 1)}
        _REF[key] = (sd, x, dout, ref, _restate64(sd, x))
    return _REF[key]


def _device_layer(sd, dev):
    return [sd[n + '_l0'].to(dev).contiguous() for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')]


def _fwd_train(w, x):
    from animateportrait_amd import _seqapi as Q, ops
    b, t, i = x.shape
    out, gates, cell = (torch.empty(b, t, n, device=x.device) for n in (H, 4 * H, H))
    args = [ops._ptr(a) for a in [x] + w + [out, gates, cell]]
    assert Q.lib().apq_lstm_layer_fwd_train_ok(*args, b, t, i, H) == 1, Q.last_error()
    Q.check(Q.lib().apq_lstm_layer_fwd_train(*args, b, t, i, H, ops._stream()), 'lstm_layer_fwd_train')
    return out, gates, cell


def _bwd(w, dout, gates, cell, last_only):
    from animateportrait_amd import _seqapi as Q, ops
    b, t, _ = gates.shape
    w_hh_t = w[1].t().contiguous()
    dg = torch.empty(b, t, 4 * H, device=gates.device)
    args = [ops._ptr(a) for a in (dout, gates, cell, w_hh_t, dg)]
    assert Q.lib().apq_lstm_layer_bwd_ok(*args, b, t, H, last_only) == 1, Q.last_error()
    Q.check(Q.lib().apq_lstm_layer_bwd(*args, b, t, H, last_only, ops._stream()), 'lstm_layer_bwd')
    return dg


def _hold(name, got, lib, ref, what):
    """the measured bar: kernel error <= max(4 x library error, 1e-6 of the tensor's range)"""
    ref = ref.double().cpu()
    e_k, e_l = float((got.double().cpu() - ref).abs().max()), float((lib.double().cpu() - ref).abs().max())
    rng = float(ref.abs().max())
    print('ERR %s %s kernel=%.3e library=%.3e range=%.3e' % (what, name, e_k, e_l, rng))
    assert e_k <= max(4.0 * e_l, 1e-6 * rng), (what, name, e_k, e_l, rng)


@pytest.mark.parametrize('bti', SHAPES)
def test_fwd_train_is_the_forward_bit_for_bit_and_its_gates_match_float64(dev, bti):
    from animateportrait_amd import _seqapi as Q, ops
    sd, x, _, _, (out64, gates64, cell64) = _case(*bti)
    b, t, i = bti
    w, dx = _device_layer(sd, dev), x.to(dev)
    out, gates, cell = _fwd_train(w, dx)
    plain = torch.empty(b, t, H, device=dev)
    Q.check(Q.lib().apq_lstm_layer_fwd(*[ops._ptr(a) for a in [dx] + w + [plain]], b, t, i, H, 0, ops._stream()), 'lstm_layer_fwd')
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), plain.view(torch.int32))
    e_o, e_g = float((out.cpu().double() - out64).abs().max()), float((gates.cpu().double() - gates64).abs().max())
    e_c, c_max = float((cell.cpu().double() - cell64).abs().max()), float(cell64.abs().max())
    print('B=%d T=%d I=%d: L-inf vs float64: out %.3e gates %.3e cell %.3e (|c| up to %.3f)' % (b, t, i, e_o, e_g, e_c, c_max))
    assert e_o < FWD_BAR and e_g < FWD_BAR and e_c < FWD_BAR * max(1.0, c_max)


@pytest.mark.parametrize('last_only', [0, 1])
@pytest.mark.parametrize('bti', SHAPES)
def test_bwd_and_the_autograd_route_against_float64_autograd(dev, bti, last_only):
    from animateportrait_amd import lstm_hip
    sd, x, dout, ref, _ = _case(*bti)
    b, t, i = bti
    what = 'B=%d,T=%d,I=%d,last_only=%d' % (b, t, i, last_only)
    d = (dout[:, -1] if last_only else dout).contiguous()
    lib = _grads_via_autograd(sd, x, d, last_only, dev, torch.float32)
    # dG from the two calls themselves
    w = _device_layer(sd, dev)
    _, gates, cell = _fwd_train(w, x.to(dev))
    dg = _bwd(w, d.to(dev), gates, cell, last_only)
    torch.cuda.synchronize()
    _hold('dG', dg, lib['dG'], ref[last_only]['dG'], what)
    # everything else through the autograd function
    lstm = torch.nn.LSTM(i, H, 1, batch_first=True)
    lstm.load_state_dict(sd)
    lstm = lstm.to(dev).train()
    xg = x.to(dev).requires_grad_(True)
    assert lstm_hip.supported_train_batched(lstm, xg)
    out = lstm_hip.lstm_train_batched(lstm, xg, last_only=bool(last_only))
    assert out.shape == ((b, H) if last_only else (b, t, H))
    (out * d.to(dev)).sum().backward()
    torch.cuda.synchronize()
    got = {'dx': xg.grad, 'dW_ih': lstm.weight_ih_l0.grad, 'dW_hh': lstm.weight_hh_l0.grad, 'db_ih': lstm.bias_ih_l0.grad,
           'db_hh': lstm.bias_hh_l0.grad}
    for name, g in got.items():
        _hold(name, g, lib[name], ref[last_only][name], what)


@pytest.mark.parametrize('last_only', [0, 1])
def test_three_layer_stack_against_float64_autograd(dev, last_only):
    from animateportrait_amd import lstm_hip
    b, t, i = 20, 4, 80
    torch.manual_seed(77)
    cpu = torch.nn.LSTM(i, H, 3, batch_first=True)
    x, dout = torch.randn(b, t, i), torch.randn(b, H) if last_only else torch.randn(b, t, H)

    def grads(lstm, xin, route):
        xin = xin.requires_grad_(True)
        out = route(lstm, xin)
        (out * dout.to(device=xin.device, dtype=xin.dtype)).sum().backward()
        return dict([('dx', xin.grad)] + [(k, p.grad) for k, p in lstm.named_parameters()])

    def module(lstm, xin):
        out = lstm(xin)[0]
        return out[:, -1, :] if last_only else out

    def copy(device, dtype):
        m = torch.nn.LSTM(i, H, 3, batch_first=True)
        m.load_state_dict(cpu.state_dict())
        return m.to(device=device, dtype=dtype).train()

    ref = grads(copy('cpu', torch.float64), x.double(), module)
    lib = grads(copy(dev, torch.float32), x.to(dev), module)
    got = grads(copy(dev, torch.float32), x.to(dev), lambda l, xin: lstm_hip.lstm_train_batched(l, xin, last_only=bool(last_only)))
    torch.cuda.synchronize()
    assert sorted(got) == sorted(ref) and len(got) == 13
    for name in ref:
        _hold(name, got[name], lib[name], ref[name], 'stack3,B=20,T=4,I=80,last_only=%d' % last_only)


def test_a_row_does_not_depend_on_its_place_in_the_batch_and_runs_repeat(dev):
    sd, x, dout, _, _ = _case(33, 2, 5)
    w = _device_layer(sd, dev)
    _, gates, cell = _fwd_train(w, x.to(dev))
    full = _bwd(w, dout.to(dev), gates, cell, 0)
    again = _bwd(w, dout.to(dev), gates, cell, 0)
    _, g1, c1 = _fwd_train(w, x[20:21].contiguous().to(dev))
    one = _bwd(w, dout[20:21].contiguous().to(dev), g1, c1, 0)
    torch.cuda.synchronize()
    assert torch.equal(full.view(torch.int32), again.view(torch.int32))
    assert torch.equal(g1.view(torch.int32), gates[20:21].view(torch.int32)) and torch.equal(c1.view(torch.int32), cell[20:21].view(torch.int32))
    assert torch.equal(one.view(torch.int32), full[20:21].view(torch.int32))


def test_refused_calls_leave_their_outputs_untouched(dev):
    from animateportrait_amd import _seqapi as Q, ops
    b, t, i = 5, 2, 80
    x, w_ih, w_hh, bias = (torch.zeros(n, device=dev) for n in (b * t * i, 512 * i, 512 * 128, 512))
    outs = [torch.full((b * t * n,), 12345.0, device=dev) for n in (H, 4 * H, H, 4 * H)]
    lib = Q.lib()
    p = ops._ptr
    assert lib.apq_lstm_layer_fwd_train(p(x), p(w_ih), p(w_hh), p(bias), p(bias), p(outs[0]), p(outs[1]), p(outs[2]), b, t, i, 128,
                                        ops._stream()) == Q.ERR_UNSUPPORTED
    assert 'H = 128' in Q.last_error()
    assert lib.apq_lstm_layer_bwd(p(outs[0]), p(outs[1]), p(outs[2]), p(w_hh), p(outs[3]), b, t, 128, 0, ops._stream()) == Q.ERR_UNSUPPORTED
    assert 'H = 128' in Q.last_error()
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o == 12345.0).all())


# ------------------------------------------------------------------------------------------------------------ the trainer
def _write_dump(dump_dir, n_frames=(60, 60), seed=0):
    rng = np.random.RandomState(seed)
    os.makedirs(dump_dir, exist_ok=True)
    for status in ('train', 'test'):
        au, fl = [], []
        for k, n in enumerate(n_frames):
            info = (k, 'clip%d.wav' % k, np.zeros(256))
            au.append((rng.randn(n, 80), info))
            fl.append((np.cumsum(rng.randn(n, 204) * 0.02, 0) + rng.randn(1, 204) * 0.3, info))
        for kind, data in (('au', au), ('fl', fl)):
            with open(os.path.join(dump_dir, 'autovc_retrain_mel_%s_%s.pickle' % (status, kind)), 'wb') as fp:
                pickle.dump(data, fp)


def test_one_trainer_step_hip_against_library(dev, tmp_path, monkeypatch):
    """One ContentTrainer step on a 24-window segment, 'hip' against the trainer in float64 on the CPU, at the bar measured on
    the 'library' route: the loss, every parameter's GRADIENT (the figure that sees a wrong factor: Adam's first step is about
    lr * sign(g), so the updated parameters see little more than the gradient's sign), and the updated parameters.  The three biases under a
    BatchNorm, whose gradient is zero in exact arithmetic, are held like every other tensor: their float64 reference is ~1e-19,
    so the figure compared is each route's rounding noise, the kernel route's against 4 x the library's.  The 'hip'
    step must have gone through the kernels: once, on a served shape."""
    from animateportrait_amd import lstm_hip, module1 as m1, module1_train as mt
    d = str(tmp_path / 'dump')
    _write_dump(d)
    g = torch.Generator().manual_seed(5)
    face = torch.randn(1, 204, generator=g) * 0.3
    walk = torch.cumsum(torch.randn(24 + 18, 204, generator=g) * 0.02, 0) + face
    fls, aus = torch.stack([walk[k:k + 18] for k in range(24)]), torch.randn(24, 18, 80, generator=g)
    opt = mt.make_parser().parse_args(['--dump_dir', d, '--ckpt_dir', str(tmp_path / 'ck'), '--nepoch', '1', '--use_prior_net', '1'])
    torch.manual_seed(9)
    sd0 = m1.Audio2LandmarkContent(use_prior_net=True).state_dict()
    served = []
    route = lstm_hip.lstm_train_batched

    def counted(lstm, x, last_only=False):
        served.append(lstm_hip.supported_train_batched(lstm, x))
        return route(lstm, x, last_only=last_only)

    monkeypatch.setattr(lstm_hip, 'lstm_train_batched', counted)
    res = {}
    prev = m1.get_lstm_train_backend()
    try:
        for name, device, dtype in (('ref', 'cpu', torch.float64), ('library', dev, torch.float32), ('hip', dev, torch.float32)):
            m1.set_lstm_train_backend('hip' if name == 'hip' else 'library')
            tr = mt.ContentTrainer(opt, device=device, dtype=dtype)
            assert m1.get_lstm_train_backend() == ('hip' if name == 'hip' else 'library')      # the trainer leaves the switch alone
            tr.C.load_state_dict({k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd0.items()})
            tr.C.train()
            _, loss = tr.train_content(fls.to(device=device, dtype=dtype), aus.to(device=device, dtype=dtype),
                                       face.to(device=device, dtype=dtype), True)
            assert served == ([True] if name == 'hip' else []), (name, served)
            res[name] = (loss, {k: p.grad.detach().clone() for k, p in tr.C.named_parameters()},
                         {k: p.detach() for k, p in tr.C.named_parameters()})
    finally:
        m1.set_lstm_train_backend(prev)
    torch.cuda.synchronize()
    _hold('loss', res['hip'][0].reshape(1), res['library'][0].reshape(1), res['ref'][0].reshape(1), 'trainer_step')
    for k in res['ref'][1]:
        _hold('grad:' + k, res['hip'][1][k], res['library'][1][k], res['ref'][1][k], 'trainer_step')
    for k in res['ref'][2]:
        _hold('adam:' + k, res['hip'][2][k], res['library'][2][k], res['ref'][2][k], 'trainer_step')


def test_cli_trains_an_epoch_on_the_kernels_and_its_checkpoint_predicts(dev, tmp_path):
    from animateportrait_amd import module1 as m1
    d, ck = str(tmp_path / 'dump'), str(tmp_path / 'ck')
    _write_dump(d)
    got = subprocess.run([sys.executable, '-m', 'animateportrait_amd.module1_train', '--dump_dir', d, '--ckpt_dir', ck, '--nepoch', '1',
                          '--lstm', 'hip', '--seed', '1'], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert got.returncode == 0, got.stderr[-2000:]
    lines = [ln for ln in got.stdout.split('\n') if ln.startswith(('TRAIN Epoch', 'EVAL Epoch'))]
    assert len(lines) == 2, got.stdout
    for ln in lines:
        assert np.isfinite(float(ln.split('loss')[1].split()[0])), ln
    saved = torch.load(os.path.join(ck, 'ckpt_last_epoch.pth'), map_location='cpu')
    assert sorted(saved) == ['epoch', 'model_g_face_id']
    net = m1.Audio2LandmarkContent()
    net.load_state_dict(saved['model_g_face_id'])
    fl = m1.predict_landmarks(net.to(dev), torch.randn(30, 18, 80), torch.randn(204) * 0.1)
    fl = fl.cpu().numpy() if torch.is_tensor(fl) else fl
    assert fl.shape == (30, 68, 2) and np.isfinite(fl).all()
