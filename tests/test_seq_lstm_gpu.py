"""GPU (-m gpu): the batched LSTM kernel of libapseq.so (csrc/seq/seq_lstm.hip) through lstm_hip.lstm_forward_batched against
nn.LSTM in float64 on the CPU, at the sizes where it can go wrong -- one row, one step, an odd input width (K tail, rows of
w_ih and x off the 16-byte grid), a batch that is no multiple of the 16-row tile, several workgroups -- and Module1's two
networks on that path against the reference-made golden (tests/golden/module1.npz)."""
import sys

import numpy as np
import pytest
import torch

from conftest import linf, GOLDEN

sys.path.insert(0, GOLDEN)
pytestmark = pytest.mark.gpu

BAR = 2e-5           # L-inf on outputs bounded by 1: the bar of the batch-1 kernel (test_module1_gpu.py)
CASES = [(1, 1, 80, 1), (5, 2, 161, 1), (16, 18, 80, 3), (17, 18, 161, 3), (33, 3, 256, 2), (512, 18, 161, 3)]
_REF = {}


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


def _case(b, t, i, layers):
    """(lstm on the CPU in fp32, x (B, T, I), float64 reference (B, T, 256)) -- computed once per case, never modified"""
    key = (b, t, i, layers)
    if key not in _REF:
        torch.manual_seed(1000 * i + 10 * b + layers)
        lstm = torch.nn.LSTM(i, 256, layers, batch_first=True).eval()
        x = torch.randn(b, t, i)
        with torch.no_grad():
            l64 = torch.nn.LSTM(i, 256, layers, batch_first=True).double().eval()
            l64.load_state_dict({k: v.double() for k, v in lstm.state_dict().items()})
            ref = l64(x.double())[0]
        _REF[key] = (lstm, x, ref)
    return _REF[key]


def _on(dev, lstm):
    import copy
    return copy.deepcopy(lstm).to(dev).eval()


@pytest.mark.parametrize('last_only', [False, True])
@pytest.mark.parametrize('cfg', CASES)
def test_batched_lstm_kernel_against_float64(dev, cfg, last_only):
    from animateportrait_amd import lstm_hip
    b, t, i, layers = cfg
    lstm, x, ref = _case(*cfg)
    dl, dx = _on(dev, lstm), x.to(dev)
    with torch.no_grad():
        assert lstm_hip.supported_batched(dl, dx)
        got = lstm_hip.lstm_forward_batched(dl, dx, last_only=last_only)
    torch.cuda.synchronize()
    want = ref[:, -1, :] if last_only else ref
    assert got.shape == want.shape and got.dtype == torch.float32
    err = float((got.cpu().double() - want).abs().max())
    print('B=%d T=%d I=%d layers=%d last_only=%d: L-inf vs float64 = %.3e' % (b, t, i, layers, last_only, err))
    assert err < BAR


def test_tile_tails_leak_nothing(dev):
    """B = 17 is one full tile and a tile of one row: the 15 rows that tile lacks are neither read (NaN behind x) nor written
    (sentinels behind out)."""
    from animateportrait_amd import _seqapi as Q, ops
    b, t, i, layers = 17, 18, 161, 1
    lstm, x, ref = _case(b, t, i, layers)
    dl = _on(dev, lstm)
    xbuf = torch.full((b + 16, t, i), float('nan'), device=dev)
    xbuf[:b] = x.to(dev)
    obuf = torch.full((b + 8, t, 256), 12345.0, device=dev)
    before = obuf.clone()
    dx, out = xbuf[:b], obuf[:b]
    assert dx.is_contiguous() and out.is_contiguous()
    w = [getattr(dl, n + '_l0').contiguous() for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')]
    args = [ops._ptr(a) for a in [dx] + w + [out]]
    assert Q.lib().apq_lstm_layer_fwd_ok(*args, b, t, i, 256, 0) == 1
    Q.check(Q.lib().apq_lstm_layer_fwd(*args, b, t, i, 256, 0, ops._stream()), 'lstm_layer_fwd')
    torch.cuda.synchronize()
    assert bool(torch.isfinite(obuf[:b]).all())
    assert float((obuf[:b].cpu().double() - ref).abs().max()) < BAR
    assert torch.equal(obuf[b:].view(torch.int32), before[b:].view(torch.int32))


def test_rows_are_independent_of_their_place_in_the_batch(dev):
    from animateportrait_amd import lstm_hip
    lstm, x, _ = _case(33, 3, 256, 2)
    dl, dx = _on(dev, lstm), x.to(dev)
    with torch.no_grad():
        a = lstm_hip.lstm_forward_batched(dl, dx)
        r = lstm_hip.lstm_forward_batched(dl, dx.flip(0).contiguous())
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int32), r.flip(0).view(torch.int32))


def test_last_only_is_the_last_step_of_the_full_output(dev):
    from animateportrait_amd import lstm_hip
    lstm, x, _ = _case(17, 18, 161, 3)
    dl, dx = _on(dev, lstm), x.to(dev)
    with torch.no_grad():
        full = lstm_hip.lstm_forward_batched(dl, dx)
        last = lstm_hip.lstm_forward_batched(dl, dx, last_only=True)
    torch.cuda.synchronize()
    assert last.shape == (17, 256) and torch.equal(last.view(torch.int32), full[:, -1, :].contiguous().view(torch.int32))


@pytest.fixture()
def hip_backend():
    from animateportrait_amd import module1 as m1
    prev = m1.set_lstm_backend('hip')
    yield m1
    m1.set_lstm_backend(prev)


def _nets(gd, dev):
    from animateportrait_amd import module1 as m1
    from test_stream_cpu import _seeded
    netc = _seeded(m1.Audio2LandmarkContent(use_prior_net=True, drop_out=0.5), gd, 'c_', 78)
    netg = _seeded(m1.Audio2LandmarkPos(drop_out=0.5), gd, 'g_', 79)
    return netc.to(dev), netg.to(dev)


def test_module1_networks_on_the_batched_kernel_match_reference_golden(dev, golden, hip_backend):
    """test_module1_gpu.py's network test with both LSTMs on apq_lstm_layer_fwd, at its bars."""
    from animateportrait_amd import lstm_hip
    gd = golden('module1.npz')
    netc, netg = _nets(gd, dev)
    with torch.no_grad():
        assert lstm_hip.supported_batched(netg.audio_content_encoder, gd['au'].to(dev))
        assert lstm_hip.supported_batched(netc.bilstm, torch.zeros(6, 18, 161, device=dev))
        c = netc(gd['au'].to(dev), gd['fid'].to(dev))[0]
        pred, face, spk = netg(gd['au'].to(dev), gd['g_emb'].to(dev), gd['fid'].repeat(6, 1).to(dev), None,
                               torch.zeros(6, 128, device=dev))
    assert linf(c, gd['c_out']) < 2e-5 * float(gd['c_out'].abs().max()) + 1e-6
    assert linf(pred, gd['g_out']) < 2e-5 * float(gd['g_out'].abs().max()) + 1e-6


def test_module1_clip_pipeline_on_the_batched_kernel_matches_reference_methods(dev, golden, hip_backend):
    """predict_landmarks_speaker_aware over the golden's 600 windows (segments of 512 and 88) to 1e-4 of the landmark range."""
    gd = golden('module1.npz')
    netc, netg = _nets(gd, dev)
    gp = torch.Generator().manual_seed(int(gd['p_seed']))
    au = torch.randn(int(gd['p_T']), 18, 80, generator=gp)
    spk = torch.randn(256, generator=gp)
    fl = hip_backend.predict_landmarks_speaker_aware(netg, netc, au, spk, gd['fid'].view(-1))
    ref = gd['p_sub'].numpy()
    assert fl.shape == (600, 204) and np.abs(fl[::16] - ref).max() < 1e-4 * np.abs(ref).max()
