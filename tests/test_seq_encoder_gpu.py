"""GPU (-m gpu): the encoder kernels of libapseq.so (csrc/seq/seq_encoder.hip) through encoder_hip.encoder_forward against the
float64 statement (tests/encoder_reference.py) and against the stock fp32 path on the same device, at the sizes where they can go
wrong -- a single key, the 16-row tile's boundary and its tails, a batch, the maximum, the smallest and the usual d_ff, large
logits, a constant row -- then the pose network and the clip loop on that path against the reference-made golden
(tests/golden/module1.npz), and end2end with --module1_encoder hip.

The parity bar: with e_hip and e_lib the L-inf distances of the kernel path and of the stock fp32 path to the float64 statement,
e_hip <= 4 e_lib + 1e-6 max|ref|.  The kernels sum K in chunks of four and reduce the softmax in another tree than the library:
they may not be worse than a small multiple of the library's own error (4: the margin the LSTM backward has).  Observed on the
MI355X: e_hip 6.9e-7 .. 5.3e-6 against e_lib 6.3e-7 .. 3.5e-6 over all cases (profiles/module1_encoder.json has them per shape)."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import encoder_reference as er
from test_seq_encoder_cpu import SHAPES, make_encoder, make_x

sys.path.insert(0, GOLDEN)
pytestmark = pytest.mark.gpu

_REF = {}


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


def _variant(kind):
    """(encoder on the CPU, fp32) of a named variant -- built once, never modified"""
    key = ('enc', kind)
    if key not in _REF:
        if kind == 'ff256':
            enc = make_encoder(d_ff=256, seed=6)
        else:
            enc = make_encoder()
        with torch.no_grad():
            if kind == 'logits':
                # layer 0's q and k projections scaled up: the scores leave the range where exp() without the maximum survives
                enc.layers[0].attn.q_linear.weight.mul_(LOGIT_FACTOR)
                enc.layers[0].attn.k_linear.weight.mul_(LOGIT_FACTOR)
            if kind == 'constant':
                # every row of layer 0's input is the same constant: std = 0, Norm_1 divides by eps alone
                enc.embed.embed.weight.zero_()
                enc.embed.embed.bias.fill_(0.25)
                enc.pe.pe.zero_()
        _REF[key] = enc
    return _REF[key]


LOGIT_FACTOR = 6.0           # picked on the CPU: layer 0's scores then span -122 .. 118 at T = 33 and -179 .. 171 at T = 113


def _case(kind, b, t):
    """(encoder, x, float64 statement) -- computed once per case, never modified"""
    key = (kind, b, t)
    if key not in _REF:
        enc, x = _variant(kind), make_x(b, t)
        _REF[key] = (enc, x, er.encoder_forward(x.numpy(), er.params_of(enc)))
    return _REF[key]


def _both(dev, enc, x):
    """(kernel path, stock path) on the device, fp32"""
    from animateportrait_amd import encoder_hip, module1 as m1
    de, dx = copy.deepcopy(enc).to(dev).eval(), x.to(dev)
    assert m1.get_encoder_backend() == 'library'
    with torch.no_grad():
        lib = de(dx)
        assert encoder_hip.supported(de, dx)
        hip = encoder_hip.encoder_forward(de, dx)
    torch.cuda.synchronize()
    assert hip.shape == lib.shape and hip.dtype == torch.float32 and hip.is_contiguous()
    return hip, lib


def _parity(what, hip, lib, ref):
    e_hip = float(np.abs(hip.cpu().double().numpy() - ref).max())
    e_lib = float(np.abs(lib.cpu().double().numpy() - ref).max())
    bar = 4 * e_lib + 1e-6 * float(np.abs(ref).max())
    print('%s: e_hip %.3e  e_lib %.3e  bar %.3e  max|ref| %.3e' % (what, e_hip, e_lib, bar, np.abs(ref).max()))
    assert bool(torch.isfinite(hip).all())
    assert e_hip <= bar


@pytest.mark.parametrize('bt', SHAPES)
def test_encoder_kernels_against_float64_and_the_library(dev, bt):
    enc, x, ref = _case('plain', *bt)
    hip, lib = _both(dev, enc, x)
    _parity('B=%d T=%d d_ff=2048' % bt, hip, lib, ref)


@pytest.mark.parametrize('bt', [(1, 17), (2, 33)])
def test_smallest_served_d_ff_runs_the_chunk_loop_once(dev, bt):
    from animateportrait_amd import _seqapi as Q
    enc, x, ref = _case('ff256', *bt)
    assert enc.layers[0].ff.linear_1.out_features == Q.ENC_FF_CHUNK
    hip, lib = _both(dev, enc, x)
    _parity('B=%d T=%d d_ff=256' % bt, hip, lib, ref)


@pytest.mark.parametrize('bt', [(1, 33), (1, 113)])
def test_large_logits_need_the_maximum_subtracted(dev, bt):
    enc, x, ref = _case('logits', *bt)
    p = er.params_of(enc)
    h = er.embed(x.numpy(), p)
    s = er.attention_scores(er.norm(h, p['layers.0.norm_1.alpha'], p['layers.0.norm_1.bias']), p, 'layers.0.', 2)
    print('scores of layer 0: %.1f .. %.1f' % (s.min(), s.max()))
    assert s.max() > 100 and s.min() < -100          # exp(100) is beyond fp32: a softmax without the maximum gives inf / inf
    hip, lib = _both(dev, enc, x)
    assert bool(torch.isfinite(lib).all())
    _parity('B=%d T=%d large logits' % bt, hip, lib, ref)


def test_constant_rows_divide_by_eps_alone(dev):
    enc, x, ref = _case('constant', 1, 17)
    p = er.params_of(enc)
    h = er.embed(x.numpy(), p)
    assert float(np.ptp(h, axis=-1).max()) == 0.0 and float(h[0, 0, 0]) == 2.0
    hip, lib = _both(dev, enc, x)
    _parity('constant rows', hip, lib, ref)


def test_keys_beyond_t_are_never_read_and_calls_repeat(dev):
    """T = 17: the second tile has one row, the last key tile one key.  q, k and v lie a third of the workspace apart: with an
    oversize workspace full of NaN every row behind each of them is NaN -- and the output is finite and has the bits of the run with
    a tight workspace.  A second call has the same bits."""
    from animateportrait_amd import encoder_hip
    enc, x, ref = _case('plain', 1, 17)
    de, dx = copy.deepcopy(enc).to(dev).eval(), x.to(dev)
    n = encoder_hip.workspace_elements(1, 17)
    tight = torch.full((n,), float('nan'), device=dev)
    wide = torch.full((3 * (17 + 40) * 64,), float('nan'), device=dev)
    with torch.no_grad():
        a = encoder_hip.encoder_forward(de, dx, workspace=tight)
        b = encoder_hip.encoder_forward(de, dx, workspace=wide)
        c = encoder_hip.encoder_forward(de, dx)
        d = encoder_hip.encoder_forward(de, dx)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())
    for other in (b, c, d):
        assert torch.equal(a.view(torch.int32), other.view(torch.int32))
    # the rows behind q, k and v were not written either
    third = wide.numel() // 3
    for i in range(3):
        assert bool(torch.isfinite(wide[i * third:i * third + 17 * 64]).all())
        assert bool(torch.isnan(wide[i * third + 17 * 64:(i + 1) * third]).all())
    with pytest.raises(ValueError):
        encoder_hip.encoder_forward(de, dx, workspace=tight[:-1])


def test_one_layer_by_hand_leaves_the_floats_behind_its_outputs_alone(dev):
    """Layer 0 through the C calls on buffers with sentinels behind x's 17 rows, q, k, v and y -- and without the closing Norm."""
    from animateportrait_amd import _seqapi as Q, encoder_hip as eh, ops
    enc, x, _ = _case('plain', 1, 17)
    de = copy.deepcopy(enc).to(dev).eval()
    layer = de.layers[0]
    t, pad = 17, 24
    h = torch.randn(1, t, 64, generator=torch.Generator().manual_seed(4)).to(dev)
    bufs = {n: torch.full((t + pad, 64), 12345.0, device=dev) for n in 'qkvy'}
    before = {n: b.clone() for n, b in bufs.items()}
    lt = eh._layer_tensors(layer)
    q, k, v, y = (ops._ptr(bufs[n]) for n in 'qkvy')
    lib = Q.lib()
    qa = eh._qkv_args(layer, lt, ops._ptr(h), q, k, v, 1, t, 64)
    aa = eh._attn_args(layer, lt, None, ops._ptr(h), q, k, v, y, 1, t, 64)
    assert lib.apq_enc_qkv_ok(*qa) == 1 and lib.apq_enc_attn_ff_ok(*aa) == 1
    Q.check(lib.apq_enc_qkv(*qa, ops._stream()), 'enc_qkv')
    Q.check(lib.apq_enc_attn_ff(*aa, ops._stream()), 'enc_attn_ff')
    torch.cuda.synchronize()
    for n in 'qkvy':
        assert torch.equal(bufs[n][t:].view(torch.int32), before[n][t:].view(torch.int32)), n
        assert bool(torch.isfinite(bufs[n][:t]).all()) and not bool((bufs[n][:t] == 12345.0).any()), n
    with torch.no_grad():
        lib_out = layer(h, None)
    p = {k_: v_.detach().cpu().double().numpy() for k_, v_ in layer.state_dict().items()}
    ref = er.encoder_layer(h.cpu().double().numpy(), p, '', 2)
    _parity('layer 0 alone', bufs['y'][:t].view(1, t, 64), lib_out, ref)


def test_a_sequence_does_not_depend_on_its_place_in_the_batch(dev):
    from animateportrait_amd import encoder_hip
    enc, x, _ = _case('plain', 3, 17)
    de, dx = copy.deepcopy(enc).to(dev).eval(), x.to(dev)
    with torch.no_grad():
        three = encoder_hip.encoder_forward(de, dx)
        alone = encoder_hip.encoder_forward(de, dx[1:2].contiguous())
    torch.cuda.synchronize()
    assert torch.equal(three[1].view(torch.int32), alone[0].view(torch.int32))


def test_encoder_forward_switches_on_the_backend(dev):
    """``Encoder.forward`` itself: the kernels with 'hip', the stock modules with a mask."""
    from animateportrait_amd import encoder_hip, module1 as m1
    enc, x, _ = _case('plain', 1, 33)
    de, dx = copy.deepcopy(enc).to(dev).eval(), x.to(dev)
    with torch.no_grad():
        lib = de(dx)
        direct = encoder_hip.encoder_forward(de, dx)
        prev = m1.set_encoder_backend('hip')
        try:
            hip = de(dx)
            masked = de(dx, torch.ones(1, 33, 33, device=dev))
        finally:
            m1.set_encoder_backend(prev)
    assert torch.equal(hip, direct) and torch.equal(masked, lib)


@pytest.fixture()
def hip_encoder():
    from animateportrait_amd import module1 as m1
    prev = m1.set_encoder_backend('hip')
    yield m1
    m1.set_encoder_backend(prev)


def _nets(gd, dev):
    from animateportrait_amd import module1 as m1
    from test_stream_cpu import _seeded
    netc = _seeded(m1.Audio2LandmarkContent(use_prior_net=True, drop_out=0.5), gd, 'c_', 78)
    netg = _seeded(m1.Audio2LandmarkPos(drop_out=0.5), gd, 'g_', 79)
    return netc.to(dev), netg.to(dev)


def test_pose_network_on_the_encoder_kernels_matches_reference_golden(dev, golden, hip_encoder):
    """test_module1_gpu.py's network test with the pose network's encoder on the kernels, at its bar."""
    from animateportrait_amd import encoder_hip
    from conftest import linf
    gd = golden('module1.npz')
    netc, netg = _nets(gd, dev)
    with torch.no_grad():
        assert encoder_hip.supported(netg.encoder, torch.zeros(1, 6, 512, device=dev))
        pred, face, spk = netg(gd['au'].to(dev), gd['g_emb'].to(dev), gd['fid'].repeat(6, 1).to(dev), None,
                               torch.zeros(6, 128, device=dev))
    assert linf(pred, gd['g_out']) < 2e-5 * float(gd['g_out'].abs().max()) + 1e-6


@pytest.mark.parametrize('post', ['host', 'device'])
def test_clip_loop_on_the_encoder_kernels_matches_reference_methods(dev, golden, hip_encoder, post):
    """predict_landmarks_speaker_aware over the golden's 600 windows (segments of 512 and 88) to 1e-4 of the landmark range, with
    both post-processing backends."""
    gd = golden('module1.npz')
    netc, netg = _nets(gd, dev)
    gp = torch.Generator().manual_seed(int(gd['p_seed']))
    au = torch.randn(int(gd['p_T']), 18, 80, generator=gp)
    spk = torch.randn(256, generator=gp)
    prev = hip_encoder.set_post_backend(post)
    try:
        fl = hip_encoder.predict_landmarks_speaker_aware(netg, netc, au, spk, gd['fid'].view(-1))
    finally:
        hip_encoder.set_post_backend(prev)
    if post == 'device':
        assert torch.is_tensor(fl) and fl.is_cuda
        fl = fl.cpu().numpy()
    ref = gd['p_sub'].numpy()
    assert fl.shape == (600, 204) and np.abs(fl[::16] - ref).max() < 1e-4 * np.abs(ref).max()


def test_end2end_cli_with_the_encoder_on_the_kernels(dev, golden, tmp_path, monkeypatch):
    """``end2end --wav ... --module1_encoder hip`` (the set-up of test_end2end_cli_from_wav, its checks on the frames) next to the
    same run with the library backend.  The two landmark sequences differ by fp32 rounding (some 1e-6 of a range of a few hundred
    pixels), so a frame's value moves by a small fraction of a grey level and its 8-bit rounding can flip where it lies on a
    boundary: no pixel differs by more than one grey level, and fewer than one in a hundred do (mean |diff| <= 0.01)."""
    from PIL import Image
    from animateportrait_amd import autovc, end2end, module1 as m1
    from animateportrait_amd.synthetic import make_landmarks
    from oracle import generator as og, static_generator as osg
    gd = golden('module1.npz')
    netc, netg = _nets(gd, torch.device('cpu'))
    monkeypatch.chdir(tmp_path)
    os.makedirs('checkpoints/e2e'); os.makedirs('checkpoints/static'); os.makedirs('m1')
    torch.save({'G': netg.state_dict()}, 'm1/g.pth')
    torch.save({'model_g_face_id': netc.state_dict()}, 'm1/c.pth')
    torch.save(og.init_params(og.generator_param_shapes(3, 1, 8, 9, 3, 3), seed=1234), 'checkpoints/e2e/7_net_G_A.pth')
    torch.save(og.init_params(osg.static_param_shapes(3, 1, 64), seed=4321), 'checkpoints/static/drawing.pth')
    yy, xx = np.meshgrid(np.linspace(-1, 1, 256), np.linspace(-1, 1, 256), indexing='ij')
    Image.fromarray(((np.stack([np.sin(3 * xx + yy), np.cos(2 * yy - xx), xx * yy], -1) + 1) * 127.5).astype(np.uint8)).save('photo.png')
    Image.fromarray(((((yy / 0.8) ** 2 + (xx / 0.6) ** 2) < 1) * 255).astype(np.uint8)).save('matte.png')
    lm0 = make_landmarks(1, torch.Generator().manual_seed(9))[0].numpy()
    lm0[0, 0], lm0[16, 0] = 190.0, 70.0
    np.savetxt('photo_lm.txt', np.concatenate([lm0, np.zeros((68, 1))], 1))
    np.savetxt('spk.txt', np.abs(np.random.RandomState(3).randn(256)) * 0.1)
    np.savetxt('trg.txt', np.abs(np.random.RandomState(4).randn(256)) * 0.1)
    torch.manual_seed(5)
    torch.save({'model': autovc.Generator(16, 256, 512, 16).state_dict()}, 'm1/autovc.pth')
    base = ['--photo', 'photo.png', '--matte', 'matte.png', '--wav', os.path.join(GOLDEN, 'female12.wav'), '--photo_landmarks',
            'photo_lm.txt', '--load_a2l_G_name', 'm1/g.pth', '--load_a2l_C_name', 'm1/c.pth', '--max_frames', '64', '--batch', '8',
            '--name', 'e2e', '--epoch', '7', '--ngf', '8', '--checkpoints_dir', 'checkpoints', '--speaker_emb', 'spk.txt',
            '--load_AUTOVC_name', 'm1/autovc.pth', '--autovc_target_emb', 'trg.txt']
    frames = {}
    before = m1.get_encoder_backend()
    try:
        for name in ('library', 'hip'):
            np.random.seed(0)                                    # the blinks come from numpy's global generator
            assert end2end.main(base + ['--out', name, '--module1_encoder', name]) == 0
            assert m1.get_encoder_backend() == name
            files = sorted(os.listdir(os.path.join(name, 'frames')))
            assert files == ['%05d.png' % k for k in range(64)]
            frames[name] = np.stack([np.asarray(Image.open(os.path.join(name, 'frames', f))) for f in files]).astype(np.float64)
            assert frames[name].shape == (64, 256, 256, 3) and frames[name].std() > 1.0
    finally:
        m1.set_encoder_backend(before)
    diff = np.abs(frames['hip'] - frames['library'])
    print('end2end, encoder hip vs library: max |diff| %.0f, mean |diff| %.3e grey levels' % (diff.max(), diff.mean()))
    assert diff.max() <= 1 and diff.mean() <= 1e-2
