"""GPU (-m gpu): the clip's speaker embedding on the device (speaker.py over apq_mel_frames / apq_speaker_head of libapseq.so,
csrc/seq/seq_speaker.hip) against its float64 restatement (tests/speaker_reference.py): the mel frames at the contract's sizes
with guarded buffers, the head with zero rows, the whole utterance with both LSTM backends, the segments, and end2end
--speaker_emb_from wav.

Bars (derived, not measured; every case prints what it measured):
  * mel: the value is carried in fp64 and rounded once, so an element is within 4 fp32 ulps of the reference plus 1e-10 of its
    frame's largest element.
  * head: a pre-activation is 64 fused multiply-adds, two additions and the bias in fp32: at most 67 roundings of 2^-24 relative
    to sum |w_i h_i| + |b| (the standard bound of a recursive sum), delta_j.  ReLU does not enlarge it.  The quotient q = v / |v|
    moves by at most delta_j / |v| + |q_j| |delta| / |v| to first order, plus its own rounding 2^-24 |q_j|; the embedding likewise
    from the mean of the rows' bounds.  1 % is added for the second order.
  * utterance: 4 times the L-inf error that the plain fp32 PyTorch statement of the same network, fed the same device mel, shows
    against float64 in the same run (the embedding has unit norm).

Measured on an MI355X: mel 0.50 fp32 ulp at every size (0.125 of the bar), first and last frames alike; head at most 1.2e-7 on a
row (bar 7.7e-6) and 4.4e-8 on the embedding (bar 9.6e-6); embed_utterance 2 s: 1.8e-8 (library LSTM) and 3.1e-8 (kernel), plain
statement 4.7e-8, bar 1.9e-7; the whole clip: 9.3e-9 and 1.5e-8, plain 1.7e-8, bar 6.8e-8; five segments 8.8e-9, bar 1.4e-7."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import speaker_reference as R

pytestmark = pytest.mark.gpu

SENTINEL = 777.0
U = 2.0 ** -24
SEED = 11


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


# ------------------------------------------------------------------------------------------------------------------ mel frames
MEL_CASES = [(400, 160, 40, 2, 201), (400, 160, 40, 2, 1600), (400, 160, 40, 2, 25637), (1024, 256, 80, 1, 513), (1024, 256, 80, 1, 4099),
             (64, 16, 8, 2, 33), (16, 16, 1, 1, 9)]


def _mel_inputs(n_fft, n_mels, L, seed):
    from animateportrait_amd import audio
    rs = np.random.RandomState(seed)
    x = (0.1 * rs.randn(L) + 0.3 * np.sin(2 * np.pi * 440.0 / 16000.0 * np.arange(L))).astype(np.float32)
    if n_fft >= 400:
        basis = audio.mel_filterbank(16000, n_fft, n_mels, 0.0, 8000.0)
    else:
        basis = rs.rand(n_mels, n_fft // 2 + 1).astype(np.float32)       # (a Slaney bank this coarse has empty rows)
    return x, R.hann_periodic(n_fft), np.ascontiguousarray(basis)


def _mel_bar(ref):
    return 4.0 * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64) + 1e-10 * np.abs(ref).max(axis=1, keepdims=True)


@pytest.mark.parametrize('n_fft,hop,n_mels,power,L', MEL_CASES)
def test_mel_frames_match_float64_with_guarded_buffers(dev, n_fft, hop, n_mels, power, L):
    from animateportrait_amd import speaker
    x, window, basis = _mel_inputs(n_fft, n_mels, L, L)
    ref = R.mel_frames(x, window, basis, hop, power)
    T = L // hop + 1
    assert ref.shape == (T, n_mels)
    # the signal sits between NaN: a read before sample 0 or past L would poison its frame
    pad = 512
    xb = torch.full((L + 2 * pad,), float('nan'), device=dev)
    xb[pad:pad + L] = torch.from_numpy(x).to(dev)
    ob = torch.full((T * n_mels + 2 * pad,), SENTINEL, device=dev)
    out = ob[pad:pad + T * n_mels].view(T, n_mels)
    got = speaker.mel_frames(xb[pad:pad + L], torch.from_numpy(window).to(dev), torch.from_numpy(basis).to(dev), hop, power, out=out)
    assert got is out
    ob_h = ob.cpu().numpy()
    assert (ob_h[:pad] == SENTINEL).all() and (ob_h[pad + T * n_mels:] == SENTINEL).all()
    g = ob_h[pad:pad + T * n_mels].reshape(T, n_mels).astype(np.float64)
    assert np.isfinite(g).all()
    excess = np.abs(g - ref) / _mel_bar(ref)
    ulps = np.abs(g - ref) / np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    print('mel %d/%d/%d power %d L %d: T %d, worst error %.3f of the bar (%.2f ulp; first frame %.3f, last frame %.3f of the bar)'
          % (n_fft, hop, n_mels, power, L, T, excess.max(), ulps[np.unravel_index(excess.argmax(), excess.shape)], excess[0].max(), excess[-1].max()))
    assert excess[0].max() <= 1.0, 'the first frame (reflected samples)'
    assert excess[-1].max() <= 1.0, 'the last frame (reflected samples)'
    assert excess.max() <= 1.0


def test_mel_power_is_the_encoders_front_end(dev):
    from animateportrait_amd import speaker
    x, _, _ = _mel_inputs(400, 40, 25600, 5)
    got = speaker.mel_power(x, dev).cpu().numpy().astype(np.float64)
    ref = R.mel_power(x)
    assert got.shape == ref.shape == (161, 40) and (np.abs(got - ref) <= _mel_bar(ref)).all()
    with pytest.raises(RuntimeError, match='L = 200'):
        speaker.mel_power(x[:200], dev)


# ------------------------------------------------------------------------------------------------------------------------ head
def _head_bars(h, w, b):
    """-> (bar of partial (B, 256), bar of embed (256,)): the module docstring's first-order bounds in float64"""
    h, w, b = (a.astype(np.float64) for a in (h, w, b))
    delta = 67 * U * (np.abs(h) @ np.abs(w).T + np.abs(b))                                   # (B, 256)
    v = np.maximum(h @ w.T + b, 0.0)
    norm = np.sqrt((v * v).sum(axis=1, keepdims=True))
    live = norm[:, 0] > 0
    q = np.divide(v, norm, out=np.zeros_like(v), where=norm > 0)
    dq = np.zeros_like(v)
    dq[live] = (delta[live] + q[live] * np.sqrt((delta[live] ** 2).sum(axis=1, keepdims=True))) / norm[live] + U * q[live]
    mean, dm = q.mean(axis=0), dq.mean(axis=0)
    n = np.sqrt((mean * mean).sum())
    de = (dm + (mean / n) * np.sqrt((dm ** 2).sum())) / n + U * mean / n if n > 0 else np.zeros_like(mean)
    return 1.01 * dq, 1.01 * de


@pytest.mark.parametrize('B,zero', [(1, None), (2, None), (17, 'row'), (17, 'all'), (4096, None)])
def test_speaker_head_matches_float64_with_guarded_buffers(dev, B, zero):
    from animateportrait_amd import speaker
    rs = np.random.RandomState(B)
    h = rs.uniform(-1, 1, (B, 256)).astype(np.float32)
    w = rs.uniform(-1 / 16, 1 / 16, (256, 256)).astype(np.float32)
    b = rs.uniform(-1 / 16, 1 / 16, 256).astype(np.float32)
    if zero is not None:
        b = -np.abs(b)                       # relu(w 0 + b) = 0: a row of zeros in h is a row of zeros behind the ReLU
        h[5 if zero == 'row' else slice(None)] = 0
    ref_e, ref_p = R.head(h, w, b)
    pad = 256
    pb = torch.full((B * 256 + 2 * pad,), SENTINEL, device=dev)
    eb = torch.full((256 + 2 * pad,), SENTINEL, device=dev)
    hb = torch.full((B * 256 + 2 * pad,), float('nan'), device=dev)
    hb[pad:pad + B * 256] = torch.from_numpy(h).to(dev).view(-1)
    out = (eb[pad:pad + 256], pb[pad:pad + B * 256].view(B, 256))
    speaker.head(hb[pad:pad + B * 256].view(B, 256), torch.from_numpy(w).to(dev), torch.from_numpy(b).to(dev), out=out)
    pb_h, eb_h = pb.cpu().numpy(), eb.cpu().numpy()
    for buf, n in ((pb_h, B * 256), (eb_h, 256)):
        assert (buf[:pad] == SENTINEL).all() and (buf[pad + n:] == SENTINEL).all()
    got_p, got_e = pb_h[pad:pad + B * 256].reshape(B, 256).astype(np.float64), eb_h[pad:pad + 256].astype(np.float64)
    bar_p, bar_e = _head_bars(h, w, b)
    err_p, err_e = np.abs(got_p - ref_p), np.abs(got_e - ref_e)
    print('head B %d %s: partial worst error %.3e (its bar %.3e), embed worst error %.3e (its bar %.3e)'
          % (B, zero or '', err_p.max(), bar_p.flat[err_p.argmax()], err_e.max(), bar_e[err_e.argmax()]))
    assert np.isfinite(got_p).all() and np.isfinite(got_e).all()
    assert (err_p <= bar_p).all() and (err_e <= bar_e).all()
    if zero == 'row':
        assert (got_p[5] == 0).all() and (ref_p[5] == 0).all() and abs(np.linalg.norm(got_e) - 1) < 1e-6
    elif zero == 'all':
        assert (got_p == 0).all() and (got_e == 0).all()
    else:
        assert np.abs(np.linalg.norm(got_p, axis=1) - 1).max() < 1e-6 and abs(np.linalg.norm(got_e) - 1) < 1e-6


# ------------------------------------------------------------------------------------------------------------------- utterance
def _encoder(dev, backend):
    from animateportrait_amd import speaker
    enc = speaker.VoiceEncoder(backend)
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in R.seeded_weights(SEED).items()}, strict=True)
    return enc.to(dev).eval()


def plain_fp32_embedding(enc, wav):
    """The same network as plain fp32 PyTorch statements on the device, fed the device's mel -> (256,) float64"""
    from animateportrait_amd import speaker
    padded, starts = R.padded(wav)
    with torch.no_grad():
        mel = speaker.mel_power(padded, enc.linear.weight.device)
        mels = torch.stack([mel[a:a + R.PARTIAL] for a in starts])
        hidden = enc.lstm(mels)[1][0]
        raw = torch.relu(enc.linear(hidden[-1]))
        partial = raw / torch.norm(raw, dim=1, keepdim=True)
        mean = partial.mean(dim=0)
        return (mean / torch.norm(mean, 2)).cpu().numpy().astype(np.float64)


@pytest.fixture(scope='module')
def clip():
    """the fixture as the encoder sees it, and the float64 embeddings of its first 2 s and of the whole; never written to"""
    from animateportrait_amd import audio
    x, sr = audio.read_wav(os.path.join(GOLDEN, 'female12.wav'))
    wav = R.preprocess_wav(x, sr)
    sd = R.seeded_weights(SEED)
    return {'x': x, 'sr': sr, 'wav': wav, 'sd': sd, '2s': R.embed_utterance(wav[:32000], sd), 'whole': R.embed_utterance(wav, sd)}


@pytest.mark.parametrize('backend', ['library', 'hip'])
@pytest.mark.parametrize('length', ['2s', 'whole'])
def test_embed_utterance_matches_float64(dev, clip, length, backend):
    wav = clip['wav'][:32000] if length == '2s' else clip['wav']
    ref_e, ref_p = clip[length]
    enc = _encoder(dev, backend)
    embed, partials = enc.embed_utterance(wav)
    assert embed.is_cuda and tuple(embed.shape) == (256,) and tuple(partials.shape) == ref_p.shape == ({'2s': 2, 'whole': 24}[length], 256)
    got_e, got_p = embed.cpu().numpy().astype(np.float64), partials.cpu().numpy().astype(np.float64)
    plain = float(np.abs(plain_fp32_embedding(enc, wav) - ref_e).max())
    err = float(np.abs(got_e - ref_e).max())
    print('embed_utterance %s, %s LSTM: L-inf %.3e against float64; the plain fp32 statement %.3e; bar %.3e; partials L-inf %.3e'
          % (length, backend, err, plain, 4 * plain, np.abs(got_p - ref_p).max()))
    assert abs(np.linalg.norm(got_e) - 1) < 1e-6 and abs(np.linalg.norm(ref_e) - 1) < 1e-12
    assert plain > 0
    assert err <= 4 * plain


def test_speaker_embedding_of_five_segments(dev, clip):
    from animateportrait_amd import speaker
    enc = _encoder(dev, 'library')
    got = speaker.speaker_embedding(clip['x'], clip['sr'], enc, segment_len=40000)
    assert got.shape == (256,) and got.dtype == np.float32
    wav = clip['wav']
    assert wav.shape[0] // 40000 == 5
    ref = R.speaker_embedding(clip['x'], clip['sr'], clip['sd'], segment_len=40000)
    plain = np.mean([plain_fp32_embedding(enc, wav[40000 * i:40000 * (i + 1)]) for i in range(5)], axis=0)
    err, perr = float(np.abs(got - ref).max()), float(np.abs(plain - ref).max())
    print('speaker_embedding, 5 segments: L-inf %.3e against float64; the plain fp32 statement %.3e; bar %.3e; norm %.4f'
          % (err, perr, 4 * perr + U, np.linalg.norm(got)))
    assert err <= 4 * perr + U                      # (+ the result's own rounding to float32)
    assert np.linalg.norm(ref) < 1.0                # a mean of unit vectors, not renormalised


# ----------------------------------------------------------------------------------------------------------------- integration
def test_end2end_with_the_embedding_from_the_wav(dev, golden, tmp_path, monkeypatch, capsys):
    """``end2end --wav ... --speaker_emb_from wav --speaker_encoder CKPT`` with stand-in checkpoints (the set-up of
    test_end2end_cli_with_f0_on_device) against a second run with ``--speaker_emb`` pointing at the txt the speaker CLI wrote: the
    same embedding bit for bit in both conditioned stages, hence the same frames."""
    from PIL import Image
    from animateportrait_amd import autovc, end2end, module1 as m1, speaker
    from animateportrait_amd.synthetic import make_landmarks
    from oracle import generator as og, static_generator as osg
    from test_module1_gpu import _nets
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
    np.savetxt('trg.txt', np.abs(np.random.RandomState(4).randn(256)) * 0.1)
    torch.manual_seed(5)
    torch.save({'model': autovc.Generator(16, 256, 512, 16).state_dict()}, 'm1/autovc.pth')
    sd = {k: torch.from_numpy(v) for k, v in R.seeded_weights(SEED).items()}
    torch.save({'model_state': dict(sd, similarity_weight=torch.tensor([10.0]), similarity_bias=torch.tensor([-5.0]))}, 'm1/encoder.pt')
    wav = os.path.join(GOLDEN, 'female12.wav')
    assert speaker.main(['--wav', wav, '--encoder', 'm1/encoder.pt', '--out', 'spk.txt']) == 0
    written = np.loadtxt('spk.txt').astype(np.float32)
    assert written.shape == (256,) and abs(np.linalg.norm(written) - 1) < 1e-6
    base = ['--photo', 'photo.png', '--matte', 'matte.png', '--wav', wav, '--photo_landmarks', 'photo_lm.txt', '--load_a2l_G_name',
            'm1/g.pth', '--load_a2l_C_name', 'm1/c.pth', '--max_frames', '48', '--batch', '8', '--name', 'e2e', '--epoch', '7',
            '--ngf', '8', '--checkpoints_dir', 'checkpoints', '--load_AUTOVC_name', 'm1/autovc.pth', '--autovc_target_emb', 'trg.txt']
    seen = {'convert': [], 'module1': [], 'windows': []}
    real_predict, real_convert = m1.predict_landmarks_speaker_aware, autovc.convert_mel

    def spy_predict(net_g, net_c, windows, spk_emb, *args, **kw):
        seen['module1'].append(np.array(spk_emb, dtype=np.float32))
        seen['windows'].append(np.array(windows, dtype=np.float32))
        return real_predict(net_g, net_c, windows, spk_emb, *args, **kw)

    def spy_convert(G, mel, f0, emb, *args, **kw):
        seen['convert'].append(np.array(emb, dtype=np.float32))
        return real_convert(G, mel, f0, emb, *args, **kw)
    monkeypatch.setattr(m1, 'predict_landmarks_speaker_aware', spy_predict)
    monkeypatch.setattr(autovc, 'convert_mel', spy_convert)
    # the converter's library convolutions are not bit-reproducible from run to run by default (test_f0_gpu.py meets the same):
    # both runs ask the library for its deterministic algorithms, so that equal inputs give equal frames
    monkeypatch.setattr(torch.backends.cudnn, 'deterministic', True)
    monkeypatch.setattr(torch.backends.cudnn, 'benchmark', False)
    np.random.seed(0)
    assert end2end.main(base + ['--out', 'from_wav', '--speaker_emb_from', 'wav', '--speaker_encoder', 'm1/encoder.pt']) == 0
    np.random.seed(0)
    assert end2end.main(base + ['--out', 'from_txt', '--speaker_emb', 'spk.txt']) == 0
    capsys.readouterr()
    assert len(seen['convert']) == len(seen['module1']) == 2
    for stage in ('convert', 'module1'):
        assert seen[stage][0].shape == (256,) and np.array_equal(seen[stage][0], written) and np.array_equal(seen[stage][1], written), stage
    names = ['%05d.png' % k for k in range(48)]
    assert sorted(os.listdir('from_wav/frames')) == sorted(os.listdir('from_txt/frames')) == names
    a = np.stack([np.asarray(Image.open(os.path.join('from_wav/frames', n))) for n in names]).astype(np.int64)
    b = np.stack([np.asarray(Image.open(os.path.join('from_txt/frames', n))) for n in names]).astype(np.int64)
    wa, wb = seen['windows']
    print('end2end --speaker_emb_from wav against --speaker_emb txt: Module1 windows differ by up to %.3e in %d of %d values, frames by up '
          'to %d levels in %d of %d pixels' % (np.abs(wa - wb).max(), int((wa != wb).sum()), wa.size, np.abs(a - b).max(), int((a != b).sum()), a.size))
    assert np.array_equal(a, b)
