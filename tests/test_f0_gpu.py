"""GPU (-m gpu): the f0 track on the device (f0.py over apq_f0_candidates / apq_f0_track of libapseq.so, csrc/seq/seq_f0.hip)
against its float64 restatement (tests/f0_reference.py) -- the candidate tables, the dynamic programme on given tables, the whole
track of the example clip, the contract's edges with sentinel-padded outputs, and end2end --f0 device.

Bars (set by the restatement's contract, not by what the kernels give): NCCF values 1e-4, lags 1e-3 samples, rr and S 1e-4
relative, normalised f0 1e-5; a candidate within 1e-3 of a threshold or of a neighbouring value is left out of the set
comparison, a frame whose float64 decision margin is below 1e-4 out of the path comparison.  Every case prints what it measured."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import f0_reference as R

pytestmark = pytest.mark.gpu

SENTINEL = 777.0
EPS_C = 1e-3          # exclusion zone of a candidate's conditions
EPS_M = 1e-4          # exclusion zone of a decision margin


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


SIGNALS = {
    'tone220': (lambda: R.harmonic_signal(220.0, 1), 'F'), 'tone311': (lambda: R.harmonic_signal(311.3, 1), 'F'),
    'tone440': (lambda: R.harmonic_signal(440.0, 1), 'F'), 'tone590': (lambda: R.harmonic_signal(590.0, 1), 'F'),
    'tone110M': (lambda: R.harmonic_signal(110.0, 1), 'M'),
    'glide': (lambda: R.harmonic_signal(np.linspace(120.0, 300.0, 16000), 2), 'F'),
    'gap': (lambda: R.harmonic_signal(200.0, 3, gap=(6400, 9600)), 'F'),
    'silence': (lambda: np.zeros(16000, np.float32), 'F'),
    'noise': (lambda: R.harmonic_signal(0.0, 5, amp=0.0), 'F'),
}


def _clip_input():
    from animateportrait_amd import audio
    x, sr = audio.read_wav(os.path.join(GOLDEN, 'female12.wav'))
    return audio.normalize_loudness(audio.resample_to_16k(x, sr))


@pytest.fixture(scope='module')
def refs():
    """signal name -> (tracker input, gender, the restatement's result); computed once, never written to"""
    cache = {}

    def get(name):
        if name not in cache:
            if name == 'clip':
                from animateportrait_amd import f0
                x, gender = f0.tracker_input(_clip_input()), 'F'
            else:
                make, gender = SIGNALS[name]
                x = make()
            cache[name] = (x, gender, R.f0_track(x, gender))
        return cache[name]
    return get


def _np(tab):
    return {k: v.cpu().numpy() for k, v in tab.items()}


def _compare_tables(got, ref, what):
    """Asserts the tables outside the exclusion zones.  -> (unsure, differs) per frame: a candidate of the restatement lies inside
    a zone (R.candidate_slack), and the device's row is not the restatement's -- which only an unsure frame may be."""
    kmin, kmax = ref['kmin'], ref['kmax']
    T = len(ref['count'])
    assert got['count'].shape == (T,) and got['lag'].shape == (T, R.N_CANDS)
    worst_lag = worst_val = 0.0
    unsure, differs = np.zeros(T, bool), np.zeros(T, bool)
    for t in range(T):
        k, lag, val, sure = R.candidate_slack(ref['phi'][t], kmin, kmax, EPS_C)
        n = int(got['count'][t])
        assert 0 <= n <= R.N_CANDS and (got['lag'][t, n:] == 0).all() and (got['val'][t, n:] == 0).all()
        glag, gval = got['lag'][t, :n].astype(np.float64), got['val'][t, :n].astype(np.float64)
        assert (np.diff(glag) > 0).all()
        if len(val) > R.N_CANDS:                                     # the cut at 19: sure only above the 20th value by the zone
            sure = sure & (val > np.sort(val)[::-1][R.N_CANDS] + EPS_C)
        unsure[t] = not sure.all()
        for l, v in zip(lag[sure], val[sure]):                       # every sure candidate is there ...
            j = int(np.abs(glag - l).argmin()) if n else -1
            assert j >= 0 and abs(glag[j] - l) <= 1e-3 and abs(gval[j] - v) <= 1e-4, (what, t, l, v)
            worst_lag, worst_val = max(worst_lag, abs(glag[j] - l)), max(worst_val, abs(gval[j] - v))
        for l in glag:                                               # ... and nothing that is not the peak of a near-candidate lag
            assert len(k) and np.abs(k - l).min() <= 0.5 + 1e-3, (what, t, l)
        rn = int(ref['count'][t])
        differs[t] = n != rn or np.abs(glag - ref['lag'][t, :n]).max(initial=0) > 1e-3 or np.abs(gval - ref['val'][t, :n]).max(initial=0) > 1e-4
        assert unsure[t] or not differs[t], (what, t)
    rr_err = float(np.abs(got['rr'] / ref['rr'] - 1).max())
    s_err = float(np.abs(got['s'] / ref['s'] - 1).max())
    print('%s: T %d, lag err %.2e (bar 1e-3), value err %.2e (bar 1e-4), rr rel %.2e, S rel %.2e (bar 1e-4); frames with a candidate '
          'in a zone %d, of which the device row differs in %d' % (what, T, worst_lag, worst_val, rr_err, s_err, int(unsure.sum()), int(differs.sum())))
    assert rr_err <= 1e-4 and s_err <= 1e-4
    return unsure, differs


# ------------------------------------------------------------------------------------------------------- stage 1: candidates
@pytest.mark.parametrize('name', list(SIGNALS) + ['clip'])
def test_candidates_match_restatement(dev, refs, name):
    from animateportrait_amd import f0
    x, gender, ref = refs(name)
    got = _np(f0.candidates(x, gender, dev))
    _compare_tables(got, ref, name)
    if name == 'silence':
        assert (got['count'] == 0).all() and (got['rr'] == 1).all() and np.abs(got['s'] - 1).max() <= 1e-6


# ------------------------------------------------------------------------------------------------------------ stage 2: track
def _tables32(ref, dev):
    """the restatement's tables rounded to fp32: what the device is given, and the same numbers in float64 for the host"""
    t32 = {'count': ref['count'].astype(np.int32)}
    for k in ('lag', 'val', 'rr', 's'):
        t32[k] = ref[k].astype(np.float32)
    return t32, {k: torch.from_numpy(v).to(dev) for k, v in t32.items()}


def _host_track(t32, kmax):
    tab = {k: (v.astype(np.float64) if v.dtype == np.float32 else v) for k, v in t32.items()}
    path, margin = R.viterbi(tab, kmax)
    return path, margin, R.speaker_normalization(R.log_f0(tab, path))


def _compare_track(out, path, margin, f0n, what, cap):
    gpath = out['path'].astype(np.int64)
    gpath[gpath == 255] = -1
    firm = margin > EPS_M
    share = 1.0 - firm.mean()
    assert share <= cap, '%s: %.3f of the frames below the margin (cap %.2f)' % (what, share, cap)
    assert np.array_equal(gpath[firm], path[firm]), (what, np.nonzero(gpath != path)[0])
    gf0 = out['f0'].astype(np.float64)
    assert np.array_equal(gf0[firm] < 0, f0n[firm] < 0) and (gf0[gf0 < 0] == np.float32(-1e10)).all()
    v = firm & (f0n >= 0)
    err = float(np.abs(gf0[v] - f0n[v]).max(initial=0))
    print('%s: frames below the margin %.4f (cap %.2f), smallest margin %.3e, voiced %d of %d, f0_norm err %.2e (bar 1e-5)'
          % (what, share, cap, float(margin.min()), int((path >= 0).sum()), len(path), err))
    assert err <= 1e-5
    assert ((gf0[gf0 >= 0] >= 0) & (gf0[gf0 >= 0] <= 1)).all()
    return firm


@pytest.mark.parametrize('name', list(SIGNALS) + ['clip'])
def test_track_matches_float64_dp_on_the_same_tables(dev, refs, name):
    from animateportrait_amd import f0
    _, gender, ref = refs(name)
    t32, tdev = _tables32(ref, dev)
    path, margin, f0n = _host_track(t32, ref['kmax'])
    out = _np(f0.track(tdev, gender))
    _compare_track(out, path, margin, f0n, name, 0.01)
    # the back-pointers of the chosen states lead along the path
    state = np.where(out['path'] == 255, t32['count'], out['path']).astype(np.int64)
    assert np.array_equal(out['back'][np.arange(1, len(state)), state[1:]], state[:-1])


# ------------------------------------------------------------------------------------------------------ end to end on the clip
def test_clip_track_matches_restatement_and_is_plausible(dev, refs):
    """female12.wav, 818 frames: the one-hot rows the converter is fed are the restatement's on every frame that neither
    exclusion touches, at most 2 % of the frames.  A frame counts as touched by the candidate exclusion when its table row on the
    device differs from the restatement's (which _compare_tables allows through candidates inside a zone only), and by the path
    exclusion when its float64 margin is at most 1e-4; the latter share is the restatement's alone (1 of 818) and is checked on
    the CPU.  Counting every frame with ANY candidate inside a zone would exclude 27 % of this clip -- its noise frames have
    dozens of weak peaks around the 0.3 max threshold and the cut at 19 -- so that reading cannot meet the cap and is printed only."""
    from animateportrait_amd import autovc, f0
    x, gender, ref = refs('clip')
    assert len(ref['path']) == 818
    got = f0.f0_track(_clip_input(), gender, dev)
    assert got.shape == (818,) and got.dtype == np.float64 and (got[got < 0] == -1e10).all()
    tab = f0.candidates(x, gender, dev)
    out = _np(f0.track(tab, gender))
    unsure, differs = _compare_tables(_np(tab), ref, 'clip')
    weak = ref['margin'] <= EPS_M
    excluded = differs | weak
    share = float(excluded.mean())
    print('clip: excluded frames %.4f (cap 0.02): %d whose table row differs through a candidate in a zone, %d below the margin (the '
          'restatement alone: %.4f); frames with any candidate in a zone: %.3f' % (share, int(differs.sum()), int(weak.sum()), weak.mean(), unsure.mean()))
    assert weak.mean() <= 0.02
    assert share <= 0.02
    rows, want = autovc.quantize_f0_interp(got), autovc.quantize_f0_interp(ref['f0_norm'])
    bad = np.nonzero((rows != want).any(1) & ~excluded)[0]
    assert bad.size == 0, bad
    voiced = out['path'] != 255
    hz = 16000.0 / np.asarray(_np(tab)['lag'])[np.nonzero(voiced)[0], out['path'][voiced]]
    print('clip: voiced share %.3f (0.3 .. 0.9), median %.1f Hz (100 .. 600)' % (voiced.mean(), np.median(hz)))
    assert 0.3 <= voiced.mean() <= 0.9 and 100.0 <= np.median(hz) <= 600.0


# ---------------------------------------------------------------------------------------------------------- contract edges
def _padded(T, dev):
    """every output of both calls as a view into a sentinel-filled buffer with room behind it"""
    pad = 64

    def buf(n, dtype, fill):
        b = torch.full((n + pad,), fill, dtype=dtype, device=dev)
        return b, b[:n]
    raw, tab, out = {}, {}, {}
    for k, n, dt, fill in (('count', T, torch.int32, 777), ('lag', T * 19, torch.float32, SENTINEL), ('val', T * 19, torch.float32, SENTINEL),
                           ('rr', T, torch.float32, SENTINEL), ('s', T, torch.float32, SENTINEL)):
        raw[k], v = buf(n, dt, fill)
        tab[k] = v.view(T, 19) if k in ('lag', 'val') else v
    for k, n, dt, fill in (('f0', T, torch.float32, SENTINEL), ('path', T, torch.uint8, 0xAB), ('back', T * 20, torch.uint8, 0xAB)):
        raw[k], v = buf(n, dt, fill)
        out[k] = v.view(T, 20) if k == 'back' else v
    return raw, tab, out


def _pads_untouched(raw, T):
    for k, b in raw.items():
        n = T * {'lag': 19, 'val': 19, 'back': 20}.get(k, 1)
        fill = 0xAB if b.dtype == torch.uint8 else 777
        assert bool((b[n:] == fill).all()), k


EDGES = {
    'L1': (lambda: np.full(1, 3000.0, np.float32), 'F', None),
    'L255': (lambda: R.harmonic_signal(200.0, 7, n=255), 'F', None),
    'L257': (lambda: R.harmonic_signal(200.0, 8, n=257), 'F', None),
    'short_of_the_span': (lambda: R.harmonic_signal(300.0, 9, n=100), 'F', None),             # 100 < 120 + 160 + 2
    'M_kmax320': (lambda: R.harmonic_signal(70.0, 10, n=2000), 'M', None),
    'frames_past_the_signal': (lambda: R.harmonic_signal(250.0, 11, n=300), 'F', 6),          # frames 3 .. 5 read no sample
}


@pytest.mark.parametrize('name', list(EDGES))
def test_contract_edges_with_guarded_outputs(dev, name):
    from animateportrait_amd import f0
    make, gender, frames = EDGES[name]
    x = make()
    T = R.frame_count(len(x)) if frames is None else frames
    assert T == {'L1': 1, 'L255': 1, 'L257': 2, 'short_of_the_span': 1, 'M_kmax320': 8, 'frames_past_the_signal': 6}[name]
    ref = R.candidate_tables(x, gender, T)
    # the input sits at the end of its buffer's used part with NaN behind it: a read past L would poison the frame
    xb = torch.full((len(x) + 512,), float('nan'), device=dev)
    xb[:len(x)] = torch.from_numpy(x).to(dev)
    raw, tab, out = _padded(T, dev)
    assert f0.candidates(xb[:len(x)], gender, frames=T, out=tab) is tab
    got = _np(tab)
    assert all(np.isfinite(got[k]).all() for k in ('lag', 'val', 'rr', 's'))
    _compare_tables(got, ref, name)
    if name == 'frames_past_the_signal':
        assert (got['count'][3:] == 0).all() and (got['rr'][4:] == 1).all()
    f0.track(tab, gender, out=out)
    _pads_untouched(raw, T)
    t32 = {k: got[k] for k in ('count', 'lag', 'val', 'rr', 's')}
    path, margin, f0n = _host_track(t32, ref['kmax'])
    _compare_track(_np(out), path, margin, f0n, name, 1.0)


def test_exactly_one_voiced_frame_gets_a_half(dev):
    """Hand-made tables whose best path is voiced in frame 2 alone: zero deviation, so that frame's f0_norm is 0.5."""
    from animateportrait_amd import f0
    T = 5
    t32 = {'count': np.array([0, 0, 1, 0, 0], np.int32), 'lag': np.zeros((T, 19), np.float32), 'val': np.zeros((T, 19), np.float32),
           'rr': np.array([1, 1, 10, 0.1, 1], np.float32), 's': np.full(T, 0.01, np.float32)}
    t32['lag'][2, 0], t32['val'][2, 0] = 50.25, 0.9
    path, margin, f0n = _host_track(t32, 160)
    assert path.tolist() == [-1, -1, 0, -1, -1] and margin.min() > 0.1 and f0n[2] == 0.5
    raw, _, out = _padded(T, dev)
    f0.track({k: torch.from_numpy(v).to(dev) for k, v in t32.items()}, 'F', out=out)
    got = _np(out)
    assert got['path'].tolist() == [255, 255, 0, 255, 255]
    assert got['f0'][2] == 0.5 and (np.delete(got['f0'], 2) == np.float32(-1e10)).all()
    for k in ('f0', 'path', 'back'):
        n = T * (20 if k == 'back' else 1)
        assert bool((raw[k][n:] == (0xAB if k != 'f0' else SENTINEL)).all())


# -------------------------------------------------------------------------------------------------------------- integration
def test_end2end_cli_with_f0_on_device(dev, golden, tmp_path, monkeypatch, capsys):
    """``end2end --wav ... --f0 device`` with stand-in checkpoints (the set-up of test_end2end_cli_with_post_on_device): the
    windows Module1 is fed differ from those of the all-unvoiced track, and without --f0 they are the windows of
    convert_mel with no track (to the converter's run-to-run rounding), with the WARNING as before."""
    from PIL import Image
    from animateportrait_amd import audio, autovc, end2end, module1 as m1
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
    np.savetxt('spk.txt', np.abs(np.random.RandomState(3).randn(256)) * 0.1)
    np.savetxt('trg.txt', np.abs(np.random.RandomState(4).randn(256)) * 0.1)
    torch.manual_seed(5)
    torch.save({'model': autovc.Generator(16, 256, 512, 16).state_dict()}, 'm1/autovc.pth')
    wav = os.path.join(GOLDEN, 'female12.wav')
    base = ['--photo', 'photo.png', '--matte', 'matte.png', '--wav', wav, '--photo_landmarks', 'photo_lm.txt', '--load_a2l_G_name',
            'm1/g.pth', '--load_a2l_C_name', 'm1/c.pth', '--max_frames', '48', '--batch', '8', '--name', 'e2e', '--epoch', '7',
            '--ngf', '8', '--checkpoints_dir', 'checkpoints', '--speaker_emb', 'spk.txt', '--load_AUTOVC_name', 'm1/autovc.pth',
            '--autovc_target_emb', 'trg.txt']
    seen = []
    real = m1.predict_landmarks_speaker_aware

    def spy(net_g, net_c, windows, *args, **kw):
        seen.append(np.array(windows, dtype=np.float32))
        return real(net_g, net_c, windows, *args, **kw)
    monkeypatch.setattr(m1, 'predict_landmarks_speaker_aware', spy)
    np.random.seed(0)
    assert end2end.main(base + ['--out', 'tracked', '--f0', 'device']) == 0
    assert 'WARNING: no --f0_npy' not in capsys.readouterr().out
    assert sorted(os.listdir('tracked/frames')) == ['%05d.png' % k for k in range(48)]
    # without --f0: the stage as it was (the frame loop behind it is not run again)
    a = end2end.make_parser().parse_known_args(base + ['--out', 'plain'])[0]
    assert a.f0 is None
    end2end.landmarks_from_audio(a, dev)
    assert 'WARNING: no --f0_npy' in capsys.readouterr().out
    tracked, plain = seen
    assert tracked.shape == plain.shape == (48, 18, 80) and np.isfinite(tracked).all()
    diff = float(np.abs(tracked - plain).max())
    print('end2end --f0 device: windows differ from the unvoiced-track windows by up to %.3e' % diff)
    assert diff > 1e-4
    G = autovc.load_generator('m1/autovc.pth', dev)
    emb, trg = np.loadtxt('spk.txt').astype(np.float32), autovc.load_target_embedding('trg.txt')
    by_hand = audio.clip_audio_features(wav, max_frames=48, converter=lambda mel: autovc.convert_mel(G, mel, None, emb, trg, dev))
    # (the converter's library convolutions are not bit-reproducible from run to run: a few fp32 ulps of values of order 1)
    same = float(np.abs(plain - by_hand).max())
    print('end2end without --f0: windows vs convert_mel with no track %.3e (bar %.3e)' % (same, 1e-5 * np.abs(by_hand).max()))
    assert same <= 1e-5 * np.abs(by_hand).max() < 1e-2 * diff
