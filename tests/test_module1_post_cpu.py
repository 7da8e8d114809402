"""CPU (-m "not gpu"): the landmark post-processing calls of libapseq.so (apq_savgol, apq_calib_baseline,
apq_segment_assemble, apq_image_landmarks) as far as they go without a device -- their host-only argument checks, the
Savitzky-Golay tap table, the blink stamps factored out of add_naive_eye, and the post-processing backend switch of
module1 / end2end.  Nothing here launches a kernel."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

A = 0x10000          # stand-in addresses, aligned to everything the kernels ask for
B = 0x20000
C = 0x30000
D = 0x40000


def _lib():
    from animateportrait_amd import _seqapi
    return _seqapi.lib()


def _sg(x=A, y=B, taps0=C, taps1=D, T=625, Cc=204, c0=0, c1=144, c2=204, W0=15, W1=5):
    return (x, y, taps0, taps1, T, Cc, c0, c1, c2, W0, W1)


def _calib(x=A, y=B, T=512, k=256, ax=2.0, ay=2.0):
    return (x, y, T, k, ax, ay)


def _seg(inp=A, base=B, fid=C, out=D, T=512, ratio=0.99, amp=0.5, flags=7):
    return (inp, base, fid, out, T, ratio, amp, flags)


def _img(inp=A, out=B, stamps=C, n=5, T=625, scale=0.01, sx=-128.0, sy=-128.0, flags=3):
    return (inp, out, stamps, n, T, scale, sx, sy, flags)


SERVED = [
    ('apq_savgol', _sg()), ('apq_savgol', _sg(T=5, Cc=3, c1=3, c2=3, W0=5, taps1=None)), ('apq_savgol', _sg(T=31, Cc=7, c1=7, c2=7, W0=31)),
    ('apq_savgol', _sg(T=512, c1=204, W0=31)), ('apq_savgol', _sg(T=9, c0=144, c1=144, W1=5, taps0=None)),       # the wide range empty
    ('apq_savgol', _sg(T=65536, Cc=204)), ('apq_savgol', _sg(c0=7, c1=7, c2=7, W0=0, W1=0, taps0=None, taps1=None)),
    ('apq_calib_baseline', _calib()), ('apq_calib_baseline', _calib(T=2, k=1)), ('apq_calib_baseline', _calib(T=10, k=5)),
    ('apq_calib_baseline', _calib(T=113, k=28)), ('apq_calib_baseline', _calib(T=512, k=511)),
    ('apq_segment_assemble', _seg()), ('apq_segment_assemble', _seg(T=1)), ('apq_segment_assemble', _seg(T=10, flags=3)),
    ('apq_segment_assemble', _seg(base=None, fid=None, flags=1)), ('apq_segment_assemble', _seg(base=None, fid=None, flags=2)),
    ('apq_image_landmarks', _img()), ('apq_image_landmarks', _img(T=46, n=1)), ('apq_image_landmarks', _img(T=1, stamps=None, n=0, flags=1)),
    ('apq_image_landmarks', _img(T=65536, n=4096)),
]

REFUSED = [
    # (call, arguments, code, what apq_last_error() names)
    ('apq_savgol', _sg(T=14), -2, 'T = 14 < W = 15'), ('apq_savgol', _sg(T=4, c0=144, c1=144), -2, 'T = 4 < W = 5'),
    ('apq_savgol', _sg(W0=14), -2, 'W0 = 14 is even'), ('apq_savgol', _sg(W1=6), -2, 'W1 = 6 is even'),
    ('apq_savgol', _sg(W0=33), -2, 'W0 = 33, served: 5 .. 31'), ('apq_savgol', _sg(W1=3), -2, 'W1 = 3, served: 5 .. 31'),
    ('apq_savgol', _sg(W0=32), -2, 'W0 = 32, served: 5 .. 31'),
    ('apq_savgol', _sg(x=None), -1, 'null x'), ('apq_savgol', _sg(y=None), -1, 'null y'), ('apq_savgol', _sg(taps0=None), -1, 'null taps0'),
    ('apq_savgol', _sg(taps1=None), -1, 'null taps1'), ('apq_savgol', _sg(y=A), -1, 'same buffer'),
    ('apq_savgol', _sg(x=A + 2), -2, 'x is not'), ('apq_savgol', _sg(y=B + 1), -2, 'y is not'), ('apq_savgol', _sg(taps0=C + 2), -2, 'taps0 is not'),
    ('apq_savgol', _sg(c1=205, c2=205), -1, 'column ranges'), ('apq_savgol', _sg(c0=150), -1, 'column ranges'), ('apq_savgol', _sg(c0=-1), -1, 'column ranges'),
    ('apq_savgol', _sg(T=0), -1, 'T = 0'), ('apq_savgol', _sg(Cc=0, c1=0, c2=0), -1, 'C = 0'), ('apq_savgol', _sg(T=65537), -2, 'T = 65537'),
    ('apq_savgol', _sg(T=65536, Cc=32768, c1=0, c2=0), -2, 'below 2^31'),
    ('apq_calib_baseline', _calib(T=513, k=256), -2, 'T = 513'), ('apq_calib_baseline', _calib(T=1, k=0), -1, 'T = 1'),
    ('apq_calib_baseline', _calib(k=0), -1, 'k = 0'), ('apq_calib_baseline', _calib(k=512), -1, 'k = 512'), ('apq_calib_baseline', _calib(k=-3), -1, 'k = -3'),
    ('apq_calib_baseline', _calib(x=None), -1, 'null x'), ('apq_calib_baseline', _calib(y=None), -1, 'null y'),
    ('apq_calib_baseline', _calib(x=A + 2), -2, 'x is not'), ('apq_calib_baseline', _calib(y=B + 3), -2, 'y is not'),
    ('apq_segment_assemble', _seg(T=513), -2, 'T = 513'), ('apq_segment_assemble', _seg(T=0), -1, 'T = 0'),
    ('apq_segment_assemble', _seg(inp=None), -1, 'null in'), ('apq_segment_assemble', _seg(out=None), -1, 'null out'),
    ('apq_segment_assemble', _seg(out=A), -1, 'same buffer'), ('apq_segment_assemble', _seg(fid=None), -1, 'base and fid come together'),
    ('apq_segment_assemble', _seg(flags=2), -1, 'belong to APQ_SEG_CLOSE'), ('apq_segment_assemble', _seg(flags=9), -1, 'flags = 9'),
    ('apq_segment_assemble', _seg(inp=A + 2), -2, 'in is not'), ('apq_segment_assemble', _seg(base=B + 2), -2, 'base is not'),
    ('apq_segment_assemble', _seg(fid=C + 1), -2, 'fid is not'), ('apq_segment_assemble', _seg(out=D + 2), -2, 'out is not'),
    ('apq_image_landmarks', _img(T=45), -2, 'T = 45'), ('apq_image_landmarks', _img(stamps=None), -1, 'null stamps'),
    ('apq_image_landmarks', _img(n=0), -2, 'n_stamps = 0'), ('apq_image_landmarks', _img(n=4097), -2, 'n_stamps = 4097'),
    ('apq_image_landmarks', _img(inp=None), -1, 'null in'), ('apq_image_landmarks', _img(out=None), -1, 'null out'),
    ('apq_image_landmarks', _img(out=A), -1, 'same buffer'), ('apq_image_landmarks', _img(scale=0.0), -1, 'scale'),
    ('apq_image_landmarks', _img(T=0), -1, 'T = 0'), ('apq_image_landmarks', _img(T=65537), -2, 'T = 65537'),
    ('apq_image_landmarks', _img(stamps=C + 2), -2, 'stamps is not'), ('apq_image_landmarks', _img(inp=A + 2), -2, 'in is not'),
    ('apq_image_landmarks', _img(flags=4), -1, 'flags = 4'),
]


@pytest.mark.parametrize('name,args', SERVED)
def test_ok_calls_accept_the_served_sizes(name, args):
    from animateportrait_amd import _seqapi
    assert getattr(_lib(), name + '_ok')(*args) == 1, _seqapi.last_error()


@pytest.mark.parametrize('name,args,code,reason', REFUSED)
def test_ok_calls_refuse_and_name_the_reason(name, args, code, reason):
    from animateportrait_amd import _seqapi
    assert getattr(_lib(), name + '_ok')(*args) == 0
    assert reason in _seqapi.last_error(), _seqapi.last_error()


@pytest.mark.parametrize('name,args,code,reason', REFUSED)
def test_launching_calls_return_the_same_codes_without_a_device(name, args, code, reason):
    """The checks run before anything touches the runtime: there is no device here, and the stream is null."""
    from animateportrait_amd import _seqapi
    assert code in (_seqapi.ERR_INVALID, _seqapi.ERR_UNSUPPORTED)
    assert getattr(_lib(), name)(*args, None) == code
    assert reason in _seqapi.last_error(), _seqapi.last_error()
    with pytest.raises(RuntimeError, match='libapseq'):
        _seqapi.check(getattr(_lib(), name)(*args, None), name)


def test_the_bindings_constants_are_the_headers():
    import re
    from animateportrait_amd import _seqapi
    hdr = open(os.path.join(ROOT, 'include', 'animateportrait_seq.h')).read()
    for macro, value in (('APQ_LM_C', _seqapi.LM_C), ('APQ_SG_MIN_W', _seqapi.SG_MIN_W), ('APQ_SG_MAX_W', _seqapi.SG_MAX_W),
                         ('APQ_SEG_MAX_T', _seqapi.SEG_MAX_T), ('APQ_MAX_STAMPS', _seqapi.MAX_STAMPS), ('APQ_SEG_CLOSE', _seqapi.SEG_CLOSE),
                         ('APQ_SEG_LIP', _seqapi.SEG_LIP), ('APQ_SEG_NOSE', _seqapi.SEG_NOSE), ('APQ_IMG_TRANSFORM', _seqapi.IMG_TRANSFORM),
                         ('APQ_IMG_EYES', _seqapi.IMG_EYES)):
        assert int(re.search(r'#define\s+%s\s+(\d+)' % macro, hdr).group(1)) == value, macro
    # every launching call is its _ok twin plus the stream
    for name, (_, args) in _seqapi.SIGNATURES.items():
        if name.endswith('_ok') and name != 'apq_lstm_layer_fwd_ok':
            assert _seqapi.SIGNATURES[name[:-3]][1] == args + [_seqapi._ptr], name


@pytest.mark.parametrize('T', [46, 200, 625])
@pytest.mark.parametrize('seed', [0, 5])
def test_blink_stamps_are_the_host_functions(T, seed):
    """The host add_naive_eye on a ramp: the two lids of a pair coincide exactly at the blink frames and nowhere else (the
    frames around a blink are blends with a weight > 0 on an open frame)."""
    from animateportrait_amd import landmark_host as lh, landmark_post as lp
    t, p, c = np.meshgrid(np.arange(T), np.arange(68), np.arange(3), indexing='ij')
    ramp = 0.01 * t + 1.0 * p + 0.1 * c
    r_host, r_fn = np.random.RandomState(seed), np.random.RandomState(seed)
    out = lh.add_naive_eye(ramp.copy(), r_host)
    seen = [f for f in range(T) if all(np.array_equal(out[f, a], out[f, b]) for a, b in ((37, 41), (38, 40), (43, 47), (44, 46)))]
    stamps = lp.blink_stamps(T, r_fn)
    assert lp.blink_stamps is lh.blink_stamps
    assert stamps == seen and stamps[0] == 30
    assert all(b - a >= 90 for a, b in zip(stamps, stamps[1:])) and all(s < T - 16 for s in stamps[1:]) and stamps[-1] + 15 <= T - 1
    assert len(stamps) == {46: 1, 200: 2}.get(T, len(stamps)) and (T != 625 or len(stamps) >= 4)
    # both generators went through the same draws
    sa, sb = r_host.get_state(), r_fn.get_state()
    assert sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]
    assert r_host.randint(1 << 30) == r_fn.randint(1 << 30)


@pytest.mark.parametrize('W', [5, 9, 15, 31])
def test_savgol_table_matches_scipy_in_float64(W):
    """The banded linear map the table describes against scipy.signal.savgol_filter (mode='interp') to 1e-12, at T = W (the
    window is the whole signal), T = W + 1 (one interior row) and a longer signal."""
    from scipy.signal import savgol_filter
    from animateportrait_amd import landmark_post as lp
    tab = lp.savgol_table(W)
    h = W // 2
    assert tab.shape == (h + 1, W) and tab.dtype == np.float64
    rs = np.random.RandomState(W)
    for T in (W, W + 1, 113):
        x = rs.randn(T, 4)
        y = np.empty_like(x)
        for t in range(T):
            if t < h:
                y[t] = tab[t] @ x[:W]
            elif t >= T - h:
                y[t] = tab[T - 1 - t] @ x[::-1][:W]
            else:
                y[t] = tab[h] @ x[t - h:t - h + W]
        assert np.abs(y - savgol_filter(x, W, 3, axis=0)).max() < 1e-12, (W, T)
    with pytest.raises(ValueError):
        lp.savgol_table(6)


def test_the_device_path_imports_no_scipy():
    code = ('import sys; from animateportrait_amd import landmark_post as lp; lp.savgol_table(31); '
            'print(sorted(m for m in sys.modules if m.split(".")[0] == "scipy")[:3])')
    got = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert got.returncode == 0, got.stderr
    assert got.stdout.split('\n')[-2] == '[]', got.stdout


@pytest.mark.parametrize('value,want', [('device', 'device'), ('host', 'host'), (None, 'host')])
def test_environment_switch_selects_the_post_backend(value, want):
    env = {k: v for k, v in os.environ.items() if k != 'APAMD_MODULE1_POST'}
    if value is not None:
        env['APAMD_MODULE1_POST'] = value
    got = subprocess.run([sys.executable, '-c', 'from animateportrait_amd import module1; print(module1.get_post_backend())'],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert got.returncode == 0, got.stderr
    assert got.stdout.split()[-1] == want


def test_environment_switch_refuses_an_unknown_name():
    env = dict(os.environ, APAMD_MODULE1_POST='gpu')
    got = subprocess.run([sys.executable, '-c', 'from animateportrait_amd import module1'], cwd=ROOT, env=env, capture_output=True,
                         text=True, timeout=120)
    assert got.returncode != 0 and 'ValueError' in got.stderr and "'gpu'" in got.stderr


def test_end2end_parser_takes_the_post_backend():
    from animateportrait_amd import end2end
    ap = end2end.make_parser()
    base = ['--photo', 'p.png', '--out', 'o']
    assert ap.parse_args(base + ['--module1_post', 'device']).module1_post == 'device'
    assert ap.parse_args(base + ['--module1_post', 'host']).module1_post == 'host'
    assert ap.parse_args(base).module1_post in (None, 'host')             # the default does not select the device path
    with pytest.raises(SystemExit):
        ap.parse_args(base + ['--module1_post', 'gpu'])


def test_set_post_backend_and_cpu_tensors_take_the_host_functions():
    """With 'device' selected, CPU networks and CPU arrays still go through numpy / scipy: the same bits, the same types."""
    from animateportrait_amd import module1 as m1
    from test_seq_lstm_cpu import _seeded_nets
    before = m1.get_post_backend()
    assert before == 'host'
    with pytest.raises(ValueError):
        m1.set_post_backend('gpu')
    assert m1.get_post_backend() == before
    netc, netg = _seeded_nets()
    g = torch.Generator().manual_seed(21)
    au, spk, fid = torch.randn(60, 18, 80, generator=g), torch.randn(256, generator=g), torch.randn(204, generator=g) * 0.1
    out = {}
    try:
        for name in ('host', 'device'):
            assert m1.set_post_backend(name) in m1.POST_BACKENDS
            assert m1.get_post_backend() == name
            fl = m1.predict_landmarks_speaker_aware(netg, netc, au, spk, fid)
            img = m1.to_image_landmarks(fl, scale=0.01, shift=(-128.0, -128.0), rng=np.random.RandomState(0))
            out[name] = (fl, img, m1.predict_landmarks(netc, au, fid, scale=0.01, shift=(-128.0, -128.0)))
    finally:
        m1.set_post_backend(before)
    assert m1.get_post_backend() == before
    assert out['host'][0].shape == (60, 204) and out['host'][1].shape == (60, 68, 3) and out['host'][2].shape == (60, 68, 2)
    for a, b in zip(out['host'], out['device']):
        assert isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype == np.float32
        assert np.array_equal(a, b)
