"""Static cartoon generator, host side: the state_dict contract of networks.Photo2CartoonGenerator, the restatement
(tests/photo2cartoon_reference.py) against the recorded outputs of the reference class, the C ABI of libapstyle.so and its
refusals (which need no device), and the uint8 round trip of the photo.

(The model itself -- ``--model geomcgt_ifw_test --name formal/cartoon`` -- has no CPU path, like every model here: its
construction is checked in tests/test_photo2cartoon_gpu.py.)"""
import ctypes
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import photo2cartoon_reference as pr      # noqa: E402


@pytest.fixture(scope='module')
def gd():
    return np.load(os.path.join(HERE, 'golden', 'photo2cartoon.npz'))


def sd_sha(sd):
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(v.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


@pytest.mark.parametrize('ngf', [8, 32])
def test_state_dict_has_the_reference_keys_order_and_shapes(gd, ngf):
    from animateportrait_amd import networks as N
    G = N.Photo2CartoonGenerator(ngf=ngf)
    got = [(k, ','.join(map(str, v.shape))) for k, v in G.state_dict().items()]
    want = list(zip(gd['keys_ngf%d' % ngf].tolist(), gd['shapes_ngf%d' % ngf].tolist()))
    assert got == want
    assert [(k, ','.join(map(str, s))) for k, s in pr.param_shapes(ngf)] == want
    for k in ('gap_fc.bias', 'gmp_fc.bias', 'HourGlass1.HG.1.ConvBlock4.2.weight'):        # keys without influence on the image
        assert k in dict(got)
    G.load_state_dict(pr.init_params(pr.param_shapes(ngf), 3), strict=True)              # as torch.load(path)['genA2B'] would


def test_light_false_and_bad_sizes_are_refused():
    from animateportrait_amd import networks as N
    with pytest.raises(NotImplementedError, match='light=False'):
        N.Photo2CartoonGenerator(ngf=8, light=False)
    G = N.Photo2CartoonGenerator(ngf=8)
    for shape in ((1, 3, 72, 64), (1, 3, 64, 40), (1, 1, 64, 64), (1, 3, 16, 16)):
        with pytest.raises(ValueError, match='multiples of 16'):
            G(torch.zeros(shape))


def test_restatement_reproduces_the_golden(gd):
    sd = pr.init_params(pr.param_shapes(int(gd['ngf'])), int(gd['seed_w']))
    assert sd_sha(sd) == str(gd['weights_sha256'])
    x = torch.rand(2, 3, int(gd['size']), int(gd['size']), generator=torch.Generator().manual_seed(int(gd['seed_x']))) * 2 - 1
    assert torch.equal(x, torch.from_numpy(gd['x']))
    y = torch.from_numpy(gd['y'])
    assert float(y.std()) >= 0.2                       # an absolute tolerance on a near-constant image would show nothing
    got = pr.generator_forward(sd, x)
    assert float((got - y.double()).abs().max()) < 1e-6          # the golden is stored as float32
    assert float((torch.from_numpy(gd['y0']) - y[:1]).abs().max()) < 1e-6      # the reference is batch independent


def test_lin_folding_equals_the_layer_as_written():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 6, 5, 7, generator=g, dtype=torch.float64) * 3 + 1
    rho = torch.rand(6, generator=g, dtype=torch.float64) * 2 - 0.5
    for gamma, beta in ((torch.randn(6, generator=g), torch.randn(6, generator=g)),
                        (torch.randn(2, 6, generator=g), torch.randn(2, 6, generator=g))):
        a, b = pr.lin_coeffs(x, rho, gamma.double(), beta.double())
        assert float((pr.affine_apply(x, a, b) - pr.lin(x, rho, gamma.double(), beta.double())).abs().max()) < 1e-12


def test_names_are_declared_and_exported():
    from animateportrait_amd import _styleapi as S, _capi
    header = open(os.path.join(ROOT, 'include', 'animateportrait_style.h')).read()
    assert all(n.startswith('aps_') and n + '(' in header for n in S.SIGNATURES)
    assert '#define APS_ABI_VERSION 1' in header and S.ABI_VERSION == 1
    lib = S.lib()
    assert all(hasattr(lib, n) for n in S.SIGNATURES) and lib.aps_abi_version() == 1
    for macro, value in (('APS_MAX_PLANES', S.MAX_PLANES), ('APS_MAX_SIDE', S.MAX_SIDE)):
        assert '#define %s %d' % (macro, value) in header
    assert not any(n.startswith('aps_') for n in _capi.SIGNATURES)         # the model library's ABI is untouched


def test_refusals_need_no_device():
    """Refused calls return a negative code and a message before anything touches a device: the pointers are never
    dereferenced, any non-null value stands in."""
    from animateportrait_amd import _styleapi as S
    lib = S.lib()
    p, null = ctypes.c_void_p(1 << 20), ctypes.c_void_p(0)

    def refused(rc, word):
        assert rc < 0 and word in S.last_error(), (rc, S.last_error())

    # null pointers
    refused(lib.aps_lin_coeffs(null, 1, 4, 8, 8, p, p, p, 0, 1e-5, p, p, p, null), 'null')
    refused(lib.aps_lin_coeffs(p, 1, 4, 8, 8, p, p, p, 0, 1e-5, p, null, p, null), 'null')
    refused(lib.aps_affine_apply(p, null, p, 0, null, 1, 4, 8, 8, p, null, null, null), 'null')
    refused(lib.aps_affine_apply(p, p, p, 0, null, 1, 4, 8, 8, null, null, null, null), 'null')
    refused(lib.aps_plane_combine(S.SUM3, p, p, null, null, 1, 4, 8, 8, 0, 0, 0, p, null, null, null), 'null')
    refused(lib.aps_plane_combine(S.POOL2, null, null, null, null, 1, 4, 8, 8, 0, 0, 0, p, null, null, null), 'null')
    # H W = 1: no unbiased variance
    refused(lib.aps_lin_coeffs(p, 2, 4, 1, 1, p, p, p, 0, 1e-5, p, p, p, null), 'unbiased')
    assert lib.aps_lin_coeffs_ok(p, p, p, p, p, p, p, 2, 4, 1, 1, 0) == 0 and lib.aps_lin_coeffs_ok(p, p, p, p, p, p, p, 2, 4, 1, 2, 0) == 1
    # a skip that is not exactly 2H x 2W
    refused(lib.aps_plane_combine(S.UP2ADD, p, p, null, null, 1, 4, 8, 8, 16, 15, 0, p, null, null, null), 'skip')
    assert lib.aps_plane_combine_ok(S.UP2ADD, p, p, null, null, 1, 4, 8, 8, 16, 16, 0, p, null, null) == 1
    assert lib.aps_plane_combine_ok(S.UP2ADD, p, null, null, null, 1, 4, 8, 8, 0, 0, 0, p, null, null) == 1       # plain up-sampling
    # JOIN with C no multiple of 4
    refused(lib.aps_plane_combine(S.JOIN, p, p, p, p, 1, 6, 8, 8, 0, 0, 0, p, null, null, null), 'multiple of 4')
    # the rest of the region
    refused(lib.aps_plane_combine(S.POOL2, p, null, null, null, 1, 4, 1, 8, 0, 0, 0, p, null, null, null), 'window')
    refused(lib.aps_plane_combine(S.SUM3, p, p, p, null, 1, 4, 8, 8, 0, 0, 0, p, p, null, null), 'together')
    refused(lib.aps_plane_combine(S.STAT, p, null, null, null, 1, 4, 8, 8, 0, 0, 0, p, p, null, null), 'STAT')
    refused(lib.aps_plane_combine(9, p, null, null, null, 1, 4, 8, 8, 0, 0, 0, p, null, null, null), 'mode')
    refused(lib.aps_affine_apply(p, p, p, 2, null, 1, 4, 8, 8, p, null, null, null), 'activation')
    refused(lib.aps_affine_apply(p, p, p, 0, null, 1, 4, 8, S.MAX_SIDE + 1, p, null, null, null), 'served')
    refused(lib.aps_affine_apply(p, p, p, 0, null, 256, 256, 8, 8, p, null, null, null), 'planes')
    refused(lib.aps_affine_apply(p, p, p, 0, null, 0, 4, 8, 8, p, null, null, null), 'empty')
    assert lib.aps_affine_apply_ok(p, p, p, p, p, p, 2, 3, 5, 7, 1) == 1


def test_uint8_round_trip_of_the_photo():
    """q(x) == ((x + 1) * 127.5).astype(uint8) / 127.5 - 1 in float32, at 0, +-1 and one ulp either side of a step."""
    from animateportrait_amd import style_ops
    steps = np.array([k / 127.5 - 1 for k in (1, 2, 64, 127, 128, 200, 254, 255)], dtype=np.float32)
    vals = np.concatenate([np.array([0.0, 1.0, -1.0], dtype=np.float32), steps, np.nextafter(steps, np.float32(2)),
                           np.nextafter(steps, np.float32(-2))]).astype(np.float32)
    vals = vals[(vals >= -1) & (vals <= 1)]
    want = (((vals + np.float32(1)) * np.float32(127.5)).astype(np.uint8) / np.float32(127.5) - np.float32(1)).astype(np.float32)
    got = style_ops.quantize_u8(torch.from_numpy(vals))
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), want)
    assert np.array_equal(pr.quantize_u8(torch.from_numpy(vals)).numpy(), want)
    # outside the contract: clamped to the byte range, not wrapped
    out = style_ops.quantize_u8(torch.tensor([-1.5, 1.25], dtype=torch.float32))
    assert out.tolist() == [-1.0, 1.0]


def test_host_checks_and_planners_under_the_sanitisers():
    """tools/style_host_check.cpp: csrc/style/style_checks.h as a stand-alone host program built with
    -fsanitize=address,undefined, every call swept over and past its served region."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('style_host_check', os.path.join(ROOT, 'tools', 'style_host_check.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    line = tool.run()
    assert line.startswith('style_host_check:') and line.endswith(' 0 failures')
