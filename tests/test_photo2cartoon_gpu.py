"""Static cartoon generator on the MI355X: the three libapstyle.so kernels against the float64 restatement
(tests/photo2cartoon_reference.py), networks.Photo2CartoonGenerator against the recorded outputs of the reference class, and the
'cartoon' branch of the streaming-inference model and of test.py.

Kernel tolerance: the project's own for InstanceNorm kernels, 2e-5 x max|ref| per compared tensor (test_gpu_parity.py:170-178).
Each kernel is compared on its OWN outputs: lin_coeffs on (a, b), affine_apply on y for given (a, b).  The chain of the two on planes
with mean 1e3 and deviation 1 is not compared with that bar, because no fp32 evaluation can meet it: a and b are then stored with
half an ulp of 1e3 (3e-5) each, which is the whole tolerance on an output of size 1."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest
import torch

from conftest import linf

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import photo2cartoon_reference as pr      # noqa: E402
import testset_fixture as tf              # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(2, 3, 2, 2), (1, 1, 5, 7), (2, 8, 16, 16), (1, 4, 64, 64), (1, 2, 256, 256)]
DATA = ['normal', 'offset', 'constant_plane']
REL = 2e-5


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    return torch.device('cuda:0')


def make(shape, kind, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    if kind == 'offset':
        x = x + 1000.0                             # planes with mean 1e3 and deviation 1
    elif kind == 'constant_plane':
        x[-1, -1] = 0.75
    return x


def close(got, ref, what):
    scale = max(float(ref.abs().max()), 1e-30)
    err = linf(got, ref)
    print('%s: L-inf %.3e, bar %.3e' % (what, err, REL * scale))
    assert got.shape == ref.shape and err <= REL * scale, what


# ------------------------------------------------------------------------------------------------ aps_lin_coeffs
@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('kind', DATA)
@pytest.mark.parametrize('per_sample', [False, True])
def test_lin_coeffs(dev, shape, kind, per_sample):
    from animateportrait_amd import style_ops as so
    n, c = shape[:2]
    x = make(shape, kind, 11)
    g = torch.Generator().manual_seed(12)
    rho = torch.rand(c, generator=g)
    rho[0] = -0.5                                   # used as given, no clamp
    if c > 1:
        rho[-1] = 1.5
    gamma = torch.randn((n, c) if per_sample else (c,), generator=g)
    beta = torch.randn((n, c) if per_sample else (c,), generator=g)
    gamma.view(-1)[0] = 0.0                         # a = 0 on one channel
    a, b = so.lin_coeffs(x.to(dev), rho.to(dev), gamma.to(dev), beta.to(dev))
    ra, rb = pr.lin_coeffs(x.double(), rho.double(), gamma.double(), beta.double())
    close(a.view(n, c), ra, 'a')
    close(b.view(n, c), rb, 'b')
    assert float(a.view(-1)[0]) == 0.0
    if kind == 'normal':
        # the chain equals the layer as written
        y = so.affine_apply(x.to(dev), a, b)
        close(y, pr.lin(x.double(), rho.double(), gamma.double(), beta.double()), 'lin')


def test_lin_layer_variance_is_combined_from_plane_moments(dev):
    """Planes whose means differ by far more than their spread: E[x^2] - E[x]^2 over the layer would lose the variance."""
    from animateportrait_amd import style_ops as so
    x = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(3)) + torch.tensor([1000., 1001., 999., 1000.5]).view(1, 4, 1, 1)
    rho = torch.zeros(4)                            # the layer statistics only
    a, b = so.lin_coeffs(x.to(dev), rho.to(dev), torch.ones(4, device=dev), torch.zeros(4, device=dev))
    ra, rb = pr.lin_coeffs(x.double(), rho.double(), torch.ones(4, dtype=torch.float64), torch.zeros(4, dtype=torch.float64))
    close(a.view(2, 4), ra, 'a')
    close(b.view(2, 4), rb, 'b')


# ------------------------------------------------------------------------------------------------ aps_affine_apply
@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('kind', DATA)
def test_affine_apply(dev, shape, kind):
    from animateportrait_amd import style_ops as so
    n, c = shape[:2]
    x = make(shape, kind, 21)
    g = torch.Generator().manual_seed(22)
    a, b = torch.randn(n * c, generator=g), torch.randn(n * c, generator=g)
    a[0] = 0.0
    if n * c > 1:
        a[1] = -abs(a[1])
    res = torch.randn(shape, generator=g)
    xd, ad, bd, rd = x.to(dev), a.to(dev), b.to(dev), res.to(dev)
    for relu in (False, True):
        for r, rr in ((None, None), (rd, res.double())):
            ref = pr.affine_apply(x.double(), a.double(), b.double(), relu, rr)
            close(so.affine_apply(xd, ad, bd, so.ACT_RELU if relu else so.ACT_NONE, r), ref, 'y')
    y, m, s = so.affine_apply(xd, ad, bd, so.ACT_RELU, rd, want_stats=True)
    ref = pr.affine_apply(x.double(), a.double(), b.double(), True, res.double())
    close(y, ref, 'y with stats')
    rm, rs = pr.instnorm_stats(y.double().cpu())    # of the tensor the consumer normalises
    close(m, rm, 'mean')
    close(s, rs, 'rstd')


# ------------------------------------------------------------------------------------------------ aps_plane_combine
def check_stats(y, m, s):
    rm, rs = pr.instnorm_stats(y.double().cpu())
    close(m, rm, 'mean')
    close(s, rs, 'rstd')


@pytest.mark.parametrize('shape', SHAPES + [(1, 2, 5, 7), (2, 3, 9, 2)])
@pytest.mark.parametrize('kind', DATA)
@pytest.mark.parametrize('stats', [False, True])
def test_plane_combine(dev, shape, kind, stats):
    from animateportrait_amd import style_ops as so
    n, c, h, w = shape
    x = make(shape, kind, 31)
    g = torch.Generator().manual_seed(32)
    xd = x.to(dev)

    def run(fn, ref, *args):
        out = fn(*args, want_stats=stats)
        y = out[0] if stats else out
        close(y, ref, fn.__name__)
        if stats:
            check_stats(y, out[1], out[2])

    # POOL2: an odd last row / column is dropped (5 x 7, 9 x 2 among the shapes)
    run(so.pool2, pr.pool2(x.double()), xd)
    # UP2ADD with a skip and with a null skip
    skip = make((n, c, 2 * h, 2 * w), kind, 33)
    run(so.up2_add, pr.up2_add(x.double(), skip.double()), xd, skip.to(dev))
    run(so.up2_add, pr.up2_add(x.double()), xd, None)
    # SUM3
    a, b = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    run(so.sum3, pr.sum3(x.double(), a.double(), b.double()), xd, a.to(dev), b.to(dev))
    # JOIN over 4 c output channels: parts of 2c, c and c channels
    r = make((n, 4 * c, h, w), kind, 34)
    p0, p1, p2 = (torch.randn((n, k, h, w), generator=g) for k in (2 * c, c, c))
    run(so.join, pr.join(r.double(), p0.double(), p1.double(), p2.double()), r.to(dev), p0.to(dev), p1.to(dev), p2.to(dev))
    # STAT
    if not stats:
        close(so.plane_mean(xd), x.double().mean(dim=(2, 3)), 'plane_mean')
        close(so.plane_mean(xd, relu=True), torch.relu(x.double()).mean(dim=(2, 3)), 'plane_mean relu')


def test_wrappers_refuse_what_the_library_refuses(dev):
    from animateportrait_amd import style_ops as so
    x = torch.zeros(1, 4, 8, 8, device=dev)
    with pytest.raises(RuntimeError, match='skip'):
        so.up2_add(x, torch.zeros(1, 4, 16, 15, device=dev))
    with pytest.raises(RuntimeError, match='unbiased'):
        so.lin_coeffs(torch.zeros(1, 4, 1, 1, device=dev), *(torch.zeros(4, device=dev),) * 3)
    with pytest.raises(RuntimeError, match='MI355X'):
        so.pool2(torch.zeros(1, 4, 8, 8))


# ------------------------------------------------------------------------------------------------ the network
@pytest.mark.parametrize('precision', ['default', 'fp32'])
def test_generator_against_the_reference_class(dev, golden, monkeypatch, precision):
    """The ngf-8 fixture (N = 2, 64 x 64): L-inf against the recorded tanh output below 1e-3, the budget of test_static_generator
    and of the bench gate; sample 0 alone equals sample 0 of the batch within the same bound.  The generator pins its convolutions
    to fp32 (networks.P2CConv), so the two cases must agree: the package's default precision does not leak into it.
    Measured: 8.0e-4 in both cases; stock fp32 operators on the CPU are 9.6e-4 from float64 on this fixture."""
    from animateportrait_amd import networks as N, ops
    if precision == 'fp32':
        monkeypatch.setattr(ops, 'DEFAULT_PRECISION', ops.PRECISION_FP32)
    gd = golden('photo2cartoon.npz')
    assert float(gd['y'].std()) >= 0.2
    sd = pr.init_params(pr.param_shapes(int(gd['ngf'])), int(gd['seed_w']))
    G = N.Photo2CartoonGenerator(ngf=int(gd['ngf'])).to(dev)
    G.load_state_dict(sd, strict=True)
    x = gd['x'].to(dev)
    y = G(x)
    y0 = G(x[:1].contiguous())
    err, err0, alone = linf(y, gd['y']), linf(y0, gd['y0']), linf(y0, y[:1])
    print('Photo2CartoonGenerator ngf 8 (%s): L-inf vs reference %.3e, sample 0 alone %.3e, alone vs batch %.3e' % (precision, err, err0, alone))
    assert y.shape == (2, 3, 64, 64) and err < 1e-3 and err0 < 1e-3 and alone < 1e-3


# ------------------------------------------------------------------------------------------------ the model
def cartoon_model(dev, extra=()):
    from animateportrait_amd.options.base_options import TestOptions
    from animateportrait_amd.models import create_model
    opt = TestOptions().parse(['--model', 'geomcgt_ifw_test', '--netG', 'resnet_9blocks_rcatland32_full_ifw', '--dataset_mode',
                               'synthetic', '--name', 'formal/cartoon', '--output_nc', '3', '--ngf', '8', '--netg_resb_div', '3',
                               '--netg_resb_disp', '3', '--gpu_ids', '0', '--allow_random_init'] + list(extra))
    with contextlib.redirect_stdout(io.StringIO()):
        return create_model(opt), opt


def test_cartoon_model_is_built_and_follows_the_checkpoint_rules(dev, tmp_path, monkeypatch):
    """``--name formal/cartoon`` builds the model (the parent commit raised NotImplementedError here); a missing
    checkpoints/static/cartoon.pt is an error without --allow_random_init, and a present one is read through ['genA2B']."""
    from animateportrait_amd import networks as N
    model, opt = cartoon_model(dev)
    assert isinstance(model.net_staticG, N.Photo2CartoonGenerator) and model.net_staticG.ngf == 32
    assert model.STATIC_CHECKPOINT == 'checkpoints/static/cartoon.pt'
    monkeypatch.chdir(tmp_path)
    opt.allow_random_init = False
    with pytest.raises(FileNotFoundError, match='cartoon.pt'):
        model.setup(opt)
    sd = pr.init_params(pr.param_shapes(32), 77)
    os.makedirs('checkpoints/static')
    torch.save({'genA2B': sd, 'genB2A': {}}, 'checkpoints/static/cartoon.pt')
    model.load_static(model.STATIC_CHECKPOINT)
    assert torch.equal(model.net_staticG.state_dict()['DecodeBlock3.norm2.w_beta'].cpu(), sd['DecodeBlock3.norm2.w_beta'])


def test_cartoon_streaming_model(dev):
    """fakeB_static against the restatement at ngf 32 (< 1e-3), fake_B == bg_blend(fake_B_fore, fakeB_static, mask1), and the
    cache: a second frame with the same photo tensor does not call the static generator."""
    from animateportrait_amd import losses
    from animateportrait_amd.synthetic import make_generator_inputs
    model, _ = cartoon_model(dev)
    sd = pr.init_params(pr.param_shapes(32), 2468)
    model.net_staticG.load_state_dict(sd, strict=True)
    n = 1
    d = make_generator_inputs(n, seed=21)
    yy, xx = torch.meshgrid(torch.arange(256.), torch.arange(256.), indexing='ij')
    matte = ((((yy - 128) / 90) ** 2 + ((xx - 120) / 70) ** 2) < 1).float().view(1, 1, 256, 256).repeat(n, 1, 1, 1).contiguous()
    batch = {'A': d['input'], 'warp_motion': d['motion'], 'A_lm': d['land1'], 'tB_lm': d['land2'], 'iw_flow': d['flow'],
             'if_mask': d['ifmask'], 'matte': matte}
    model.set_input(batch)
    model.test()
    static = pr.generator_forward(sd, pr.quantize_u8(d['input']))
    assert float(static.std()) >= 0.2
    err = linf(model.fakeB_static, static)
    print('cartoon model: fakeB_static ngf 32, 256 x 256, L-inf vs restatement %.3e' % err)
    assert model.fakeB_static.shape == (n, 3, 256, 256) and err < 1e-3
    assert model.fake_B.shape == (n, 3, 256, 256)
    assert torch.equal(model.fake_B, losses.bg_blend(model.fake_B_fore, model.fakeB_static, model.mask1))
    calls = []
    orig = model.net_staticG.forward
    model.net_staticG.forward = lambda *a: (calls.append(1), orig(*a))[1]
    model.set_input(batch)
    model.test()
    assert not calls
    model.set_input(dict(batch, A=batch['A'].clone()))
    model.test()
    assert len(calls) == 1


def test_entry_point_writes_three_channel_cartoon_pngs(dev, tmp_path, tmp_path_factory):
    from PIL import Image
    from animateportrait_amd import end2end, standins, test as entry
    work = tmp_path_factory.mktemp('cartoon_tree')
    root, lists = str(work / 'tree'), str(work / 'lists')
    tf.write_test_tree(root, lists)
    kept = []

    def prepare(model):
        model.aux['netF'] = standins.StandinFlowNet().to(dev)
        model.aux['modnet'] = standins.StandinMatteNet().to(dev)
        run = model.test

        def test_and_keep():
            run()
            kept.append((list(model.get_image_paths()), model.fake_B.detach().clone(), model.fakeB_static.detach().clone()))
        model.test = test_and_keep
    argv = ['--model', 'geomcgt_ifw_test', '--netG', 'resnet_9blocks_rcatland32_full_ifw', '--netg_resb_div', '3', '--netg_resb_disp',
            '3', '--output_nc', '3', '--ngf', '8', '--dataset_mode', 'umlvdfw_test', '--dataroot', tf.NAME, '--list_dir', lists,
            '--draw_op', '1', '--lmark_lookup', tf.LOOKUP, '--batch_size', '2', '--gpu_ids', '0', '--allow_random_init', '--name',
            'formal/cartoon', '--checkpoints_dir', str(tmp_path / 'ck'), '--results_dir', str(tmp_path / 'res'), '--save_format', 'png']
    entry.main(argv, prepare_model=prepare)
    out = tmp_path / 'res' / 'formal' / 'cartoon' / 'test_latest' / 'images'
    stems = [os.path.splitext(p)[0] for paths, _, _ in kept for p in paths]
    assert stems == ['p0->p1', 'p1->d0', 'p2->d1']
    frames = torch.cat([f for _, f, _ in kept])
    static = torch.cat([s for _, _, s in kept])
    assert frames.shape == (3, 3, 256, 256) and static.shape == (3, 3, 256, 256)
    for i, s in enumerate(stems):
        png = np.asarray(Image.open(out / ('%s_fake_B.png' % s)))
        assert png.shape == (256, 256, 3) and np.array_equal(png, end2end.tensor2im(frames[i])), s
        assert (png[:, :, 0] != png[:, :, 1]).any()                      # three channels of their own, not a grey image
        assert np.array_equal(np.asarray(Image.open(out / ('%s_fakeB_static.png' % s))), end2end.tensor2im(static[i])), s


def test_end2end_style_cartoon(dev, tmp_path):
    """end2end.main --style cartoon on a synthetic 3-frame clip: the model options of the cartoon experiment without naming them,
    three-channel frames in the PNG and the AVI sinks."""
    from PIL import Image
    from animateportrait_amd import end2end, standins
    from animateportrait_amd.synthetic import make_landmarks
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import jpeg_fixture as jf
    yy, xx = np.meshgrid(np.linspace(-1, 1, 256), np.linspace(-1, 1, 256), indexing='ij')
    photo = np.stack([np.sin(3 * xx + yy), np.cos(2 * yy - xx), xx * yy], -1)
    Image.fromarray(((photo + 1) * 127.5).astype(np.uint8)).save(tmp_path / 'photo.png')
    Image.fromarray(((((yy / 0.8) ** 2 + (xx / 0.6) ** 2) < 1) * 255).astype(np.uint8)).save(tmp_path / 'matte.png')
    lm0 = make_landmarks(1, torch.Generator().manual_seed(9))[0]
    t = torch.arange(3).view(3, 1, 1).float()
    seq = lm0.unsqueeze(0) + 2.0 * torch.sin(0.3 * t + lm0.unsqueeze(0) / 40.0)
    np.save(tmp_path / 'lm.npy', torch.cat([lm0.unsqueeze(0), seq]).numpy())
    built = []

    def prepare(model):
        model.aux['netF'] = standins.StandinFlowNet().to(dev)
        model.aux['modnet'] = standins.StandinMatteNet().to(dev)
        built.append(model)
    out = tmp_path / 'out'
    assert end2end.main(['--photo', str(tmp_path / 'photo.png'), '--matte', str(tmp_path / 'matte.png'), '--landmarks_npy',
                         str(tmp_path / 'lm.npy'), '--out', str(out), '--batch', '2', '--video', 'avi', '--style', 'cartoon', '--ngf', '8',
                         '--allow_random_init', '--checkpoints_dir', str(tmp_path / 'ck')], prepare_model=prepare) == 0
    model = built[0]
    assert model.cartoon and model.opt.name == 'formal/cartoon' and model.opt.output_nc == 3 and model.opt.blendbg == 1
    files = sorted(os.listdir(out / 'frames'))
    assert len(files) == 3
    for f in files:
        png = np.asarray(Image.open(out / 'frames' / f))
        assert png.shape == (256, 256, 3) and (png[:, :, 0] != png[:, :, 2]).any()
    got = jf.read_avi((out / 'output.avi').read_bytes())
    assert got['avih'][4] == 3 and len([p for cc, p in got['movi'] if cc == b'00dc']) == 3
    with pytest.raises(SystemExit):
        end2end.main(['--photo', 'p', '--landmarks_npy', 'l', '--out', 'o', '--style', 'cartoon', '--name', 'run'])
