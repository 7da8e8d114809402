"""GPU (-m gpu): one G step and one D step of ``geomgm_ifw_cartoon_fore`` (3-channel frames) against a float64 torch-autograd
restatement of the same losses on the CPU, at the small configuration tests/test_train_gpu.py uses for the drawing step
(ngf = ndf = 8, B = 1, stand-in aux nets, fixed seeds), in both precisions that test runs; the cartoon dataset's device and
host batches; and the readme's training command end to end.

The restatement below is written from the reference's loss expressions (Module2/models/geomgm_ifw_cartoon_fore_model.py:
backward_G :672-775, backward_D_basic3 :608-630) on the oracle's layer functions (generator, PatchGAN, lsgan, masked, the aux
glue).  The forward composition (:512-560) is the drawing model's, line for line, so oracle.train_step.forward serves it.
As in the drawing test, the TPS-warped constants are handed from the product to the restatement: the fp32 spline solve is
ill-conditioned and has its own tests."""
import itertools
import os
import random
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cartoon_fixture as cf          # noqa: E402
from conftest import linf             # noqa: E402

pytestmark = pytest.mark.gpu

DNAMES = ['D_A', 'D_A_l', 'D_A_le', 'D_A_ll']
README = ['--model', 'geomgm_ifw_cartoon_fore', '--netG', 'resnet_9blocks_rcatland32_full_ifw', '--netg_resb_div', '3',
          '--netg_resb_disp', '3', '--output_nc', '3', '--lr', '0.00005', '--lambda_geom', '50', '--lambda_geom_lipline', '0',
          '--more_weight_for_lip', '2', '--lambda_face', '3.0', '--lambda_warp_inter', '10', '--blendbg', '1', '--niter', '70',
          '--niter_decay', '0']                                                                   # readme.md:67
# The parity budget of the drawing step, tests/test_train_gpu.py::_train_step_vs_oracle, for the same kernels and precision
# modes: a gradient tensor may be 3 x (the restatement's own fp32-vs-fp64 distance) + a floor from fp64 -- floor / floor_d there
# (generator / discriminators): 5e-5 / 5e-5 in exact fp32, 2e-3 / 1e-2 in split-bf16 -- relative to the tensor's largest element;
# a loss term 1e-3 relative + 1e-5 (G terms) or + 1e-6 (D losses); a generated frame 1e-3 L-inf.
FLOOR_G = {'fp32': 5e-5, 'bf16x3': 2e-3}
FLOOR_D = {'fp32': 5e-5, 'bf16x3': 1e-2}
LOSS_RTOL, LOSS_ATOL_G, LOSS_ATOL_D, FRAME_TOL = 1e-3, 1e-5, 1e-6, 1e-3


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


def _make_model(extra=()):
    from animateportrait_amd.options.base_options import TrainOptions
    from animateportrait_amd.models import create_model
    opt = TrainOptions().parse(README + ['--dataset_mode', 'synthetic', '--ngf', '8', '--ndf', '8', '--batch_size', '1',
                                         '--gpu_ids', '0'] + list(extra))
    return create_model(opt), opt


class Opt:
    """what oracle.train_step.forward reads, at the cartoon readme's values"""
    blendbg, mask_type, div, disp = 1, 3, 3, 3


def luminance(x):
    return 0.299 * x[:, 0:1] + 0.587 * x[:, 1:2] + 0.114 * x[:, 2:3]


def g_terms(sdD, o, batch, opt, aux, fake_B_warp):
    """backward_G of the cartoon model: every term of loss_names that the G step sets"""
    from oracle import discriminator as od, losses as ol, aux_glue as oa
    gan, D, t = ol.gan_loss_lsgan, od.patchgan_forward, {}
    t['G_A'] = gan(D(sdD['D_A'], o['fake_B']), True) + gan(D(sdD['D_A'], o['fake_B2']), True)
    for name, suf in (('D_A_l', ''), ('D_A_le', 'e'), ('D_A_ll', 'l')):
        t['G_A_l' + suf] = (gan(D(sdD[name], o['fake_B_l' + suf]), True)
                            + gan(D(sdD[name], o['fake_B2_l' + suf]), True)) * opt.lambda_G_A_l
    cs, mse = opt.crop_size, F.mse_loss
    lm1 = oa.get_lm(aux['landmarks'], o['fake_B'], batch['winB'])
    lm2 = oa.get_lm(aux['landmarks'], o['fake_B2'], batch['winB2'])
    t1, t2 = batch['tB_lm_68'][:, :68].to(lm1.dtype), batch['tB2_lm_68'][:, :68].to(lm1.dtype)
    assert opt.more_weight_for_lip == 2
    t['geom_B'] = (mse(lm1[:, :48] / cs, t1[:, :48] / cs) + 2 * mse(lm1[:, 48:68] / cs, t1[:, 48:68] / cs)
                   + mse(lm2[:, :48] / cs, t2[:, :48] / cs) + 2 * mse(lm2[:, 48:68] / cs, t2[:, 48:68] / cs)) * opt.lambda_geom
    t['warp_B'] = F.l1_loss(o['fake_B'], o['fakeB_static_warp']) * opt.lambda_warp
    t['warp_inter1'] = F.l1_loss(o['fake_B2'], fake_B_warp) * opt.lambda_warp_inter
    rep = lambda x: x.repeat(1, 3, 1, 1)                                    # noqa: E731
    if opt.identity_loss == 2:                                              # :743-749
        t['iden_B'] = torch.mean(oa.face_loss(aux['faceloss'], rep(luminance(o['fake_B'])), rep(luminance(batch['fakeB_static_fore'])),
                                              batch['winB'], batch['winA'])) * opt.lambda_face
    t['G'] = sum(t.values())
    return t


def d_terms(sdD, o, batch):
    from oracle import discriminator as od, losses as ol
    D = od.patchgan_forward
    out = {'D_A': ol.d_loss_basic3(D(sdD['D_A'], batch['B']), D(sdD['D_A'], o['fake_B'].detach()), D(sdD['D_A'], o['fake_B2'].detach()))}
    for name, suf in (('D_A_l', ''), ('D_A_le', 'e'), ('D_A_ll', 'l')):
        out[name] = ol.d_loss_basic3(D(sdD[name], o['real_B_l' + suf]), D(sdD[name], o['fake_B_l' + suf].detach()),
                                     D(sdD[name], o['fake_B2_l' + suf].detach()))
    return out


def _relerr(a, b64):
    b64 = b64.double()
    return float((a.detach().cpu().double() - b64).abs().max() / b64.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize('identity_loss', [2])
@pytest.mark.parametrize('precision', ['bf16x3', 'fp32'])
def test_cartoon_step_losses_and_grads_vs_float64(dev, precision, identity_loss, monkeypatch):
    """``--identity_loss 2`` (the model's default, given here by name): the identity term is computed on luminance planes and its
    gradient reaches the generator through the luminance kernel's backward; the term itself is pinned apart in
    test_identity_term_flows_through_the_luminance_kernel."""
    from animateportrait_amd import networks as N, standins, ops
    from animateportrait_amd.data.synthetic_dataset import make_train_batch
    from animateportrait_amd.models.sparse_image_warp import check_status
    from oracle import generator as og, discriminator as od, train_step as ts
    monkeypatch.setattr(ops, 'DEFAULT_PRECISION', ops.PRECISION_FP32 if precision == 'fp32' else ops.PRECISION_BF16X3)
    torch.manual_seed(0)
    model, opt = _make_model(['--identity_loss', str(identity_loss)])
    assert model.model_names == ['G_A'] + DNAMES and not hasattr(model, 'netD_A_coh')
    sdG = og.init_params(og.generator_param_shapes(3, 3, 8, 9, 3, 3), seed=11)
    model.netG_A.load_state_dict(sdG, strict=True)
    sdD = {}
    for i, name in enumerate(DNAMES):
        sdD[name] = og.init_params(od.patchgan_param_shapes(3 if name == 'D_A' else 4, 8), seed=20 + i)
        getattr(model, 'net' + name).load_state_dict(sdD[name], strict=True)
    model.aux['landmarks'] = standins.StandinLandmarkNet().to(dev)
    model.aux['faceloss'] = N.FaceLoss(standins.StandinFaceNet().to(dev))
    batch = make_train_batch(1, seed=5, output_nc=3)
    assert batch['B'].shape == (1, 3, 256, 256) and batch['fakeB_static'].shape == (1, 3, 256, 256)
    batch['winB'], batch['winB2'], batch['winA'] = (torch.tensor([w]) for w in ([-12, 200, 24, 230], [40, 260, 50, 256], [20, 230, 20, 228]))
    # ---------------- product
    model.set_input(batch)
    model.forward()
    nets_D = [getattr(model, 'net' + n) for n in DNAMES]
    model.set_requires_grad(nets_D, False)
    model.optimizer_G.zero_grad()
    model.backward_G()
    gG = {k: p.grad.detach().clone().cpu() for k, p in model.netG_A.named_parameters()}
    model.set_requires_grad(nets_D, True)
    model.optimizer_D.zero_grad()
    model.backward_D_A(); model.backward_D_A_l(); model.backward_D_A_le(); model.backward_D_A_ll()
    gD = {n: {k: p.grad.detach().clone().cpu() for k, p in getattr(model, 'net' + n).named_parameters()} for n in DNAMES}
    check_status()
    assert model.fake_B.shape == (1, 3, 256, 256) and model.fake_B_l.shape == (1, 4, 256, 256)
    ov32 = {k: getattr(model, k).detach().cpu() for k in ('mask1', 'mask2', 'fakeB_static_warp', 'fake_B_warp')}
    fakes32 = {k: getattr(model, k).detach().cpu() for k in ('fake_B', 'fake_B2', 'fake_B_l', 'fake_B2_l', 'fake_B_le', 'fake_B2_le',
                                                              'fake_B_ll', 'fake_B2_ll')}
    # ---------------- restatement, fp32 (the noise of the reference's own arithmetic) and fp64 (the truth)
    res = {}
    for tag, dt in (('f32', torch.float32), ('f64', torch.float64)):
        cast = lambda t: t.to(dt) if torch.is_tensor(t) and t.is_floating_point() else t     # noqa: E731
        sG = {k: cast(v).clone().requires_grad_(True) for k, v in sdG.items()}
        sD = {n: {k: cast(v).clone() for k, v in sd.items()} for n, sd in sdD.items()}
        b = {k: cast(v) for k, v in batch.items()}
        ov = {k: cast(v) for k, v in ov32.items()}
        aux = {'landmarks': standins.StandinLandmarkNet().to(dt), 'faceloss': standins.StandinFaceNet().to(dt)}
        o = ts.forward(sG, b, opt=Opt, overrides=ov)
        # blendbg = 1: the static cartoon stays whole (only --blendbg 0 composes it on white, :518-522)
        b['fakeB_static_fore'] = b['fakeB_static']
        terms = g_terms(sD, o, b, opt, aux, ov['fake_B_warp'])
        terms['G'].backward()
        for sd in sD.values():
            for v in sd.values():
                v.requires_grad_(True)
        od_ = dict(o)
        od_.update({k: cast(v) for k, v in fakes32.items()})      # the D step on the product's own frames, as the drawing test
        dl = d_terms(sD, od_, b)
        sum(dl.values()).backward()
        res[tag] = dict(o=o, terms=terms, dl=dl, gG={k: v.grad for k, v in sG.items()},
                        gD={n: {k: v.grad for k, v in sd.items()} for n, sd in sD.items()})
    r32, r64 = res['f32'], res['f64']
    # ---------------- frames and every loss term of loss_names
    for k in ('fake_B_fore', 'fake_B2_fore', 'fake_B', 'fake_B2', 'fake_B_l'):
        e = linf(getattr(model, k), r64['o'][k])
        print('%s %s L-inf %.3e' % (precision, k, e))
        assert e < FRAME_TOL, (k, e)
    want = list(model.loss_names)
    assert set(want) == set(r64['terms']) | set(r64['dl']), (want, sorted(r64['terms']), sorted(r64['dl']))
    for k in want:
        a = float(getattr(model, 'loss_' + k))
        t, atol = (float(r64['dl'][k].detach()), LOSS_ATOL_D) if k in r64['dl'] else (float(r64['terms'][k].detach()), LOSS_ATOL_G)
        print('%s loss %-12s product %.7f  fp64 %.7f' % (precision, k, a, t))
        assert abs(a - t) <= LOSS_RTOL * abs(t) + atol, (k, a, t)
    assert float(r64['terms']['iden_B']) > 0
    # ---------------- gradients: the generator's first layers (the stem on the image; the first key, the merge layer), its last
    # layer (Cout = 3) and the first layer of every discriminator (Cin = 3 and Cin = output_nc + 1 = 4)
    bad = []

    def check(tag, k, mine, g32, g64, floor):
        e, noise = _relerr(mine, g64), _relerr(g32, g64)
        print('%s grad %-6s %-24s err %.3e  fp32 noise %.3e' % (precision, tag, k, e, noise))
        if not e <= 3.0 * noise + floor:
            bad.append((tag, k, e, noise))
    assert gG['model3.7.weight'].shape == (3, 8, 7, 7) and gD['D_A']['model.0.weight'].shape == (8, 3, 4, 4) \
        and gD['D_A_l']['model.0.weight'].shape == (8, 4, 4, 4)
    for k in ('model_tri00.1.weight', 'model_tri_merge.weight', 'model3.7.weight', 'model3.7.bias'):
        check('G', k, gG[k], r32['gG'][k], r64['gG'][k], FLOOR_G[precision])
    for n in DNAMES:
        for k in ('model.0.weight', 'model.0.bias'):
            check(n, k, gD[n][k], r32['gD'][n][k], r64['gD'][n][k], FLOOR_D[precision])
    assert not bad, bad


def test_identity_term_flows_through_the_luminance_kernel(dev):
    """d iden_B / d fake_B of the product (FaceLoss on the luminance plane, backward through aps_luma_bwd) against autograd of the
    float64 restatement; budget: the drawing step's generator floor for exact-fp32 elementwise paths (5e-5,
    tests/test_train_gpu.py floor) on top of 3 x the restatement's fp32 noise."""
    from animateportrait_amd import networks as N, standins, losses
    from oracle import aux_glue as oa
    g = torch.Generator().manual_seed(4)
    fake = torch.rand(1, 3, 256, 256, generator=g) * 2 - 1
    static = torch.rand(1, 3, 256, 256, generator=g) * 2 - 1
    winB, winA = torch.tensor([[-12, 200, 24, 230]]), torch.tensor([[20, 230, 20, 228]])
    fl = N.FaceLoss(standins.StandinFaceNet().to(dev))
    x = fake.clone().to(dev).requires_grad_(True)
    loss = torch.mean(fl(losses.luminance(x), losses.luminance(static.to(dev)), bbox1=winB, bbox2=winA))
    loss.backward()
    ref = {}
    for tag, dt in (('f32', torch.float32), ('f64', torch.float64)):
        xr = fake.detach().clone().to(dt).requires_grad_(True)
        rep = lambda t: t.repeat(1, 3, 1, 1)                                # noqa: E731
        lr = torch.mean(oa.face_loss(standins.StandinFaceNet().to(dt), rep(luminance(xr)), rep(luminance(static.to(dt))), winB, winA))
        lr.backward()
        ref[tag] = (float(lr), xr.grad)
    assert abs(float(loss) - ref['f64'][0]) <= LOSS_RTOL * abs(ref['f64'][0]) + LOSS_ATOL_G
    e, noise = _relerr(x.grad, ref['f64'][1]), _relerr(ref['f32'][1], ref['f64'][1])
    print('d iden / d fake_B: err %.3e, fp32 noise %.3e' % (e, noise))
    assert float(ref['f64'][1].abs().max()) > 0 and e <= 3.0 * noise + FLOOR_G['fp32']
    # each channel's gradient is the luminance plane's scaled by its constant: a channel permutation would show
    gx = x.grad.cpu().double()
    assert linf(gx[:, 0] * 0.587, gx[:, 1] * 0.299) <= 1e-6 * float(gx.abs().max())
    assert linf(gx[:, 0] * 0.114, gx[:, 2] * 0.299) <= 1e-6 * float(gx.abs().max())


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    work = tmp_path_factory.mktemp('umlvd_cartoon_gpu')
    root, lists = str(work / 'tree'), str(work / 'lists')
    cf.write_tree(root, lists)
    return root, lists


def test_device_and_host_batches_have_equal_bits(dev, tree):
    """two batches of umlvd_ifw_cartoon from the fixture tree, prepared on the device and through PIL on the host"""
    from animateportrait_amd.data import create_dataset
    from animateportrait_amd.options.base_options import TrainOptions
    batches = {}
    for prep in ('device', 'host'):
        opt = TrainOptions().parse(README + ['--dataset_mode', 'umlvd_ifw_cartoon', '--dataroot', cf.NAME, '--list_dir', tree[1],
                                             '--batch_size', '1', '--gpu_ids', '0', '--data_prep', prep])
        ds = create_dataset(opt)
        assert type(ds).__name__ == 'UMLVDIFWCartoonDataset' and ds.data_prep == prep
        random.seed(3)
        torch.manual_seed(3)
        batches[prep] = list(itertools.islice(iter(ds), 2))
        assert len(batches[prep]) == 2
    for a, b in zip(batches['device'], batches['host']):
        assert set(a) == set(b) and a['B'].shape == (1, 3, 256, 256) and a['fakeB_static'].shape == (1, 3, 256, 256)
        assert not any(k in a for k in ('B1', 'B2', 'B3', 'B4', 'winBr1'))
        for k in a:
            if torch.is_tensor(a[k]):
                assert a[k].dtype == b[k].dtype and torch.equal(a[k].cpu(), b[k].cpu()), k
            else:
                assert a[k] == b[k], k


@pytest.mark.parametrize('mode', ['synthetic', 'umlvd_ifw_cartoon'])
def test_readme_command_trains_saves_and_end2end_loads(dev, tree, tmp_path, capsys, monkeypatch, mode):
    """the readme's cartoon command (readme.md:67) at ngf = ndf = 8: starts, steps, saves latest_net_G_A.pth with the reference's
    keys; the saved file loads strictly into the generator ``end2end --style cartoon`` builds"""
    import json
    from animateportrait_amd import train
    from conftest import GOLDEN
    ck = str(tmp_path / 'ck')
    data = ['--dataset_mode', 'synthetic', '--synthetic_batches', '2'] if mode == 'synthetic' else \
        ['--dataset_mode', 'umlvd_ifw_cartoon', '--dataroot', cf.NAME, '--list_dir', tree[1]]
    argv = [a for a in README] + data + ['--name', 'training/cartoon1', '--checkpoints_dir', ck, '--ngf', '8', '--ndf', '8',
                                         '--batch_size', '1', '--gpu_ids', '0', '--print_freq', '1', '--save_epoch_freq', '1']
    argv[argv.index('--niter') + 1] = '1'
    if mode != 'synthetic':
        # a file tree carries no matte / intrinsic flow: they come from the frozen nets BaseModel.setup attaches from
        # checkpoints/ -- here the fixed-seed stand-ins, as in tests/test_dataset_gpu.py::test_one_training_step_fed_by_the_dataset
        from animateportrait_amd import networks as N, standins
        from animateportrait_amd.models.base_model import BaseModel

        def attach(model):
            model.aux.update(landmarks=standins.StandinLandmarkNet().to(dev), faceloss=N.FaceLoss(standins.StandinFaceNet().to(dev)),
                             netF=standins.StandinFlowNet().to(dev), modnet=standins.StandinMatteNet().to(dev))
        monkeypatch.setattr(BaseModel, 'attach_aux_networks', attach)
    random.seed(1)
    torch.manual_seed(1)
    train.main(argv)
    out = capsys.readouterr().out
    assert 'End of epoch 1 / 1' in out and 'G_A:' in out and 'nan' not in out.lower()
    path = os.path.join(ck, 'training/cartoon1', 'latest_net_G_A.pth')
    sd = torch.load(path)
    ref = json.load(open(os.path.join(GOLDEN, 'cartoon_model.json')))['readme']
    assert list(sd.keys()) == ref['G_A_keys'] and sd['model3.7.weight'].shape == (3, 8, 7, 7)
    for name in DNAMES:
        assert os.path.exists(os.path.join(ck, 'training/cartoon1', 'latest_net_%s.pth' % name))
    assert not os.path.exists(os.path.join(ck, 'training/cartoon1', 'latest_net_D_A_coh.pth'))
    assert all(bool(torch.isfinite(v).all()) for v in sd.values())
    # end2end --style cartoon builds geomcgt_ifw_test with --output_nc 3 under an experiment name that contains 'cartoon' and
    # loads <checkpoints_dir>/<name>/latest_net_G_A.pth strictly (BaseModel.load_networks)
    from animateportrait_amd.models import create_model
    from animateportrait_amd.options.base_options import TestOptions
    model = create_model(TestOptions().parse(['--model', 'geomcgt_ifw_test', '--name', 'training/cartoon1', '--checkpoints_dir', ck,
                                              '--netG', 'resnet_9blocks_rcatland32_full_ifw', '--output_nc', '3', '--ngf', '8',
                                              '--netg_resb_div', '3', '--netg_resb_disp', '3', '--gpu_ids', '0']))
    assert model.cartoon
    model.load_networks('latest')
    assert torch.equal(model.netG_A.state_dict()['model3.7.weight'].cpu(), sd['model3.7.weight'])
