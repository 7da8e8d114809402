"""GPU (-m gpu): the HIP path, called through the C ABI, against the oracle and the goldens
captured from the reference.  Tolerances are L-inf in fp32, as north_star states (1e-3 on the
generator output); per-op checks are tighter."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import linf, sd_sha

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


def _layer(dev, w, b, **kw):
    from animateportrait_amd.networks import ConvLayer
    transposed = kw.get('transposed', False)
    cout = w.shape[1] if transposed else w.shape[0]
    cin = w.shape[0] if transposed else w.shape[1]
    segs = kw.pop('segs', [cin])
    l = ConvLayer(segs, cout, w.shape[2], **kw).to(dev)
    with torch.no_grad():
        l.weight.copy_(w)
        if b is not None:
            l.bias.copy_(b)
    return l


def _load_block(dev, blk, gd, prefix):
    with torch.no_grad():
        for k, p in blk.state_dict().items():
            p.copy_(gd[prefix + k])


def test_library_loaded():
    from animateportrait_amd import _capi
    assert b'gfx950' in _capi.lib().ap_version()


def test_resnet_blocks(dev, golden):
    from animateportrait_amd import networks as N, ops
    gd = golden('ops_small.npz')
    rb = N.ResnetBlock(16).to(dev)
    _load_block(dev, rb, gd, 'rb_')
    x = ops.Feat(gd['rb_x'].to(dev))
    first = rb.conv_block['1'].run(x, norm_act=ops.ACT_RELU)
    assert linf(ops.materialize(first).data, gd['rb_first']) < 2e-5
    assert linf(rb.run(x).data, gd['rb_y']) < 5e-5
    rb2 = N.ResnetBlock2([16, 1, 1], 16).to(dev)
    _load_block(dev, rb2, gd, 'rb2_')
    xx = gd['rb2_x'].to(dev)
    srcs = [ops.Feat(xx[:, :16].contiguous()), ops.Feat(xx[:, 16:17].contiguous()), ops.Feat(xx[:, 17:18].contiguous())]
    assert linf(rb2.run(srcs).data, gd['rb2_y']) < 5e-5


def test_generator_pieces(dev, golden):
    from animateportrait_amd import networks as N, ops
    from oracle import generator as og
    gd = golden('ops_small.npz')
    sd = og.init_params(og.generator_param_shapes(3, 1, 8, 9, 3, 3), seed=1234)
    G = N.define_G(3, 1, 8, 'resnet_9blocks_rcatland32_full_ifw', 'instance', False, 'normal', 0.02, [0], div=3, disp=3)
    G.load_state_dict(sd, strict=True)
    x = ops.Feat(gd['stem_x'].to(dev))
    assert linf(ops.materialize(G.model_tri10['1'].run(x, norm_act=ops.ACT_RELU)).data, gd['stem10_y']) < 2e-5
    assert linf(ops.materialize(G.model_tri00['1'].run(x, norm_act=ops.ACT_RELU)).data, gd['stem00_y']) < 2e-5
    x = ops.Feat(gd['down_x'].to(dev))
    assert linf(ops.materialize(G.model_tri01['0'].run(x, norm_act=ops.ACT_RELU)).data, gd['down01_y']) < 2e-5
    x = ops.Feat(gd['up_x'].to(dev))
    up = G.model3['0'].run(x, norm_act=ops.ACT_RELU)
    assert linf(ops.materialize(up).data, gd['up_y']) < 2e-5
    up2 = G.model3['3'].run(up, norm_act=ops.ACT_RELU)
    assert linf(ops.materialize(up2).data, gd['up2_y']) < 2e-5
    assert linf(G.model3['7'].run(up2, act=ops.ACT_TANH).data, gd['final_y']) < 2e-5
    l = ops.Feat(gd['land_x'].to(dev))
    l = G.model_landmark_trans['0'].run(l, norm_act=ops.ACT_RELU)
    l = G.model_landmark_trans['3'].run(l, norm_act=ops.ACT_RELU)
    l = G.model_landmark_trans['6'].run(l, norm_act=ops.ACT_NONE)
    assert linf(ops.materialize(l).data, gd['land_y']) < 5e-5


def test_double_feature_warping(dev, golden):
    from animateportrait_amd import ops
    from animateportrait_amd.synthetic import make_generator_inputs
    gd = golden('dfw.npz')
    d = make_generator_inputs(1, seed=int(gd['seed']))
    mo, fl, mk = d['motion'].to(dev), d['flow'].to(dev), d['ifmask'].to(dev)
    for level, size in ((0, 256), (1, 128), (2, 64)):
        x = torch.randn(1, 2, size, size, generator=torch.Generator().manual_seed(100 + level))
        y = ops.warp_concat(ops.Feat(x.to(dev)), mo, fl, mk, level).data.cpu()
        diff = (y - gd['y%d' % level]).abs()
        # the mask threshold (> 0.5 after a bilinear resize) is discontinuous: allow isolated flips
        assert float((diff > 1e-4).float().mean()) < 1e-4, (level, float(diff.max()))


def test_warp_of_virtual_feature(dev):
    """IN+ReLU applied per gathered tap == warping the materialised tensor."""
    from animateportrait_amd import ops
    from animateportrait_amd.synthetic import make_generator_inputs
    from oracle import warp as ow
    d = make_generator_inputs(2, seed=5)
    x = torch.randn(2, 8, 64, 64, generator=torch.Generator().manual_seed(2)) * 3 + 1
    ref = ow.double_feature_warping(F.relu(F.instance_norm(x)), d['motion'], d['flow'], d['ifmask'], 2)
    m = x.mean((2, 3)).reshape(-1)
    r = 1.0 / torch.sqrt(x.var((2, 3), unbiased=False).reshape(-1) + 1e-5)
    f = ops.Feat(x.to(dev), m.to(dev), r.to(dev), ops.ACT_RELU)
    y = ops.warp_concat(f, d['motion'].to(dev), d['flow'].to(dev), d['ifmask'].to(dev), 2).data.cpu()
    assert float(((y - ref).abs() > 1e-4).float().mean()) < 1e-4


def _decode_split(xs, n, c, h, w):
    """XS[n][head|tail][c/8][h*w + 1][8 x bf16] (include/animateportrait_amd.h) -> (head + tail as fp32 NCHW,
    the all-zero slots)."""
    t = xs.view(torch.bfloat16).view(n, 2, c // 8, h * w + 1, 8).float()
    val = (t[:, 0] + t[:, 1])[:, :, :h * w]                      # n, c/8, hw, 8
    return val.permute(0, 1, 3, 2).reshape(n, c, h, w), t[:, :, :, h * w]


def test_warp_split_output(dev):
    """The warp kernel's split-bf16 output (what the next split-bf16 conv stages) carries the same values as its
    fp32 output, to the 16 mantissa bits a bf16 head + tail hold; split-only mode writes no fp32 tensor."""
    from animateportrait_amd import ops
    from animateportrait_amd.synthetic import make_generator_inputs
    d = make_generator_inputs(2, seed=9)
    mo, fl, mk = d['motion'].to(dev), d['flow'].to(dev), d['ifmask'].to(dev)
    x = torch.randn(2, 16, 64, 64, generator=torch.Generator().manual_seed(3)) * 3 + 1
    m = x.mean((2, 3)).reshape(-1)
    r = 1.0 / torch.sqrt(x.var((2, 3), unbiased=False).reshape(-1) + 1e-5)

    def feat():
        return ops.Feat(x.to(dev), m.to(dev), r.to(dev), ops.ACT_RELU)
    plain = ops.warp_concat(feat(), mo, fl, mk, 2)
    both = ops.warp_concat(feat(), mo, fl, mk, 2, emit_xs=True)
    only = ops.warp_concat(feat(), mo, fl, mk, 2, emit_xs=True, keep_fp32=False)
    assert plain.xs is None and torch.equal(both.data, plain.data)
    assert only.is_split_only and tuple(only.shape) == (2, 32, 64, 64) and torch.equal(only.xs, both.xs)
    val, zeros = _decode_split(both.xs, 2, 32, 64, 64)
    assert float(zeros.abs().max()) == 0.0
    err = (val - plain.data).abs()
    assert float((err - plain.data.abs() * 2.0 ** -16).max()) <= 1e-30
    with pytest.raises(RuntimeError):
        ops.materialize(ops.Feat(only.data, m.to(dev).repeat(2), r.to(dev).repeat(2)))   # no fp32 data to read


@pytest.mark.parametrize('shape', [(2, 64, 32, 32), (1, 48, 17, 23), (2, 8, 40, 40)])
def test_fused_norm_residual_split(dev, shape):
    """ap_norm_apply_split: InstanceNorm finalised from the conv's partial tiles + activation + residual add, written
    as fp32 and as the split copy in one pass == finalize + instnorm_apply + split_prepass."""
    from animateportrait_amd import ops
    from animateportrait_amd.networks import ConvLayer
    n, c, h, w = shape
    g = torch.Generator().manual_seed(n * 1000 + c)
    src = ops.Feat((torch.randn(n, 16, h, w, generator=g) * 2).to(dev))
    res = torch.randn(n, c, h, w, generator=g).to(dev)
    layer = ConvLayer([16], c, 3, 1, 1, ops.PAD_REFLECT).to(dev)
    with torch.no_grad():
        layer.weight.copy_(torch.randn(layer.weight.shape, generator=g) * 0.1)
    a = layer.run(src, norm_act=ops.ACT_RELU)        # statistics pending
    b = layer.run(src, norm_act=ops.ACT_RELU)
    assert a.pending is not None
    mean, rstd = b.mean.clone(), b.rstd.clone()       # standalone finalize
    y, xs = ops._norm_apply_split(a, ops.Feat(res), want_y=True, want_xs=True)
    assert a.pending is None and torch.equal(a.mean, mean) and torch.equal(a.rstd, rstd)
    ref = F.relu(F.instance_norm(b.data.double().cpu())) + res.double().cpu()
    assert linf(y, ref) < 2e-5 * float(ref.abs().max())
    val, zeros = _decode_split(xs, n, c, h, w)
    assert float(zeros.abs().max()) == 0.0
    assert float(((val - y).abs() - y.abs() * 2.0 ** -16).max()) <= 1e-30
    # the split of a plain feature, and of a virtual one without residual
    xs2 = ops.presplit(ops.Feat(y))
    assert torch.equal(_decode_split(xs2, n, c, h, w)[0], val)
    y3, xs3 = ops._norm_apply_split(b, None, want_y=True, want_xs=True)
    assert linf(y3, F.relu(F.instance_norm(b.data.double().cpu()))) < 2e-5 * float(ref.abs().max())
    assert float(((_decode_split(xs3, n, c, h, w)[0] - y3).abs() - y3.abs() * 2.0 ** -16).max()) <= 1e-30


@pytest.mark.parametrize('disp', [3, 1])
def test_generator_ngf8(dev, golden, disp):
    from animateportrait_amd import networks as N
    from animateportrait_amd.synthetic import make_generator_inputs, generator_args
    from oracle import generator as og
    gd = golden('gen_ngf8.npz')
    d = make_generator_inputs(2, seed=1234)
    sd = og.init_params(og.generator_param_shapes(3, 1, 8, 9, 3, disp), seed=1234)
    G = N.define_G(3, 1, 8, 'resnet_9blocks_rcatland32_full_ifw', 'instance', False, 'normal', 0.02, [0], div=3, disp=disp)
    G.load_state_dict(sd, strict=True)
    with torch.no_grad():
        y = G(*[a.to(dev) for a in generator_args(d)])
    assert y.shape == (2, 1, 256, 256)
    assert linf(y, gd['y_disp%d' % disp]) < 1e-3


def test_generator_ngf64_headline_tolerance(dev, golden):
    """BASELINE config 2: full-width generator, fp32, within 1e-3 L-inf of the reference output."""
    from animateportrait_amd import networks as N
    from animateportrait_amd.synthetic import make_generator_inputs, generator_args
    from oracle import generator as og
    gd = golden('gen_ngf64.npz')
    d = make_generator_inputs(2, seed=1234)
    sd = og.init_params(og.generator_param_shapes(3, 1, 64, 9, 3, 3), seed=1234)
    assert sd_sha(sd) == str(gd['weights_sha256'])
    G = N.define_G(3, 1, 64, 'resnet_9blocks_rcatland32_full_ifw', 'instance', False, 'normal', 0.02, [0], div=3, disp=3)
    G.load_state_dict(sd, strict=True)
    with torch.no_grad():
        y = G(*[a.to(dev) for a in generator_args(d)])
        y1 = G(*[a[:1].to(dev) for a in generator_args(d)])
    err = linf(y, gd['y'])
    print('ngf64 generator L-inf vs reference: %.3e' % err)
    assert err < 1e-3
    assert torch.equal(y1, y[:1]), 'samples must be independent (InstanceNorm): B=1 == B=2[0] bitwise'


@pytest.mark.parametrize('batch', (16, 8, 5))
def test_generator_ngf64_at_the_reported_batch(dev, batch):
    """The configuration bench.py reports (BASELINE configs[1]: ngf=64, B=16, seed 1234) against the oracle's forward of the
    SAME batch (networks.py:1315-1340 restated in oracle/generator.py; a few seconds of host time): at B=16 the plan takes
    the 16-row 3x3 tile -- the kernel that is most of the timed step and that the B=2 golden test never runs -- and B=5 gives
    a tile list that is not a multiple of the 8 XCDs.  Which instantiations ran is read back through ap_conv2d_kernel_name."""
    from animateportrait_amd import networks as N, ops
    from animateportrait_amd.synthetic import make_generator_inputs, generator_args
    from oracle import generator as og
    args = generator_args(make_generator_inputs(batch, seed=1234))
    sd = og.init_params(og.generator_param_shapes(3, 1, 64, 9, 3, 3), seed=1234)
    G = N.define_G(3, 1, 64, 'resnet_9blocks_rcatland32_full_ifw', 'instance', False, 'normal', 0.02, [0], div=3, disp=3)
    G.load_state_dict(sd, strict=True)
    prof = ops.LaunchProfiler()
    ops.PROFILER = prof
    try:
        with torch.no_grad():
            y = G(*[a.to(dev) for a in args])
    finally:
        ops.PROFILER = None
    names = {r[0].replace(' ', '') for r in prof.records}
    with torch.no_grad():
        ref = og.generator_forward(sd, *args, div=3, disp=3)
    err = linf(y, ref)
    print('ngf64 B=%d generator L-inf vs oracle: %.3e; kernels: %s' % (batch, err, sorted(names)))
    assert 'Bf3Cfg<1,3,1,2,4,4>' in names, names      # the 16-row tile of the 3x3 stride-1 kernel
    assert err < 1e-3
    # the batch is sample-independent: the first frame alone gives the same bits
    with torch.no_grad():
        y1 = G(*[a[:1].to(dev) for a in args])
    assert linf(y1, ref[:1]) < 1e-3


def test_trunk_raw_outputs_in_the_channel_octet_layout(dev, monkeypatch):
    """Inference, round 6: the trunk convolutions whose raw output is read by one split-only norm pass write the channel-octet layout
    (ap_conv2d_fwd_octet on the 3x3 kernel; ap_norm_apply_split_ex flags bit 4 -> norm_split_oct_kernel, residual none or the
    previous block's split copy).  Same values as the NCHW route up to the order of the statistics' row sums, both within the
    path's budget of the oracle; B = 2 (4-row tiles) and B = 8 (16-row tiles)."""
    from animateportrait_amd import networks as N, ops
    from animateportrait_amd.synthetic import make_generator_inputs, generator_args
    from oracle import generator as og
    sd = og.init_params(og.generator_param_shapes(3, 1, 64, 9, 3, 3), seed=21)
    G = N.define_G(3, 1, 64, 'resnet_9blocks_rcatland32_full_ifw', 'instance', False, 'normal', 0.02, [0], div=3, disp=3)
    G.load_state_dict(sd, strict=True)
    for b in (2, 8):
        args = generator_args(make_generator_inputs(b, seed=21))
        outs = {}
        for flag in (True, False):
            monkeypatch.setattr(ops, 'OCTET_TRUNK', flag)
            calls = []
            real = ops._norm_apply_split

            def spy(f, *a, **k):
                calls.append(f.oct is not None)
                return real(f, *a, **k)
            monkeypatch.setattr(ops, '_norm_apply_split', spy)
            with torch.no_grad():
                outs[flag] = G(*[a.to(dev) for a in args])
            monkeypatch.setattr(ops, '_norm_apply_split', real)
            assert (sum(calls) == 15) if flag else (sum(calls) == 0), (flag, sum(calls), len(calls))
        with torch.no_grad():
            ref = og.generator_forward(sd, *args, div=3, disp=3)
        assert linf(outs[True], outs[False]) < 2e-4            # (InstanceNorm statistics summed in another order: ~6e-5 at ngf 64)
        assert linf(outs[True], ref) < 1e-3 and linf(outs[False], ref) < 1e-3


@pytest.mark.parametrize('ngf', [16, 20])
def test_generator_width_whose_upconvolution_reads_fp32(dev, ngf):
    """at 4 * ngf in {48, 64, 80} the trunk output qualifies for the split-only residual stream (c >= 48, c % 16 == 0)
    but the first up-convolution (dim -> dim / 2 <= 40 outputs, < 128 inputs) stays on the fp32 kernel: the last block must
    keep its fp32 tensor (autograd.materialize_forward consumer=...).  Inference raised a RuntimeError there."""
    from animateportrait_amd import networks as N
    from animateportrait_amd.synthetic import make_generator_inputs, generator_args
    from oracle import generator as og
    args = generator_args(make_generator_inputs(2, seed=5))
    sd = og.init_params(og.generator_param_shapes(3, 1, ngf, 9, 3, 3), seed=5)
    G = N.define_G(3, 1, ngf, 'resnet_9blocks_rcatland32_full_ifw', 'instance', False, 'normal', 0.02, [0], div=3, disp=3)
    G.load_state_dict(sd, strict=True)
    with torch.no_grad():
        y = G(*[a.to(dev) for a in args])
        ref = og.generator_forward(sd, *args, div=3, disp=3)
    assert linf(y, ref) < 1e-3


@pytest.mark.parametrize('ngf', [8, 64])
def test_generator_output_nc3_cartoon_configuration(dev, ngf):
    """The cartoon configuration (readme.md:67, `--output_nc 3`, geomgm_ifw_cartoon_fore_model.py): define_G(3, 3, ...) -- the
    generator's last layer is ReflectionPad(3) + Conv7x7(ngf -> 3) + tanh (networks.py:1277-1279) and nothing else changes.
    Against the oracle's forward on the same weights and batch, at the reduced width and at full width."""
    from animateportrait_amd import networks as N
    from animateportrait_amd.synthetic import make_generator_inputs, generator_args
    from oracle import generator as og
    args = generator_args(make_generator_inputs(2, seed=11))
    sd = og.init_params(og.generator_param_shapes(3, 3, ngf, 9, 3, 3), seed=11)
    G = N.define_G(3, 3, ngf, 'resnet_9blocks_rcatland32_full_ifw', 'instance', False, 'normal', 0.02, [0], div=3, disp=3)
    G.load_state_dict(sd, strict=True)
    with torch.no_grad():
        y = G(*[a.to(dev) for a in args])
        ref = og.generator_forward(sd, *args, div=3, disp=3)
    assert y.shape == (2, 3, 256, 256)
    err = linf(y, ref)
    print('output_nc=3 ngf=%d generator L-inf vs oracle: %.3e' % (ngf, err))
    assert err < 1e-3


def test_static_generator(dev, golden):
    """resnet_style2_9blocks (networks.py:573-637) on the HIP path against the reference's
    outputs; cat[f1, style] is a two-segment source of model.0, never a tensor."""
    from animateportrait_amd import networks as N
    from oracle import generator as og, static_generator as osg
    gd = golden('static_gen.npz')
    for tag, ngf, tol in (('ngf8', 8, 1e-4), ('ngf64', 64, 1e-3)):
        size = int(gd['size_' + tag])
        x = torch.rand(2, 3, size, size, generator=torch.Generator().manual_seed(int(gd['seed_' + tag]))) * 2 - 1
        sd = og.init_params(osg.static_param_shapes(3, 1, ngf), seed=4321)
        assert sd_sha(sd) == str(gd['weights_sha256_' + tag])
        G = N.define_G(3, 1, ngf, 'resnet_style2_9blocks', 'instance', use_dropout=False, gpu_ids=[0])
        G.load_state_dict(sd, strict=True)
        style = osg.style_code(2, size // 4).to(dev)
        y = G(x.to(dev), style)
        y1 = G(x[:1].to(dev), style[:1])
        err = linf(y, gd['y_' + tag])
        print('static generator %s L-inf vs reference: %.3e' % (tag, err))
        assert y.shape == (2, 1, size, size) and err < tol
        assert torch.equal(y1, y[:1])


def test_resize_and_grid_sample(dev):
    """ap_resize_bilinear / ap_grid_sample == F.interpolate(bilinear, align_corners=False) / F.grid_sample(bilinear,
    zeros), the image-level ops of geomcgt_ifw_test_model.py:282-285, 294."""
    from animateportrait_amd import ops
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 3, 37, 53, generator=g)
    for size in ((74, 106), (512, 512), (19, 26), (37, 53), (40, 20)):
        ref = F.interpolate(x, size=size, mode='bilinear', align_corners=False)
        assert linf(ops.resize_bilinear(x.to(dev), size), ref) < 1e-5, size     # fp32 source-index rounding
    grid = torch.rand(2, 29, 31, 2, generator=g) * 2.4 - 1.2           # some samples fall outside
    for ac in (True, False):
        ref = F.grid_sample(x, grid, mode='bilinear', padding_mode='zeros', align_corners=ac)
        assert linf(ops.grid_sample(x.to(dev), grid.to(dev), align_corners=ac), ref) < 2e-5, ac   # fp32 coordinates


def test_motion_grid_rasteriser(dev, golden):
    """ap_motion_grid (host Delaunay + device rasterisation) against the reference's
    cal_motion256 (scipy griddata, fp64): the grid agrees to fp32 rounding of the barycentric weights, batched."""
    from animateportrait_amd.data.motion import cal_motion256
    gd = golden('motion.npz')
    lm0 = np.stack([gd['lm0_%d' % i].numpy() for i in range(2)])
    lm = np.stack([gd['lm_%d' % i].numpy() for i in range(2)])
    got = cal_motion256(lm0, lm, device=dev)
    assert got.shape == (2, 256, 256, 2) and got.is_cuda
    for i in range(2):
        assert linf(got[i], gd['motion_%d' % i]) < 2e-5          # 2.5e-3 px
    one = cal_motion256(lm0[1], lm[1], device=dev)
    assert torch.equal(one[0], got[1])
    # a clip: ONE source landmark set broadcast over the frames (zero-stride view), as the clip streamer passes it
    clip = cal_motion256(torch.from_numpy(lm0[1]).unsqueeze(0).expand(2, -1, -1).numpy(), np.stack([lm[1], lm[1]]), device=dev)
    assert torch.equal(clip[0], got[1]) and torch.equal(clip[1], got[1])
    ident = cal_motion256(lm[0], lm[0], device=dev)              # identical landmarks: the identity grid
    ax = torch.arange(256., device=dev) / 127.5 - 1
    assert linf(ident[0, :, :, 0], ax.view(1, 256).expand(256, 256)) < 1e-5
    assert linf(ident[0, :, :, 1], ax.view(256, 1).expand(256, 256)) < 1e-5


def test_streaming_inference_model(dev):
    """GeomCGTIFWTestModel (geomcgt_ifw_test_model.py:254-302, 'drawing' branch): masked photo -> hot-path generator,
    static drawing at 512^2 (cached per photo), mask warped by the motion grid, blend -- against the oracle
    composition with the same seeded weights."""
    from animateportrait_amd.options.base_options import TestOptions
    from animateportrait_amd.models import create_model
    from animateportrait_amd.synthetic import make_generator_inputs
    from oracle import generator as og, static_generator as osg
    import contextlib
    import io
    opt = TestOptions().parse(['--model', 'geomcgt_ifw_test', '--netG', 'resnet_9blocks_rcatland32_full_ifw',
                               '--dataset_mode', 'synthetic', '--name', 'drawing_test', '--output_nc', '1', '--ngf', '8',
                               '--netg_resb_div', '3', '--netg_resb_disp', '3', '--gpu_ids', '0'])
    with contextlib.redirect_stdout(io.StringIO()):
        model = create_model(opt)
    sd_g = og.init_params(og.generator_param_shapes(3, 1, 8, 9, 3, 3), seed=1234)
    sd_s = og.init_params(osg.static_param_shapes(3, 1, 64), seed=4321)
    model.netG_A.load_state_dict(sd_g, strict=True)
    model.net_staticG.load_state_dict(sd_s, strict=True)
    n = 2
    d = make_generator_inputs(n, seed=21)
    gen = torch.Generator().manual_seed(5)
    yy, xx = torch.meshgrid(torch.arange(256.), torch.arange(256.), indexing='ij')
    matte = ((((yy - 128) / 90) ** 2 + ((xx - 120) / 70) ** 2) < 1).float().view(1, 1, 256, 256).repeat(n, 1, 1, 1)
    matte = (matte * 0.9 + torch.rand(n, 1, 256, 256, generator=gen) * 0.05).contiguous()
    batch = {'A': d['input'], 'warp_motion': d['motion'], 'A_lm': d['land1'], 'tB_lm': d['land2'],
             'iw_flow': d['flow'], 'if_mask': d['ifmask'], 'matte': matte}
    model.set_input(batch)
    model.test()
    with torch.no_grad():
        static = osg.static_drawing(sd_s, d['input'])
        fake, fore, mask1, masked = osg.streaming_forward(
            lambda *a: og.generator_forward(sd_g, *a, div=3, disp=3), d['input'], matte, static, d['land1'], d['land2'],
            d['motion'], d['flow'], d['ifmask'])
    assert linf(model.fakeB_static, static) < 1e-3
    assert linf(model.real_A, masked) < 1e-6
    assert linf(model.mask1, mask1) < 1e-5
    assert linf(model.fake_B_fore, fore) < 1e-3
    assert linf(model.fake_B, fake) < 1e-3
    # the static drawing is cached per photo: the next frame of the same clip (same photo tensor) does not recompute it
    calls = []
    orig = model.net_staticG.forward
    model.net_staticG.forward = lambda *a: (calls.append(1), orig(*a))[1]
    model.set_input(batch)
    model.test()
    assert not calls and linf(model.fake_B, fake) < 1e-3
    batch2 = dict(batch, A=batch['A'].clone())
    model.set_input(batch2)
    model.test()
    assert len(calls) == 1


def test_patchgan(dev, golden):
    from animateportrait_amd import networks as N
    from oracle import generator as og, discriminator as od
    gd = golden('patchgan.npz')
    for cin in (1, 2):
        x = torch.rand(2, cin, 256, 256, generator=torch.Generator().manual_seed(900 + cin)) * 2 - 1
        for ndf, tol in ((8, 5e-5), (64, 2e-4)):
            D = N.define_D(cin, ndf, 'basic', 3, 'instance', 'normal', 0.02, [0])
            D.load_state_dict(og.init_params(od.patchgan_param_shapes(cin, ndf), seed=4321 + cin), strict=True)
            with torch.no_grad():
                y = D(x.to(dev) if ndf == 8 else x[:1].to(dev))
            assert y.shape[1:] == (1, 30, 30)
            assert linf(y, gd['y%d_c%d' % (ndf, cin)]) < tol, (cin, ndf)


CONV_CASES = [
    # cin segs, cout, k, stride, pad, mode, transposed, H, W
    ([5], 7, 3, 1, 1, 'zero', False, 19, 45),
    ([6, 3], 40, 3, 1, 1, 'reflect', False, 33, 31),
    ([8, 16, 8], 130, 3, 1, 1, 'zero', False, 12, 70),
    ([3], 64, 7, 1, 3, 'reflect', False, 40, 40),
    ([16], 1, 7, 1, 3, 'reflect', False, 20, 50),
    ([10, 6], 3, 7, 1, 3, 'reflect', False, 70, 33),
    ([5], 2, 7, 1, 3, 'zero', False, 16, 130),
    ([12], 20, 3, 2, 1, 'zero', False, 37, 41),
    ([1], 8, 3, 1, 1, 'zero', False, 40, 70),          # landmark encoder: narrow layers on the vector-ALU kernel
    ([8], 16, 3, 2, 1, 'zero', False, 37, 41),
    ([16], 16, 3, 2, 1, 'zero', False, 64, 64),
    ([5], 8, 3, 1, 1, 'reflect', False, 9, 33),
    ([2], 64, 4, 2, 1, 'zero', False, 64, 64),
    ([24], 96, 4, 2, 1, 'zero', False, 30, 34),
    ([16], 48, 4, 1, 1, 'zero', False, 32, 32),
    ([32], 1, 4, 1, 1, 'zero', False, 31, 31),
    ([96], 1, 4, 1, 1, 'zero', False, 31, 31),         # PatchGAN output layer: half-wave row kernel (conv_head.h)
    ([70], 1, 4, 1, 1, 'zero', False, 45, 23),
    ([16], 24, 3, 2, 1, 'zero', True, 9, 21),
    ([10], 12, 4, 2, 1, 'zero', True, 15, 16),
    ([24], 2, 4, 2, 1, 'zero', True, 17, 45),          # few-output transposed 4x4 (D first-layer data gradient): conv_tsmall.h
    ([64], 1, 4, 2, 1, 'zero', True, 32, 32),
    ([9], 3, 4, 2, 1, 'zero', True, 8, 33),
]


@pytest.mark.parametrize('case', CONV_CASES)
def test_conv_sweep_vs_oracle(dev, case):
    """Ragged sizes, multi-source inputs with fused producer IN+act, every kernel family."""
    from animateportrait_amd import ops
    segs, cout, k, stride, pad, mode, transposed, H, W = case
    g = torch.Generator().manual_seed(sum(map(ord, str(case))))
    cin = sum(segs)
    n = 2
    xs = [torch.randn(n, c, H, W, generator=g) * 2 + 0.5 for c in segs]
    w = torch.randn((cin, cout, k, k) if transposed else (cout, cin, k, k), generator=g) * 0.1
    b = torch.randn(cout, generator=g)
    feats, refs = [], []
    for i, x in enumerate(xs):
        if i % 2 == 0:   # virtual source: IN + activation fused into the loader
            act = ops.ACT_RELU if i == 0 else ops.ACT_LRELU
            m = x.mean((2, 3)).reshape(-1)
            r = 1.0 / torch.sqrt(x.var((2, 3), unbiased=False).reshape(-1) + 1e-5)
            feats.append(ops.Feat(x.to(dev), m.to(dev), r.to(dev), act))
            xn = F.instance_norm(x)
            refs.append(F.relu(xn) if act == ops.ACT_RELU else F.leaky_relu(xn, 0.2))
        else:
            feats.append(ops.Feat(x.to(dev)))
            refs.append(x)
    xr = torch.cat(refs, 1)
    if transposed:
        ref = F.conv_transpose2d(xr, w, b, stride=2, padding=pad, output_padding=1 if k == 3 else 0)
    elif mode == 'reflect':
        ref = F.conv2d(F.pad(xr, (pad,) * 4, mode='reflect'), w, b, stride=stride)
    else:
        ref = F.conv2d(xr, w, b, stride=stride, padding=pad)
    layer = _layer(dev, w, b, segs=segs, stride=stride, pad=pad,
                   pad_mode=ops.PAD_REFLECT if mode == 'reflect' else ops.PAD_ZERO, transposed=transposed,
                   output_padding=(1 if k == 3 else 0) if transposed else 0)
    y = layer.run(feats, act=ops.ACT_LRELU)
    scale = float(ref.abs().max())
    assert y.data.shape == ref.shape
    tol = 5e-5 if ops.stem_rows_eligible(layer.spec) else 2e-5       # 7x7 stems run on the split-bf16 path
    assert linf(y.data, F.leaky_relu(ref, 0.2)) < tol * max(scale, 1.0)
    # statistics epilogue: IN of the bias-free output
    yn = layer.run(feats, norm_act=ops.ACT_NONE)
    refn = F.instance_norm(ref)
    assert linf(ops.materialize(yn).data if (ref.shape[2] * ref.shape[3]) % 4 == 0 else
                (yn.data - yn.mean.view(n, cout, 1, 1)) * yn.rstd.view(n, cout, 1, 1), refn) < 1e-4


# ------------------------------------------------------------------------------------ backward
BWD_CASES = [
    # cin segs, cout, k, stride, pad, mode, transposed, H, W
    ([6, 3], 40, 3, 1, 1, 'reflect', False, 33, 31),
    ([8, 16, 8], 130, 3, 1, 1, 'zero', False, 12, 70),
    ([3], 64, 7, 1, 3, 'reflect', False, 40, 40),
    ([16], 1, 7, 1, 3, 'reflect', False, 20, 50),      # last layer of the generator: wgrad_final.h
    ([24], 1, 7, 1, 3, 'zero', False, 33, 64),
    ([12], 20, 3, 2, 1, 'zero', False, 36, 40),
    ([2], 64, 4, 2, 1, 'zero', False, 64, 64),         # 1..2 input channels: streaming weight gradient (wgrad_narrow.h)
    ([1], 64, 4, 2, 1, 'zero', False, 36, 40),
    ([1], 20, 4, 2, 1, 'zero', False, 128, 128),       # ... the LDS-staged form (power-of-two rows), 4 rows per iteration
    ([2], 10, 4, 2, 1, 'zero', False, 24, 256),        # ... one row per iteration, partial cout group
    ([1], 8, 3, 1, 1, 'zero', False, 40, 70),
    ([16], 48, 4, 1, 1, 'zero', False, 32, 32),
    ([32], 1, 4, 1, 1, 'zero', False, 31, 31),
    ([96], 1, 4, 1, 1, 'zero', False, 31, 31),
    ([70], 1, 4, 1, 1, 'zero', False, 32, 23),
    ([16], 24, 3, 2, 1, 'zero', True, 9, 21),
    # reflection-padded 3x3 on the split-bf16 path, padded gradient 32 m + 2 columns wide: main launch + transposed strip
    ([64], 64, 3, 1, 1, 'reflect', False, 32, 32),
    ([48, 16], 96, 3, 1, 1, 'reflect', False, 20, 64),
]


@pytest.mark.parametrize('case', BWD_CASES)
@pytest.mark.parametrize('norm', [True, False])
def test_conv_backward_vs_autograd(dev, case, norm):
    """dgrad / wgrad / IN-backward / bias-grad of one layer against torch.autograd on the CPU oracle ops."""
    from animateportrait_amd import ops
    from animateportrait_amd.autograd import Tape, conv_forward
    segs, cout, k, stride, pad, mode, transposed, H, W = case
    g = torch.Generator().manual_seed(sum(map(ord, str(case))) + int(norm))
    cin = sum(segs)
    n = 2
    xs = [(torch.randn(n, c, H, W, generator=g) * 1.5 + 0.3).requires_grad_(True) for c in segs]
    w = (torch.randn((cin, cout, k, k) if transposed else (cout, cin, k, k), generator=g) * 0.1).requires_grad_(True)
    b = torch.randn(cout, generator=g).requires_grad_(True)
    xr = torch.cat(xs, 1)
    if transposed:
        ref = F.conv_transpose2d(xr, w, b, stride=2, padding=pad, output_padding=1 if k == 3 else 0)
    elif mode == 'reflect':
        ref = F.conv2d(F.pad(xr, (pad,) * 4, mode='reflect'), w, b, stride=stride)
    else:
        ref = F.conv2d(xr, w, b, stride=stride, padding=pad)
    ref = F.relu(F.instance_norm(ref)) if norm else F.leaky_relu(ref, 0.2)
    up = torch.randn(ref.shape, generator=g)
    (ref * up).sum().backward()

    layer = _layer(dev, w.detach(), b.detach(), segs=segs, stride=stride, pad=pad,
                   pad_mode=ops.PAD_REFLECT if mode == 'reflect' else ops.PAD_ZERO, transposed=transposed,
                   output_padding=(1 if k == 3 else 0) if transposed else 0)
    tape = Tape()
    feats = [tape.track(ops.Feat(x.detach().to(dev))) for x in xs]
    out = conv_forward(tape, layer, feats, norm_act=ops.ACT_RELU if norm else None,
                       act=ops.ACT_NONE if norm else ops.ACT_LRELU)
    # the consumer of a virtual output sees act(IN(y)): feed the upstream gradient w.r.t. that
    tape.add(out, up.to(dev), 0)
    tape.backward()
    gw = tape.param_grads[layer.weight]
    assert linf(gw, w.grad) <= 2e-4 * float(w.grad.abs().max()) + 1e-5
    gb = tape.param_grads[layer.bias]
    if norm:
        assert float(gb.abs().max()) == 0.0 and float(b.grad.abs().max()) < 1e-3
    else:
        assert linf(gb, b.grad) <= 2e-4 * float(b.grad.abs().max()) + 1e-5
    for f, x in zip(feats, xs):
        g1, p1, g2 = ops._split_contribs(tape.take(f))
        gx = ops.fold_add(g1, p1, g2) if (p1 or g2 is not None) else g1
        assert linf(gx, x.grad) <= 2e-4 * float(x.grad.abs().max()) + 1e-5


@pytest.mark.parametrize('case', [
    # cin segs, cout, k, pad, mode, H, W, n
    ([64], 64, 3, 1, 'reflect', 32, 32, 2),
    ([32, 16, 16], 96, 3, 1, 'zero', 21, 45, 3),        # ragged: odd rows, partial column tile, 3 segments
    ([256], 256, 3, 1, 'reflect', 64, 64, 2),
    ([64], 128, 4, 1, 'zero', 32, 32, 2),               # PatchGAN 4x4 stride 1 (output 31 x 31)
    ([40], 48, 3, 1, 'zero', 40, 40, 1),                # channel counts that are not multiples of 64
    ([40, 24, 8], 80, 3, 1, 'zero', 19, 64, 2),         # padded-row operand kernel: 3 segments, odd rows, partial group
    ([32], 64, 3, 1, 'reflect', 10, 128, 1),            # ... two rows per workgroup
    ([32], 48, 3, 1, 'reflect', 5, 256, 1),             # ... one row per workgroup
    ([3], 64, 7, 3, 'reflect', 64, 64, 2),              # 7x7 stem: with APAMD_ROWS_WGRAD=1 in plain-bf16 arithmetic the row form (1 x 7 taps over 21 row channels)
    ([4], 48, 7, 3, 'reflect', 21, 45, 1),              # ... ragged: odd rows, partial column tile, 48 outputs
    ([9], 64, 7, 3, 'zero', 32, 40, 1),                 # ... 63 of the tile's 64 row channels, zero padding
    ([3], 32, 7, 3, 'reflect', 40, 40, 2),              # ... 32 outputs (the generator's half-width stem): half a tile
])
def test_wgrad_bf16x3(dev, case, monkeypatch):
    """Weight gradient on the bf16 matrix pipe (split operands) against the fp64 gradient, beside the exact-fp32
    kernel on the same data; the input is a virtual (IN + ReLU) feature for the first segment."""
    from animateportrait_amd import ops
    segs, cout, k, pad, mode, H, W, n = case
    g = torch.Generator().manual_seed(sum(map(ord, str(case))))
    cin = sum(segs)
    xs = [torch.randn(n, c, H, W, generator=g) * 1.5 + 0.3 for c in segs]
    m0 = xs[0].mean((2, 3)).reshape(-1)
    r0 = 1.0 / torch.sqrt(xs[0].var((2, 3), unbiased=False).reshape(-1) + 1e-5)
    feats = [ops.Feat(xs[0].to(dev), m0.to(dev), r0.to(dev), ops.ACT_RELU)] + [ops.Feat(x.to(dev)) for x in xs[1:]]
    xr = torch.cat([F.relu(F.instance_norm(xs[0]))] + xs[1:], 1).double()
    w = torch.zeros(cout, cin, k, k, dtype=torch.float64, requires_grad=True)
    xp = F.pad(xr, (pad,) * 4, mode='reflect') if mode == 'reflect' else F.pad(xr, (pad,) * 4)
    y = F.conv2d(xp, w)
    up = torch.randn(y.shape, generator=g)
    (y * up.double()).sum().backward()
    ref = w.grad
    pm = ops.PAD_REFLECT if mode == 'reflect' else ops.PAD_ZERO
    scale = float(ref.abs().max())
    got = {}
    for prec in (ops.PRECISION_BF16X3, ops.PRECISION_FP32):
        got[prec] = ops.wgrad(k, 1, pad, pm, ops.Feat(up.to(dev)), feats, (cout, cin, k, k), precision=prec)
    assert linf(got[ops.PRECISION_FP32], ref) < 5e-6 * scale
    assert linf(got[ops.PRECISION_BF16X3], ref) < 5e-5 * scale, linf(got[ops.PRECISION_BF16X3], ref) / scale
    if k == 7:
        # the stems' row form (opt-in, plain-bf16 arithmetic only: one product per tap): the fp64 sum of bf16-rounded operands
        monkeypatch.setenv('APAMD_ROWS_WGRAD', '1')
        r16 = lambda t: t.float().bfloat16().double()
        w16 = torch.zeros(cout, cin, k, k, dtype=torch.float64, requires_grad=True)
        xp16 = F.pad(r16(xr), (pad,) * 4, mode='reflect') if mode == 'reflect' else F.pad(r16(xr), (pad,) * 4)
        (F.conv2d(xp16, w16) * r16(up)).sum().backward()
        # (a plain source: act(IN(.)) evaluated on the device may round an element to the neighbouring bf16)
        got16 = ops.wgrad(k, 1, pad, pm, ops.Feat(up.to(dev)), [ops.Feat(xr.float().to(dev))], (cout, cin, k, k),
                          precision=ops.PRECISION_BF16)
        assert linf(got16, w16.grad) < 3e-5 * float(w16.grad.abs().max())
    # ... and with the shifted operand re-tiled from the forward pass's split copies (ap_wgrad_desc.src_xs: every segment a
    # multiple of 8 channels), which the sources carry once a split-bf16 convolution has staged them
    if all(c % 8 == 0 for c in segs) and k != 7:
        for f in feats:
            ops.presplit(f, ops.PRECISION_BF16X3)
        again = ops.wgrad(k, 1, pad, pm, ops.Feat(up.to(dev)), feats, (cout, cin, k, k), precision=ops.PRECISION_BF16X3)
        assert linf(again, ref) < 5e-5 * scale, linf(again, ref) / scale
        # ... and with BOTH operands read as split copies by the kernel itself (ap_conv2d_wgrad_xs: 3x3 layers, transposing LDS reads)
        if k in (3, 4) and cout % 8 == 0:
            gf = ops.Feat(up.to(dev))
            ops.presplit(gf, ops.PRECISION_BF16X3)
            for prec, tol in ((ops.PRECISION_BF16X3, 5e-5), (ops.PRECISION_BF16, None)):
                if k == 4 and prec == ops.PRECISION_BF16:
                    continue              # (the 4x4 form exists for split bf16 only)
                direct = ops.wgrad(k, 1, pad, pm, gf, feats, (cout, cin, k, k), precision=prec, g_xs=gf.xs)
                if tol is not None:
                    assert linf(direct, ref) < tol * scale, linf(direct, ref) / scale
                else:           # plain bf16: the same products as the prepared-operand kernel in that mode
                    same = ops.wgrad(k, 1, pad, pm, ops.Feat(up.to(dev)), feats, (cout, cin, k, k), precision=prec)
                    assert linf(direct, same) < 2e-5 * scale, linf(direct, same) / scale


@pytest.mark.parametrize('k', [3, 4])
def test_wgrad_stride2_operand_from_forward_copies(dev, k):
    """Stride-2 weight gradients run as 2 x 2 layers over the space-to-depth view; that view's operand comes from the fp32
    source, from the space-to-depth split copy the forward pass staged (ap_wgrad_desc.src_xs_s2d) or is gathered from the
    plain split copy (src_xs[0], where the forward pass ran the stride-2 kernel): all three against the fp64 gradient."""
    from animateportrait_amd import ops
    g = torch.Generator().manual_seed(40 + k)
    n, cin, cout, H, W = 2, 64, 128, 32, 48
    x = torch.randn(n, cin, H, W, generator=g) * 1.5 + 0.3
    m0 = x.mean((2, 3)).reshape(-1)
    r0 = 1.0 / torch.sqrt(x.var((2, 3), unbiased=False).reshape(-1) + 1e-5)
    w = torch.zeros(cout, cin, k, k, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(F.relu(F.instance_norm(x)).double(), w, stride=2, padding=1)
    up = torch.randn(y.shape, generator=g)
    (y * up.double()).sum().backward()
    ref, scale = w.grad, float(w.grad.abs().max())

    def feat():
        return ops.Feat(x.to(dev), m0.to(dev), r0.to(dev), ops.ACT_RELU)
    plain, with_xs, with_s2d = feat(), feat(), feat()
    ops.presplit(with_xs, ops.PRECISION_BF16X3)
    with_s2d.s2d = ops.presplit_s2d(with_s2d)
    for f in (plain, with_xs, with_s2d):
        got = ops.wgrad(k, 2, 1, ops.PAD_ZERO, ops.Feat(up.to(dev)), [f], (cout, cin, k, k), precision=ops.PRECISION_BF16X3)
        assert linf(got, ref) < 5e-5 * scale, linf(got, ref) / scale
    # ... and with both operands read as split copies by the kernel (ap_conv2d_wgrad_xs on the space-to-depth copy)
    gf = ops.Feat(up.to(dev))
    ops.presplit(gf, ops.PRECISION_BF16X3)
    for f in (with_s2d, with_xs):          # (from the space-to-depth copy; from the plain copy: the view gathered inside the kernel)
        got = ops.wgrad(k, 2, 1, ops.PAD_ZERO, gf, [f], (cout, cin, k, k), precision=ops.PRECISION_BF16X3, g_xs=gf.xs)
        assert linf(got, ref) < 5e-5 * scale, linf(got, ref) / scale


@pytest.mark.parametrize('shape,act,two,pad', [((2, 5, 40, 36), 1, True, 0), ((2, 3, 128, 128), 2, False, 0),
                                                ((1, 3, 256, 256), 1, True, 0), ((1, 2, 200, 256), 0, False, 0),
                                                ((1, 2, 300, 300), 1, True, 0), ((2, 3, 64, 64), 1, True, 1),
                                                ((1, 2, 30, 30), 1, False, 1), ((1, 2, 128, 128), 2, True, 1),
                                                ((1, 2, 256, 256), 1, True, 1), ((1, 2, 256, 256), 0, False, 3),
                                                ((1, 2, 40, 44), 1, True, 3)])
def test_instnorm_backward_all_plane_sizes(dev, shape, act, two, pad):
    """ap_instnorm_bwd against autograd through act(instance_norm(y)) [and ReflectionPad2d(1) when the incoming
    gradient is a padded convolution's]: the register-resident kernels (planes up to 64^2 and 128^2; 16-byte-lane and
    scalar fold readers), the 256^2 kernel that parks half of the plane in LDS, and the reduce / apply pair beyond."""
    from animateportrait_amd import ops
    n, c, h, w = shape
    g = torch.Generator().manual_seed(sum(shape) + act + pad)
    y = (torch.randn(shape, generator=g, dtype=torch.float64) * 1.3 + 0.4).requires_grad_(True)
    xh = F.instance_norm(y)
    out = xh if act == 0 else (F.relu(xh) if act == 1 else F.leaky_relu(xh, 0.2))
    ga, gb = torch.randn(n, c, h + 2 * pad, w + 2 * pad, generator=g), torch.randn(shape, generator=g)
    outp = F.pad(out, (pad,) * 4, mode='reflect') if pad else out
    ((outp * ga.double()).sum() + ((out * gb.double()).sum() if two else 0.0)).backward()
    yf = y.detach().float()
    m = yf.double().mean((2, 3)).reshape(-1).float()
    r = (1.0 / torch.sqrt(yf.double().var((2, 3), unbiased=False).reshape(-1) + 1e-5)).float()
    f = ops.Feat(yf.to(dev), m.to(dev), r.to(dev), act)
    dy = ops.instnorm_bwd([(ga.to(dev), pad)] + ([(gb.to(dev), 0)] if two else []), f)
    assert linf(dy, y.grad) < 2e-5 * float(y.grad.abs().max())


@pytest.mark.parametrize('shape,pad,act,two', [((2, 3, 64, 64), 1, 0, True), ((1, 2, 5, 8), 1, 2, True),
                                                ((1, 2, 3, 4), 1, 1, False), ((2, 2, 9, 10), 1, 3, True),
                                                ((1, 2, 12, 16), 3, 0, True), ((1, 3, 16, 16), 0, 2, True)])
def test_act_bwd_fold_forms(dev, shape, pad, act, two):
    """ap_act_bwd: dy = (fold(g1) + g2) * act'(out) against autograd through act(.) and ReflectionPad2d: the pad-1
    16-byte-lane kernel (incl. H = 3 / W = 4, where both border terms land on one row / one lane group), the general
    fold (pad 3, W % 4 != 0) and the unpadded form."""
    from animateportrait_amd import ops
    n, c, h, w = shape
    g = torch.Generator().manual_seed(h * 100 + w + act)
    pre = torch.randn(shape, generator=g, dtype=torch.float64).requires_grad_(True)
    out = pre if act == 0 else (F.relu(pre) if act == 1 else (F.leaky_relu(pre, 0.2) if act == 2 else torch.tanh(pre)))
    g1 = torch.randn(n, c, h + 2 * pad, w + 2 * pad, generator=g)
    g2 = torch.randn(shape, generator=g)
    padded = F.pad(out, (pad,) * 4, mode='reflect') if pad else out
    ((padded * g1.double()).sum() + ((out * g2.double()).sum() if two else 0.0)).backward()
    got = ops.act_bwd([(g1.to(dev), pad)] + ([(g2.to(dev), 0)] if two else []), out.detach().float().to(dev), act)
    assert linf(got, pre.grad) < 1e-5 * float(pre.grad.abs().max())


def test_warp_backward(dev):
    from animateportrait_amd import ops
    from animateportrait_amd.synthetic import make_generator_inputs
    from oracle import warp as ow
    d = make_generator_inputs(2, seed=9)
    for level, size, c in ((0, 256, 3), (2, 64, 9)):
        x = torch.randn(2, c, size, size, generator=torch.Generator().manual_seed(level)).requires_grad_(True)
        y = ow.double_feature_warping(x, d['motion'], d['flow'], d['ifmask'], level)
        up = torch.randn(y.shape, generator=torch.Generator().manual_seed(7))
        (y * up).sum().backward()
        gx = ops.warp_concat_bwd(up.to(dev), d['motion'].to(dev), d['flow'].to(dev), d['ifmask'].to(dev), level)
        diff = (gx.cpu() - x.grad).abs()
        assert float((diff > 1e-3).float().mean()) < 1e-4 and float(diff.mean()) < 1e-5
    # the accumulation's corner cases: a strongly compressing map (hundreds of pixels of a tile hit the same window
    # element: same-instruction conflicts, claim losers), a magnifying one (the window does not fit: direct scatter),
    # and every pixel sampling ONE point
    for name, scale in (('compress', 0.06), ('magnify', 3.0), ('point', 0.0)):
        motion = (d['motion'] * scale).contiguous()
        x = torch.randn(2, 10, 64, 64, generator=torch.Generator().manual_seed(3), dtype=torch.float64).requires_grad_(True)
        y = ow.double_feature_warping(x, motion.double(), d['flow'].double(), d['ifmask'].double(), 2)
        up = torch.randn(y.shape, generator=torch.Generator().manual_seed(8), dtype=torch.float64)
        (y * up).sum().backward()
        gx = ops.warp_concat_bwd(up.float().to(dev), motion.to(dev), d['flow'].to(dev), d['ifmask'].to(dev), 2)
        ref = x.grad
        # (fp32 sampling coordinates against the fp64 evaluation: 1e-4 of the maximum under 3x magnification)
        assert float((gx.cpu().double() - ref).abs().max()) < 2e-4 * float(ref.abs().max()), name


def test_generator_ngf8_grads(dev, golden):
    from animateportrait_amd import networks as N
    from animateportrait_amd.synthetic import make_generator_inputs, generator_args
    from oracle import generator as og
    gd = golden('gen_ngf8.npz')
    d = make_generator_inputs(2, seed=1234)
    sd = og.init_params(og.generator_param_shapes(3, 1, 8, 9, 3, 3), seed=1234)
    G = N.define_G(3, 1, 8, 'resnet_9blocks_rcatland32_full_ifw', 'instance', False, 'normal', 0.02, [0], div=3, disp=3)
    G.load_state_dict(sd, strict=True)
    y = G(*[a.to(dev) for a in generator_args(d)])
    assert y.requires_grad
    assert linf(y, gd['y_disp3']) < 1e-3
    up = torch.randn(y.shape, generator=torch.Generator().manual_seed(5))
    (y * up.to(dev)).sum().backward()
    names = list(sd.keys())
    grads = dict(G.named_parameters())
    # Accuracy bar: fp32 weight gradients of this net are intrinsically noisy (cancellation over 131k pixels
    # behind InstanceNorm).  The golden holds the reference evaluated in fp64 and the fp32 reference's own
    # relative L-inf distance to it; the HIP path must be as close to the fp64 truth as the reference is.
    noise = dict(zip(names, np.asarray(gd['grad32_relerr'], dtype=np.float64)))
    live = [k for k in names if k.endswith('.weight') or k in ('model_tri_merge.bias', 'model3.7.bias')]
    for k in names:
        if k not in live:     # bias in front of InstanceNorm: exact zero here, rounding noise in the reference
            assert float(grads[k].grad.abs().max()) == 0.0, k
    for k in gd:
        if k.startswith('grad64_model'):
            name = k[7:]
            t = gd[k].double()
            err = float((grads[name].grad.cpu().double() - t).abs().max() / t.abs().max())
            assert err <= 2.0 * noise[name] + 2e-5, (name, err, noise[name])
    norms = np.array([float(grads[k].grad.double().norm()) for k in names])
    ref = np.asarray(gd['grad64_norms'], dtype=np.float64)
    idx = [names.index(k) for k in live]
    assert np.allclose(norms[idx], ref[idx], rtol=2e-2)


def test_patchgan_grads(dev, golden):
    from animateportrait_amd import networks as N
    from oracle import generator as og, discriminator as od
    gd = golden('patchgan.npz')
    for cin in (1, 2):
        D = N.define_D(cin, 8, 'basic', 3, 'instance', 'normal', 0.02, [0])
        D.load_state_dict(og.init_params(od.patchgan_param_shapes(cin, 8), seed=4321 + cin), strict=True)
        x = (torch.rand(2, cin, 256, 256, generator=torch.Generator().manual_seed(900 + cin)) * 2 - 1).to(dev)
        x.requires_grad_(True)
        y = D(x)
        up = torch.randn(y.shape, generator=torch.Generator().manual_seed(6))
        (y * up.to(dev)).sum().backward()
        ref = gd['dx8_c%d' % cin]
        assert linf(x.grad, ref) <= 2e-3 * float(ref.abs().max()) + 1e-7
        for k, p in D.named_parameters():
            ref = gd['g8_c%d_%s' % (cin, k)]
            if k.endswith('bias') and k not in ('model.0.bias', 'model.11.bias'):
                assert float(p.grad.abs().max()) == 0.0
                continue
            assert linf(p.grad, ref) <= 3e-3 * float(ref.abs().max()) + 1e-5, k


# ------------------------------------------------------------------------------------ split-bf16 matrix path
BF3_CASES = [
    # cin segs, cout, mode, H, W
    ([64], 64, 'reflect', 32, 32),
    ([128, 16, 16], 96, 'zero', 20, 70),
    ([256], 256, 'reflect', 64, 64),
    ([64, 64, 64], 130, 'zero', 17, 33),
    ([48], 64, 'reflect', 33, 40),                 # odd chunk count: the pipeline pads with an all-zero chunk
    ([32, 16, 32], 70, 'zero', 40, 40),
]


@pytest.mark.parametrize('tall', [0, 1])
@pytest.mark.parametrize('case', BF3_CASES)
def test_conv_bf16x3_vs_oracle(dev, case, tall, monkeypatch):
    """Wide 3x3 layers on the bf16 matrix pipe (operands split into bf16 head + tail): fp32-class accuracy, and the
    exact-fp32 kernel on the same data for comparison.  tall = 1 forces the 16-row tiles of full batches; otherwise the
    plan picks 4-row tiles for these small problems."""
    from animateportrait_amd import ops
    from animateportrait_amd.networks import ConvLayer
    monkeypatch.setenv('APAMD_NO_SMALL_TILES', str(tall))
    segs, cout, mode, H, W = case
    g = torch.Generator().manual_seed(sum(map(ord, str(case))))
    n = 2
    xs = [torch.randn(n, c, H, W, generator=g) * 2 + 0.5 for c in segs]
    w = torch.randn(cout, sum(segs), 3, 3, generator=g) * 0.05
    b = torch.randn(cout, generator=g)
    feats, refs = [], []
    for i, x in enumerate(xs):
        if i % 2 == 0:
            m = x.mean((2, 3)).reshape(-1)
            r = 1.0 / torch.sqrt(x.var((2, 3), unbiased=False).reshape(-1) + 1e-5)
            feats.append(ops.Feat(x.to(dev), m.to(dev), r.to(dev), ops.ACT_RELU))
            refs.append(F.relu(F.instance_norm(x)))
        else:
            feats.append(ops.Feat(x.to(dev)))
            refs.append(x)
    xr = torch.cat(refs, 1).double()
    ref = (F.conv2d(F.pad(xr, (1,) * 4, mode='reflect'), w.double(), b.double()) if mode == 'reflect'
           else F.conv2d(xr, w.double(), b.double(), padding=1))
    scale = float(ref.abs().max())
    errs = {}
    for prec in (ops.PRECISION_BF16X3, ops.PRECISION_FP32):
        layer = ConvLayer(segs, cout, 3, 1, 1, ops.PAD_REFLECT if mode == 'reflect' else ops.PAD_ZERO).to(dev)
        layer.spec.precision = prec
        with torch.no_grad():
            layer.weight.copy_(w); layer.bias.copy_(b)
        y = layer.run(feats, act=ops.ACT_NONE)
        errs[prec] = linf(y.data, ref) / scale
        yn = layer.run(feats, norm_act=ops.ACT_NONE)          # statistics epilogue
        refn = F.instance_norm(ref.float())
        got = (yn.data - yn.mean.view(n, cout, 1, 1)) * yn.rstd.view(n, cout, 1, 1)
        assert linf(got, refn) < (2e-3 if prec == ops.PRECISION_BF16X3 else 1e-4)
    assert errs[ops.PRECISION_FP32] < 2e-6
    assert errs[ops.PRECISION_BF16X3] < 5e-5, errs     # ~2^-17 per product, averaged down by the K-sum


@pytest.mark.parametrize('case', [
    # cin, cout, mode, H, W
    (3, 64, 'reflect', 40, 40),
    (3, 32, 'reflect', 33, 70),
    (1, 48, 'zero', 16, 130),
    (4, 100, 'reflect', 21, 37),
])
def test_stem7x7_rows_bf16x3(dev, case):
    """7x7 stems (ReflectionPad2d(3) + Conv2d(input_nc, ., 7), networks.py:1218) as a 1x7 split-bf16 convolution over
    the row expansion of the input: fp32-class result, same statistics epilogue; the exact-fp32 kernel beside it."""
    from animateportrait_amd import ops
    from animateportrait_amd.networks import ConvLayer
    cin, cout, mode, H, W = case
    g = torch.Generator().manual_seed(sum(map(ord, str(case))))
    n = 2
    x = torch.randn(n, cin, H, W, generator=g) * 1.5 + 0.2
    w = torch.randn(cout, cin, 7, 7, generator=g) * 0.05
    b = torch.randn(cout, generator=g)
    xd = x.double()
    ref = (F.conv2d(F.pad(xd, (3,) * 4, mode='reflect'), w.double(), b.double()) if mode == 'reflect'
           else F.conv2d(xd, w.double(), b.double(), padding=3))
    scale = float(ref.abs().max())
    for prec, tol in ((ops.PRECISION_BF16X3, 5e-5), (ops.PRECISION_FP32, 2e-6)):
        layer = ConvLayer([cin], cout, 7, 1, 3, ops.PAD_REFLECT if mode == 'reflect' else ops.PAD_ZERO).to(dev)
        layer.spec.precision = prec
        with torch.no_grad():
            layer.weight.copy_(w); layer.bias.copy_(b)
        assert ops.stem_rows_eligible(layer.spec) == (prec == ops.PRECISION_BF16X3)
        src = ops.Feat(x.to(dev))
        y = layer.run(src, act=ops.ACT_NONE)
        assert y.data.shape == ref.shape
        assert linf(y.data, ref) / scale < tol, (prec, linf(y.data, ref) / scale)
        yn = layer.run(src, norm_act=ops.ACT_RELU)
        got = (yn.data - yn.mean.view(n, cout, 1, 1)) * yn.rstd.view(n, cout, 1, 1)
        assert linf(got, F.instance_norm(ref.float())) < (2e-3 if prec == ops.PRECISION_BF16X3 else 1e-4)
        if prec == ops.PRECISION_BF16X3:
            assert len(src.xs_rows) == 1          # one expansion shared by both runs


@pytest.mark.parametrize('case', [
    # cin, cout, H, W, virtual source
    (64, 128, 64, 64, True),
    (32, 48, 36, 70, False),
    (128, 130, 30, 34, True),
    (40, 64, 2, 66, True),
])
def test_conv4x4s2_space_to_depth_bf16x3(dev, case):
    """PatchGAN body layers (Conv2d(c, 2c, 4, stride 2, pad 1), networks.py:2620-2636) as a 2x2 stride-1 split-bf16
    convolution over the space-to-depth copy of the input: fp32-class result; the exact-fp32 kernel beside it."""
    from animateportrait_amd import ops
    from animateportrait_amd.networks import ConvLayer
    cin, cout, H, W, virt = case
    g = torch.Generator().manual_seed(sum(map(ord, str(case))))
    n = 2
    x = torch.randn(n, cin, H, W, generator=g) * 1.5 + 0.2
    w = torch.randn(cout, cin, 4, 4, generator=g) * 0.05
    b = torch.randn(cout, generator=g)
    if virt:
        m = x.mean((2, 3)).reshape(-1)
        r = 1.0 / torch.sqrt(x.var((2, 3), unbiased=False).reshape(-1) + 1e-5)
        src = ops.Feat(x.to(dev), m.to(dev), r.to(dev), ops.ACT_LRELU)
        xd = F.leaky_relu(F.instance_norm(x), 0.2).double()
    else:
        src = ops.Feat(x.to(dev))
        xd = x.double()
    ref = F.conv2d(xd, w.double(), b.double(), stride=2, padding=1)
    scale = float(ref.abs().max())
    for prec, tol in ((ops.PRECISION_BF16X3, 5e-5), (ops.PRECISION_FP32, 2e-6)):
        layer = ConvLayer([cin], cout, 4, 2, 1, ops.PAD_ZERO).to(dev)
        layer.spec.precision = prec
        with torch.no_grad():
            layer.weight.copy_(w); layer.bias.copy_(b)
        assert ops.s2d_eligible(layer.spec, H, W) == (prec == ops.PRECISION_BF16X3)
        y = layer.run(src, act=ops.ACT_LRELU)
        assert y.data.shape == ref.shape
        assert linf(y.data, F.leaky_relu(ref, 0.2)) / scale < tol, (prec, linf(y.data, F.leaky_relu(ref, 0.2)) / scale)
        yn = layer.run(src, norm_act=ops.ACT_RELU)
        got = (yn.data - yn.mean.view(n, cout, 1, 1)) * yn.rstd.view(n, cout, 1, 1)
        assert linf(got, F.instance_norm(ref.float())) < (2e-3 if prec == ops.PRECISION_BF16X3 else 1e-4)


@pytest.mark.parametrize('tall', [0, 1])
@pytest.mark.parametrize('blocks', [1, 7, 24])
def test_conv_bf16x3_persistent_walk(dev, blocks, tall, monkeypatch):
    """The split-bf16 kernel's workgroups are persistent: each walks several (image, pixel tile, cout tile) entries
    with the LDS stages of consecutive tiles overlapped.  Force small grids (also ones that are not a multiple of
    the 8 XCDs) and compare bit-for-bit with the default launch of the same layer -- for the 16-row tiles of full
    batches (tall) and for the 4-row tiles the plan picks when the tile list would leave most CUs idle."""
    from animateportrait_amd import ops
    from animateportrait_amd.networks import ConvLayer
    monkeypatch.setenv('APAMD_NO_SMALL_TILES', str(tall))
    g = torch.Generator().manual_seed(77 + blocks)
    n, H, W = 3, 50, 70
    segs, cout = [64, 48], 136
    feats = [ops.Feat((torch.randn(n, c, H, W, generator=g) * 2).to(dev)) for c in segs]
    layer = ConvLayer(segs, cout, 3, 1, 1, ops.PAD_REFLECT).to(dev)
    layer.spec.precision = ops.PRECISION_BF16X3
    with torch.no_grad():
        layer.weight.copy_(torch.randn(layer.weight.shape, generator=g) * 0.05)
    monkeypatch.delenv('APAMD_BF3_BLOCKS', raising=False)
    want = layer.run(feats, norm_act=ops.ACT_NONE)
    monkeypatch.setenv('APAMD_BF3_BLOCKS', str(blocks))
    got = layer.run(feats, norm_act=ops.ACT_NONE)
    assert torch.equal(got.data, want.data)
    assert torch.equal(got.mean, want.mean) and torch.equal(got.rstd, want.rstd)
    xr = torch.cat([f.data for f in feats], 1).double().cpu()
    ref = F.conv2d(F.pad(xr, (1,) * 4, mode='reflect'), layer.weight.detach().double().cpu())
    gotn = (got.data - got.mean.view(n, cout, 1, 1)) * got.rstd.view(n, cout, 1, 1)
    assert linf(gotn, F.instance_norm(ref.float())) < 2e-3


@pytest.mark.parametrize('case', [
    # cin, cout, k, stride, transposed, H, W
    (64, 96, 4, 1, False, 33, 31),               # PatchGAN 4x4 stride-1 layers (32-cout tiles)
    (256, 512, 4, 1, False, 32, 32),
    (48, 64, 3, 2, False, 30, 66),
    (80, 64, 3, 2, True, 16, 32),
    (64, 128, 3, 2, False, 64, 64),
    (128, 96, 3, 2, False, 38, 70),
    (256, 128, 3, 2, True, 16, 32),
    (64, 64, 4, 2, True, 20, 24),
    (64, 48, 3, 2, True, 13, 21),                # conv_ph4: partial cout tile, phase grid not a multiple of the 8 x 32 tile
    (96, 80, 4, 2, True, 9, 37),
])
def test_conv_bf16x3_strided_and_transposed(dev, case):
    """Stride-2 3x3 and ConvTranspose2d (as sub-pixel phases) on the split-bf16 path, virtual (IN+ReLU) source."""
    from animateportrait_amd import ops
    from animateportrait_amd.networks import ConvLayer
    cin, cout, k, stride, transposed, H, W = case
    g = torch.Generator().manual_seed(sum(map(ord, str(case))))
    n = 2
    x = torch.randn(n, cin, H, W, generator=g) * 2 + 0.5
    w = torch.randn((cin, cout, k, k) if transposed else (cout, cin, k, k), generator=g) * 0.05
    b = torch.randn(cout, generator=g)
    m = x.mean((2, 3)).reshape(-1)
    r = 1.0 / torch.sqrt(x.var((2, 3), unbiased=False).reshape(-1) + 1e-5)
    feat = ops.Feat(x.to(dev), m.to(dev), r.to(dev), ops.ACT_RELU)
    xr = F.relu(F.instance_norm(x)).double()
    op = 1 if k == 3 else 0
    ref = (F.conv_transpose2d(xr, w.double(), b.double(), stride=2, padding=1, output_padding=op) if transposed
           else F.conv2d(xr, w.double(), b.double(), stride=stride, padding=1))
    scale = float(ref.abs().max())
    for prec, tol in ((ops.PRECISION_BF16X3, 5e-5), (ops.PRECISION_FP32, 2e-6)):
        layer = ConvLayer([cin], cout, k, stride, 1, ops.PAD_ZERO, transposed, op if transposed else 0).to(dev)
        layer.spec.precision = prec
        with torch.no_grad():
            layer.weight.copy_(w); layer.bias.copy_(b)
        y = layer.run(feat, act=ops.ACT_NONE)
        assert y.data.shape == ref.shape
        assert linf(y.data, ref) / scale < tol, (prec, linf(y.data, ref) / scale)
        yn = layer.run(feat, norm_act=ops.ACT_NONE)
        got = (yn.data - yn.mean.view(n, cout, 1, 1)) * yn.rstd.view(n, cout, 1, 1)
        assert linf(got, F.instance_norm(ref.float())) < (2e-3 if prec == ops.PRECISION_BF16X3 else 1e-4)


@pytest.mark.parametrize('precision', ['bf16x3', 'fp32'])
def test_instnorm_ill_conditioned_planes(dev, precision, monkeypatch):
    """ADVICE r1 (instnorm.hip): a plane whose |mean| is hundreds of standard deviations -- what a PatchGAN sees on a
    mostly-white masked crop (base_model.py:245-247) -- must still be normalised like F.instance_norm: the statistics
    from the conv epilogue's fp32 (sum, sum of squares) tiles are recomputed from the data for such planes, in both
    consumers (standalone finalize and the fused norm / split pass)."""
    from animateportrait_amd import ops
    from animateportrait_amd.networks import ConvLayer
    monkeypatch.setattr(ops, 'DEFAULT_PRECISION', ops.PRECISION_FP32 if precision == 'fp32' else ops.PRECISION_BF16X3)
    g = torch.Generator().manual_seed(77)
    n, cin, c, h, w = 2, 32, 64, 64, 64
    x = torch.ones(n, cin, h, w) + torch.randn(n, cin, h, w, generator=g) * 1e-3      # near-constant input planes
    x[:, :, 20:28, 30:40] += torch.randn(n, cin, 8, 10, generator=g) * 0.05            # a small textured box
    layer = ConvLayer([cin], c, 3, 1, 1, ops.PAD_REFLECT).to(dev)
    with torch.no_grad():
        layer.weight.copy_(torch.randn(layer.weight.shape, generator=g) * 0.05 + 0.02)
    src = ops.Feat(x.to(dev))
    a = layer.run(src, norm_act=ops.ACT_NONE)
    b = layer.run(src, norm_act=ops.ACT_NONE)
    raw = a.data.double().cpu()
    ratio = (raw.mean(dim=(2, 3)) ** 2 / raw.var(dim=(2, 3), unbiased=False)).min()
    assert float(ratio) > 100.0                                   # the case under test: |mean| > 10 std everywhere
    ref = F.instance_norm(raw)                                    # fp64 on the kernel's own conv output
    y_fin = (a.data - a.mean.view(n, c, 1, 1)) * a.rstd.view(n, c, 1, 1)              # standalone finalize (+ refine)
    assert linf(y_fin, ref) < 5e-4 * float(ref.abs().max())
    y_ns, _ = ops._norm_apply_split(b, None, want_y=True, want_xs=False)               # fused pass, inline recompute
    assert linf(y_ns, ref) < 5e-4 * float(ref.abs().max())
    assert linf(b.rstd, a.rstd) <= 1e-6 * float(a.rstd.abs().max())
    rstd_ref = 1.0 / torch.sqrt(raw.var(dim=(2, 3), unbiased=False) + 1e-5)
    assert float(((a.rstd.view(n, c).double().cpu() - rstd_ref) / rstd_ref).abs().max()) < 1e-4


def test_grid_sample_and_warp_acc_flow_reference_goldens(dev, golden):
    """SURVEY App. D G4 / G5 on the device: F.grid_sample(x, motion) with out-of-range grid points and
    warp_acc_flow(x, flow, mask) with flows of +-40 px (modules.py:596-625) are the two halves of the fused
    ap_warp_concat kernel at level 0 -- against outputs of the reference's own functions (ops_small.npz), through the
    fp32 and the split-bf16 outputs; the backward kernel scatters through the same taps."""
    from animateportrait_amd import ops
    gd = golden('ops_small.npz')
    x, grid, flow, mask = (gd[k].to(dev).contiguous() for k in ('gs_x', 'gs_grid', 'wf_flow', 'wf_mask'))
    assert float(flow.abs().max()) > 30.0
    out = ops.warp_concat(ops.Feat(x), grid, flow, mask, 0).data
    assert linf(out[:, :8], gd['gs_y']) < 2e-5 and linf(out[:, 8:], gd['wf_y']) < 2e-5
    ones = torch.ones_like(mask)
    assert linf(ops.warp_concat(ops.Feat(x), grid, flow, ones, 0).data[:, 8:], gd['wf_y_nomask']) < 2e-5
    both = ops.warp_concat(ops.Feat(x), grid, flow, mask, 0, emit_xs=True)
    val, _ = _decode_split(both.xs, 2, 16, 32, 32)
    assert float(((val - both.data).abs() - both.data.abs() * 2.0 ** -16).max()) <= 1e-30
    # backward through the same (out-of-frame) taps == autograd of the reference formulas
    gout = torch.randn(2, 16, 32, 32, generator=torch.Generator().manual_seed(4))
    dx = ops.warp_concat_bwd(gout.to(dev), grid, flow, mask, 0)
    xr = gd['gs_x'].clone().requires_grad_(True)
    from oracle import warp as ow
    ref = torch.cat([F.grid_sample(xr, gd['gs_grid'], mode='bilinear', padding_mode='zeros', align_corners=False),
                     ow.warp_acc_flow(xr, gd['wf_flow'], gd['wf_mask'])], 1)
    ref.backward(gout)
    assert linf(dx, xr.grad) < 1e-5


def test_degenerate_shapes_are_errors_not_crashes(dev):
    """Empty / ragged inputs are refused at the boundary (negative status + message), never launched."""
    from animateportrait_amd import networks as N, ops, losses
    G = N.define_G(3, 1, 8, 'resnet_9blocks_rcatland32_full_ifw', 'instance', False, 'normal', 0.02, [0], div=3, disp=3)
    z = lambda *s: torch.zeros(*s, device=dev)                                      # noqa: E731
    with torch.no_grad():
        with pytest.raises((RuntimeError, ValueError)):
            G(z(0, 3, 256, 256), z(0, 1, 256, 256), z(0, 1, 256, 256), z(0, 256, 256, 2), z(0, 2, 256, 256), z(0, 1, 256, 256))
        with pytest.raises((RuntimeError, ValueError)):                             # ragged: land maps of another batch size
            G(z(2, 3, 256, 256), z(1, 1, 256, 256), z(2, 1, 256, 256), z(2, 256, 256, 2), z(2, 2, 256, 256), z(2, 1, 256, 256))
        with pytest.raises((RuntimeError, ValueError)):                             # motion grid of the wrong size
            G(z(1, 3, 256, 256), z(1, 1, 256, 256), z(1, 1, 256, 256), z(1, 128, 128, 2), z(1, 2, 256, 256), z(1, 1, 256, 256))
    with pytest.raises(ValueError):
        ops.conv2d(ops.ConvSpec([8], 8, 3, 1, 1), [ops.Feat(z(1, 4, 16, 16))], None)   # channel mismatch
    with pytest.raises((RuntimeError, ValueError)):
        losses.l1_loss(z(2, 1, 8, 8), z(2, 1, 8, 4))
    with pytest.raises(RuntimeError):
        losses.kp_to_map(z(0, 68, 2))
    y = G(torch.rand(1, 3, 256, 256, device=dev), -torch.ones(1, 1, 256, 256, device=dev), -torch.ones(1, 1, 256, 256, device=dev),
          z(1, 256, 256, 2), z(1, 2, 256, 256), z(1, 1, 256, 256)).detach()        # the device still works afterwards
    assert bool(torch.isfinite(y).all())


def test_warp_writes_space_to_depth_split_layout(dev):
    """ap_warp_concat_fwd_ex(flags = 1): the split copy of the warped concat in the space-to-depth layout of its stride-2
    consumer (model_tri01 / model_tri12) == ap_split_prepass_s2d of the fp32 concat, byte for byte, zero ring included."""
    from animateportrait_amd import ops
    g = torch.Generator().manual_seed(21)
    n, c, s = 2, 16, 64
    for level in (0, 1):
        h = s >> level
        x = torch.randn(n, c, h, h, generator=g).to(dev)
        yy, xx = torch.meshgrid(torch.linspace(-1, 1, s), torch.linspace(-1, 1, s), indexing='ij')
        motion = (torch.stack([xx, yy], -1).unsqueeze(0).repeat(n, 1, 1, 1) + 0.05 * torch.randn(n, s, s, 2, generator=g)).to(dev)
        flow = (3.0 * torch.randn(n, 2, s, s, generator=g)).to(dev)
        ifmask = (torch.rand(n, 1, s, s, generator=g) > 0.3).float().to(dev)
        res = ops.warp_concat(ops.Feat(x), motion, flow, ifmask, level, emit_xs=True, keep_fp32=True, s2d=True)
        assert res.s2d is not None and tuple(res.s2d.shape) == (n, 8 * c, h // 2 + 1, h // 2 + 1)
        ref = ops.warp_concat(ops.Feat(x), motion, flow, ifmask, level, emit_xs=False)
        assert torch.equal(res.data, ref.data)
        want = ops.presplit_s2d(ops.Feat(ref.data))
        assert torch.equal(res.s2d.xs.cpu(), want.xs.cpu())


def test_batched_packer_equals_per_layer_packer(dev):
    """ap_conv2d_pack_entries / ap_conv2d_pack_run (one launch per optimiser for all layers) write the same packed images as
    ap_conv2d_pack_weights on contiguous operands: forward, data-gradient operands as strided views of the parameter (channel
    slice, transposed taps), the space-to-depth and row forms, transposed layers (four fused phases)."""
    from animateportrait_amd import ops
    from animateportrait_amd.networks import ConvLayer
    from animateportrait_amd.optim import FlatAdam
    from animateportrait_amd.autograd import _dgrad_spec
    torch.manual_seed(5)
    layers = [ConvLayer([64, 16, 16], 64, 3, 1, 1, ops.PAD_REFLECT), ConvLayer([64], 128, 3, 2, 1), ConvLayer([3], 64, 7, 1, 3, ops.PAD_REFLECT),
              ConvLayer([64], 128, 4, 2, 1), ConvLayer([128], 64, 3, 2, 1, transposed=True, output_padding=1), ConvLayer([64], 64, 4, 1, 1)]
    for l in layers:
        l.to(dev)
        torch.nn.init.normal_(l.weight, 0.0, 0.05)
    opt = FlatAdam([p for l in layers for p in l.parameters()], lr=1e-3)
    checks = []
    l0, l1, l2, l3, l4, l5 = layers
    checks.append((l0.packed(), l0.spec, l0.weight.detach()))
    c0 = 0
    for i, c in enumerate(l0.spec.cin_segments):                       # data gradients per input segment + the strip form
        spec, _ = _dgrad_spec(l0, c)
        w = l0.weight.detach()[:, c0:c0 + c]
        checks.append((l0.packed_dgrad(i, spec, w), spec, w.contiguous()))
        checks.append((l0.packed_dgrad((i, 'T'), spec, w.transpose(2, 3)), spec, w.transpose(2, 3).contiguous()))
        c0 += c
    checks.append((l1.packed_s2d(), l1.s2d_spec(), ops.s2d_weight(l1.weight.detach())))
    checks.append((l3.packed_s2d(), l3.s2d_spec(), ops.s2d_weight(l3.weight.detach())))
    checks.append((l2.packed_rows(), l2.rows_spec(), ops.stem_rows_weight(l2.weight.detach())))
    checks.append((l4.packed(), l4.spec, l4.weight.detach()))
    spec4, _ = _dgrad_spec(l4, 128)
    checks.append((l4.packed_dgrad(0, spec4, l4.weight.detach()), spec4, l4.weight.detach()))
    spec1, _ = _dgrad_spec(l1, 64)
    checks.append((l1.packed_dgrad(0, spec1, l1.weight.detach()), spec1, l1.weight.detach()))
    checks.append((l5.packed(), l5.spec, l5.weight.detach()))
    # the wide operators go through the table (narrow ones -- the data gradient towards a 16-channel segment -- are planned on
    # the fp32 kernels and keep their own packer)
    assert opt._packset.count >= 12
    assert all(l._slots[k].batched for l, k in ((l0, 'fwd'), (l0, ('dgrad', 0)), (l0, ('dgrad', (0, 'T'))), (l1, 's2d'),
                                                 (l3, 's2d'), (l2, 'rows'), (l4, 'fwd'), (l5, 'fwd')))
    for got, spec, dense in checks:
        assert torch.equal(got, ops.pack_weights(spec, dense.contiguous()))
    # an optimiser step invalidates every image; the next access rebuilds all of them with one launch
    before = l0.packed().clone()
    for p in opt._params:
        p.grad.normal_()
    opt.step()
    after = l0.packed()
    assert not torch.equal(before, after) and torch.equal(after, ops.pack_weights(l0.spec, l0.weight.detach()))
    assert torch.equal(l1.packed_s2d(), ops.pack_weights(l1.s2d_spec(), ops.s2d_weight(l1.weight.detach())))


def _octet_to_nchw(t, c, h, w):
    """[N, C/8, H*W, 8] (ap_conv2d_fwd_octet) -> NCHW."""
    n = t.shape[0]
    return t.view(n, c // 8, h, w, 8).permute(0, 1, 4, 2, 3).reshape(n, c, h, w)


@pytest.mark.parametrize('case', ['s2d_3x3', 'stem_rows', 's2d_ragged'])
def test_conv_channel_octet_output(dev, case):
    """ap_conv2d_fwd_octet: the layers in front of the three warps (3x3 stride-2 on the space-to-depth route, 7x7 stem in the
    row form) write y[n][C/8][H*W][8]; the values are the NCHW launch's accumulators bit for bit, the InstanceNorm statistics
    (summed in another order) agree to rounding, and ap_instnorm_finalize_octet's data pass reads the strided planes."""
    from animateportrait_amd import ops
    g = torch.Generator().manual_seed(31)
    if case == 'stem_rows':
        n, cin, cout, h, k, stride, pad, pm = 2, 3, 32, 64, 7, 1, 3, ops.PAD_REFLECT
    elif case == 's2d_ragged':
        n, cin, cout, h, k, stride, pad, pm = 1, 32, 72, 44, 3, 2, 1, ops.PAD_ZERO
    else:
        n, cin, cout, h, k, stride, pad, pm = 2, 64, 128, 64, 3, 2, 1, ops.PAD_ZERO
    w = torch.randn(cout, cin, k, k, generator=g) * 0.05
    l = _layer(dev, w, None, stride=stride, pad=pad, pad_mode=pm)
    x = (torch.randn(n, cin, h, h, generator=g) + 0.5).to(dev)
    ref = l.run([ops.Feat(x)], norm_act=ops.ACT_RELU)
    got = l.run([ops.Feat(x)], norm_act=ops.ACT_RELU, out_octet=True)
    assert got.oct is not None and got.data.stride(0) == 0 and tuple(got.shape) == tuple(ref.shape)
    ho = ref.shape[2]
    assert torch.equal(_octet_to_nchw(got.oct, cout, ho, ho), ref.data)
    assert float(((got.mean - ref.mean).abs() / (ref.mean.abs() + 1e-3)).max()) < 1e-5
    assert float(((got.rstd - ref.rstd).abs() / ref.rstd).max()) < 1e-5
    # the data pass of the finaliser (ill-conditioned planes): a large common offset makes every plane take it
    xb = (torch.randn(n, cin, h, h, generator=g) * 0.01 + 40.0).to(dev)
    wpos = w.abs()
    lp = _layer(dev, wpos, None, stride=stride, pad=pad, pad_mode=ops.PAD_REFLECT if k == 7 else ops.PAD_ZERO)
    refb = lp.run([ops.Feat(xb)], norm_act=ops.ACT_RELU)
    gotb = lp.run([ops.Feat(xb)], norm_act=ops.ACT_RELU, out_octet=True)
    assert float(((gotb.rstd - refb.rstd).abs() / refb.rstd).max()) < 1e-5
    # plain conv + bias + activation form
    l2 = _layer(dev, w, torch.randn(cout, generator=g), stride=stride, pad=pad, pad_mode=pm)
    r2 = l2.run([ops.Feat(x)], act=ops.ACT_LRELU)
    g2 = l2.run([ops.Feat(x)], act=ops.ACT_LRELU, out_octet=True)
    assert torch.equal(_octet_to_nchw(g2.oct, cout, ho, ho), r2.data)
    # a channel-octet feature has no NCHW tensor: every other reader refuses it
    with pytest.raises(RuntimeError):
        ops.materialize(got)


def test_conv_octet_falls_back_to_nchw_where_unsupported(dev):
    """out_octet is a request: a layer whose kernel has no octet epilogue (4x4 stride-1, fp32 plans) returns NCHW; the 3x3 stride-1
    split-bf16 kernel has one since round 6 (the inference trunk, test_trunk_raw_outputs_in_the_channel_octet_layout)."""
    from animateportrait_amd import ops
    g = torch.Generator().manual_seed(32)
    l = _layer(dev, torch.randn(64, 64, 4, 4, generator=g) * 0.05, None, stride=1, pad=1, pad_mode=ops.PAD_ZERO)
    x = torch.randn(1, 64, 32, 32, generator=g).to(dev)
    out = l.run([ops.Feat(x)], norm_act=ops.ACT_RELU, out_octet=True)
    assert out.oct is None and out.data.is_contiguous()
    l3 = _layer(dev, torch.randn(64, 64, 3, 3, generator=g) * 0.05, None, stride=1, pad=1, pad_mode=ops.PAD_REFLECT)
    out3 = l3.run([ops.Feat(x)], norm_act=ops.ACT_RELU, out_octet=True)
    ref3 = l3.run([ops.Feat(x)], norm_act=ops.ACT_RELU)
    assert out3.oct is not None and out3.oct.shape == (1, 8, 32 * 32, 8)
    assert torch.equal(out3.oct.permute(0, 1, 3, 2).reshape(1, 64, 32, 32), ref3.data)          # the same accumulators, another layout
    assert linf(out3.mean, ref3.mean) < 1e-6 and linf(out3.rstd, ref3.rstd) < 1e-5


@pytest.mark.parametrize('level', [0, 1, 2])
def test_warp_reads_channel_octet_input(dev, level):
    """ap_warp_concat_fwd_ex(flags bit 1): gathering 8 channels of a tap as 32 contiguous bytes gives the NCHW launch's
    output bit for bit -- fp32, split-only and space-to-depth split forms, with the producer's IN + ReLU applied per tap."""
    from animateportrait_amd import ops
    from animateportrait_amd.synthetic import make_generator_inputs
    d = make_generator_inputs(2, seed=11)
    mo, fl, mk = d['motion'].to(dev), d['flow'].to(dev), d['ifmask'].to(dev)
    s = mo.shape[1]
    h = s >> level
    c = 16
    x = (torch.randn(2, c, h, h, generator=torch.Generator().manual_seed(4)) * 3 + 1).to(dev)
    m = x.mean((2, 3)).reshape(-1)
    r = 1.0 / torch.sqrt(x.var((2, 3), unbiased=False).reshape(-1) + 1e-5)

    def feat(octet):
        f = ops.Feat(x, m, r, ops.ACT_RELU)
        if octet:
            f = ops.Feat(torch.empty(1, device=dev).expand(x.shape), m, r, ops.ACT_RELU)
            f.oct = x.view(2, c // 8, 8, h * h).permute(0, 1, 3, 2).contiguous()
        return f
    for kw in ({}, dict(emit_xs=True, keep_fp32=False), dict(emit_xs=True, keep_fp32=True, s2d=True)):
        a = ops.warp_concat(feat(False), mo, fl, mk, level, **kw)
        b = ops.warp_concat(feat(True), mo, fl, mk, level, **kw)
        def close(u, v):
            return torch.equal(u, v)
        if not a.is_split_only:
            assert close(a.data, b.data) and torch.equal(a.data == -1.0, b.data == -1.0)
        if a.xs is not None:
            (va, za), (vb, zb) = _decode_split(a.xs, 2, 2 * c, h, h), _decode_split(b.xs, 2, 2 * c, h, h)
            assert close(va, vb) and float(zb.abs().max()) == 0.0
        if a.s2d is not None:
            sh = tuple(a.s2d.shape)
            (va, za), (vb, zb) = _decode_split(a.s2d.xs, *sh), _decode_split(b.s2d.xs, *sh)
            assert close(va, vb) and float(zb.abs().max()) == 0.0 and torch.equal(va == 0, vb == 0)
    # a map whose size is not a multiple of 4 takes the one-lane-per-pixel octet path: bit-identical to NCHW
    x3 = torch.randn(1, 8, 3, 3, generator=torch.Generator().manual_seed(5)).to(dev)
    mo3 = (torch.rand(1, 3, 3, 2, generator=torch.Generator().manual_seed(6)) * 2 - 1).to(dev)
    fl3, mk3 = torch.zeros(1, 2, 3, 3, device=dev), torch.ones(1, 1, 3, 3, device=dev)
    fo = ops.Feat(torch.empty(1, device=dev).expand(x3.shape))
    fo.oct = x3.view(1, 1, 8, 9).permute(0, 1, 3, 2).contiguous()
    assert torch.equal(ops.warp_concat(ops.Feat(x3), mo3, fl3, mk3, 0).data, ops.warp_concat(fo, mo3, fl3, mk3, 0).data)


def test_warp_quad_gather_variant_is_bitwise_the_lane_gather(dev, monkeypatch):
    """APAMD_WARP_GATHER=quad (the quad-cooperative "wavefront-shuffle" gather BASELINE.json names; rejected on its measurement,
    profiles/r04_warp_variants.md, and kept for A/B runs) fetches the same taps through shared 64-byte requests and a DPP
    transpose: the same values in the same order of operations, so the output equals the default kernel's bit for bit --
    also with samples that leave the frame on every side."""
    from animateportrait_amd import ops
    from animateportrait_amd.synthetic import make_generator_inputs
    d = make_generator_inputs(2, seed=21)
    mo, fl, mk = d['motion'].clone(), d['flow'].clone(), d['ifmask']
    mo[0, :40] += 0.9                     # a band sampled far outside on the right / bottom
    mo[1, :, :30] -= 1.3                  # ... and on the left / top
    fl[:, :, 100:140] *= 30.0
    mo, fl, mk = mo.to(dev), fl.to(dev), mk.to(dev)
    g = torch.Generator().manual_seed(4)
    for level, c in ((0, 32), (1, 64), (2, 128)):
        h = 256 >> level
        x = torch.randn(2, c, h, h, generator=g)
        m = x.mean((2, 3)).reshape(-1).to(dev)
        r = (1.0 / torch.sqrt(x.var((2, 3), unbiased=False).reshape(-1) + 1e-5)).to(dev)
        xo = x.view(2, c // 8, 8, h * h).permute(0, 1, 3, 2).contiguous().to(dev)

        def run():
            f = ops.Feat(torch.empty(1, device=dev).expand(x.shape), m, r, ops.ACT_RELU)
            f.oct = xo
            return ops.warp_concat(f, mo, fl, mk, level).data
        monkeypatch.delenv('APAMD_WARP_GATHER', raising=False)
        lane = run()
        nchw = ops.warp_concat(ops.Feat(x.to(dev), m, r, ops.ACT_RELU), mo, fl, mk, level).data
        monkeypatch.setenv('APAMD_WARP_GATHER', 'quad')
        quad = run()
        monkeypatch.delenv('APAMD_WARP_GATHER', raising=False)
        assert torch.equal(lane, nchw), level
        assert torch.equal(quad, lane), (level, float((quad - lane).abs().max()))


def test_launches_on_different_streams_are_fenced(dev):
    """ops._stream(): a launch on another stream than the previous one waits for it (kernels of this
    library must not share compute units).  A chain of convolutions issued on stream A and consumed on stream B WITHOUT any wait
    by the caller must therefore give the serial result, bit for bit."""
    from animateportrait_amd import ops
    from animateportrait_amd.networks import ConvLayer
    torch.manual_seed(3)
    layers = [ConvLayer([64], 64, 3, 1, 1, ops.PAD_REFLECT, False, 0).to(dev) for _ in range(4)]
    for l in layers:                                     # (ConvLayer weights are torch.empty until init_net runs)
        torch.nn.init.normal_(l.weight, 0.0, 0.05)
    x = torch.randn(8, 64, 64, 64, device=dev)

    def chain(f, ls):
        for l in ls:
            f = l.run([f], norm_act=ops.ACT_RELU)
        return f
    ref = ops.materialize(chain(ops.Feat(x), layers)).data.clone()
    torch.cuda.synchronize()
    a, b = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    for _ in range(5):
        with torch.cuda.stream(a):
            mid = chain(ops.Feat(x), layers[:3])
        with torch.cuda.stream(b):                 # no wait_stream / event here: the package fences its own launches
            out = ops.materialize(chain(mid, layers[3:])).data
        torch.cuda.synchronize()
        assert torch.equal(out, ref)


def test_residual_stream_as_split_copies(dev):
    """Inference keeps the ResNet trunk's residual stream only as split copies (ops.materialize keep_fp32=False; the next block's
    residual add reads head + tail: ap_norm_apply_split_ex flags bit 2).  Three blocks chained that way against the same blocks
    with the fp32 stream: the split representation costs 2^-17 relative per block, nothing else."""
    from animateportrait_amd import ops
    from animateportrait_amd.networks import ResnetBlock
    torch.manual_seed(11)
    blocks = [ResnetBlock(64).to(dev) for _ in range(3)]
    for blk in blocks:                                   # (ConvLayer parameters are uninitialised until init_net runs)
        for p_ in blk.parameters():
            torch.nn.init.normal_(p_, 0.0, 0.05)
    x0 = torch.randn(3, 64, 40, 36, device=dev)

    def run(as_split):
        old = ops.RESIDUAL_AS_SPLIT
        ops.RESIDUAL_AS_SPLIT = as_split
        try:
            x = ops.Feat(x0.clone())
            for b in blocks:
                x = b.run(x, None)
            return x
        finally:
            ops.RESIDUAL_AS_SPLIT = old
    a, b = run(True), run(False)
    assert a.is_split_only and not b.is_split_only
    # compare through the split copies (what the next convolution stages): heads + tails back to fp32
    def unsplit(f):
        n, c, h, w = f.data.shape
        t = f.xs.view(torch.bfloat16).view(n, 2, c // 8, h * w + 1, 8)[:, :, :, :h * w].float()
        return (t[:, 0] + t[:, 1]).permute(0, 1, 3, 2).reshape(n, c, h, w)
    ya, yb = unsplit(a), unsplit(b)
    assert linf(yb, b.data) <= 2 ** -16 * float(b.data.abs().max())
    assert linf(ya, yb) <= 3e-5 * float(yb.abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize('case', [(3, 64, 128, 128, 2, 0), (2, 8, 64, 80, 1, 0), (2, 16, 66, 66, 2, 1), (1, 5, 70, 61, 3, 0)],
                         ids=lambda c: 'N%d C%d %dx%d act%d pad%d' % c)
def test_act_bwd_with_the_bias_gradient_in_one_pass(dev, case):
    """ap_act_bwd_bias: dy of a layer without InstanceNorm and db[c] = sum dy in one pass (the PatchGAN's first layer,
    networks.py:2620-2623: autograd's LeakyReLU backward + the bias gradient of the convolution in front of it)."""
    from animateportrait_amd import ops
    n, c, h, w, act, pad = case
    gen = torch.Generator().manual_seed(41 + sum(case))
    out = torch.randn(n, c, h, w, generator=gen)
    if act == 3:
        out = torch.tanh(out)
    g1 = torch.randn(n, c, h + 2 * pad, w + 2 * pad, generator=gen)
    g2 = torch.randn(n, c, h, w, generator=gen)
    contribs = [(g1.to(dev), pad), (g2.to(dev), 0)]
    dy_ref = ops.act_bwd(contribs, out.to(dev), act)
    dy, db = ops.act_bwd_bias(contribs, out.to(dev), act)
    assert torch.equal(dy, dy_ref)
    ref = dy_ref.double().sum((0, 2, 3))
    assert linf(db, ref) <= 2e-6 * float(dy_ref.double().abs().sum((0, 2, 3)).max())
    assert torch.equal(db, ops.act_bwd_bias(contribs, out.to(dev), act)[1])          # fixed summation order
