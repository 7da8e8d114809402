"""Host-side mirror of the reference's network registry for the hot path.

Same entry points, argument meaning and error behaviour as Module2/models/networks.py:
``define_G`` (:123-201), ``define_D`` (:204-247), ``init_weights`` (:71-102), ``get_scheduler``
(:42-68), ``GANLoss`` (:407-473); same ``state_dict`` keys as
``ResnetConditionTriGenerator32_full_ifw`` (:1190-1340) and ``NLayerDiscriminator`` (:2602-2647)
so reference checkpoints (``<epoch>_net_G_A.pth`` ...) load with ``strict=True``.

The modules own their parameters as ordinary ``nn.Parameter``s; ``forward`` never touches a
torch operator for the math -- every layer is a call into libapamd.so (HIP, gfx950).
"""
import functools

import torch
import torch.nn as nn
from torch.optim import lr_scheduler

from . import ops
from .autograd import (conv_forward, materialize_forward, warp_forward, batch_split_forward,
                       generator_apply, discriminator_apply)
from .ops import (Feat, ConvSpec, ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH, PAD_ZERO, PAD_REFLECT,
                  W_OIHW, W_IOHW)

GENERATOR_NAMES = ('resnet_9blocks_rcatland32_full_ifw', 'resnet_style2_9blocks')
# names the reference registry knows (networks.py:152-199) but that are outside this build's hot path
_REFERENCE_ONLY_G = (
    'resnet_9blocks', 'resnet_9blocks_rcatland', 'resnet_9blocks_rcatland3',
    'resnet_9blocks_rcatland32', 'resnet_10blocks_rcatland32', 'resnet_9blocks_rcatland4',
    'resnet_9blocks_rcatland32_fw', 'resnet_9blocks_rcatland32_fw2', 'resnet_9blocks_rcatland32_ifw',
    'resnet_9blocks_rcatland32_ifw_single2', 'resnet_9blocks_rcatland32_full_ifw_colorcoded',
    'resnet_9blocks_rcatland32_full_ifw2', 'resnet_9blocks_rcatland32_full_ifw_single',
    'resnet_9blocks_rcatland32_full_ifw_single2', 'resnet_9blocks_rcatland32_full_ifw_single3', 'regressor',
    'combiner', 'resnet_9blocks_rcatland2', 'resnet_6blocks', 'unet_128', 'unet_256')


class ConvLayer(nn.Module):
    """Parameters of one nn.Conv2d / nn.ConvTranspose2d plus the kernel-side spec.
    state_dict: ``weight`` (OIHW, or IOHW when transposed) and ``bias`` -- as the reference layer."""

    def __init__(self, cin_segments, cout, k, stride=1, pad=0, pad_mode=PAD_ZERO, transposed=False,
                 output_padding=0):
        super().__init__()
        cin = sum(cin_segments)
        shape = (cin, cout, k, k) if transposed else (cout, cin, k, k)
        self.weight = nn.Parameter(torch.empty(shape, dtype=torch.float32))
        self.bias = nn.Parameter(torch.zeros(cout, dtype=torch.float32))
        self.spec = ConvSpec(cin_segments, cout, k, stride, pad, pad_mode, transposed, output_padding,
                             W_IOHW if transposed else W_OIHW)
        self._slots = {}                   # operator variant -> ops.PackedSlot (forward, row / space-to-depth forms, data gradients)
        self._rows_spec = None
        self._s2d_spec = None

    def _packed(self, slot_id, spec, view):
        slot = ops.packed_slot(spec, self.weight, view, self._slots.get(slot_id))
        self._slots[slot_id] = slot
        return slot.buf

    def packed_dgrad(self, seg, spec, view):
        """Packed weights of the data-gradient operator for input segment ``seg``; ``view``: the operand as a (strided)
        view of this layer's parameter (a channel slice, transposed taps): no contiguous copy is made for the batched packer."""
        return self._packed(('dgrad', seg), spec, ops.WeightView(view))

    def packed(self):
        return self._packed('fwd', self.spec, ops.WeightView(self.weight.detach()))

    def run(self, srcs, norm_act=None, act=ACT_NONE, out_octet=False, out_bf16=False):
        """norm_act=None: plain conv + bias + act.  norm_act=ACT_*: conv followed by InstanceNorm
        (bias skipped -- it cancels exactly under the mean subtraction) and that activation,
        both deferred to the consumer.  out_octet: see ops.conv2d (the output is read by the warp kernel only)."""
        if not isinstance(srcs, (list, tuple)):
            srcs = [srcs]
        spec, packed = self.spec, None
        if norm_act is None and ops.conv_d0_ok(spec, srcs, act):
            # the PatchGAN's first layer in plain-bf16 arithmetic: an output stream on the bf16 matrix pipe (csrc/conv_d0.h)
            return ops.conv_d0(srcs[0], self.weight, self.bias.detach(), act)
        if ops.stem_rows_eligible(spec) and not srcs[0].is_split_only:
            # 7x7 stem on <= 4 channels: 1x7 split-bf16 convolution over the row expansion of the input
            spec, packed = self.rows_spec(), self.packed_rows()
            srcs = [ops.presplit_rows(srcs[0], self.spec.k, self.spec.pad, self.spec.pad_mode)]
        elif (srcs[0].s2d is not None or not srcs[0].is_split_only) and ops.s2d_eligible(spec, *srcs[0].data.shape[2:]):
            # 4x4 stride-2 PatchGAN layer / 3x3 stride-2 encoder layer: 2x2 split-bf16 convolution over the space-to-depth
            # copy of the input -- made here, or already written by the producer (the warp kernel, ops.warp_concat s2d=True)
            spec, packed = self.s2d_spec(), self.packed_s2d()
            if srcs[0].s2d is None:
                srcs[0].s2d = ops.presplit_s2d(srcs[0])      # (kept on the source: the weight gradient re-tiles its operand from it)
            srcs = [srcs[0].s2d]
        if packed is None:
            packed = self.packed()
        if norm_act is None:
            return ops.conv2d(spec, srcs, packed, self.bias.detach(), act=act, out_octet=out_octet)
        return ops.conv2d(spec, srcs, packed, None, want_stats=True, out_act=norm_act, out_octet=out_octet,
                          out_bf16=out_bf16 and spec is self.spec)

    def stages_split(self, shape):
        """Whether this layer reads a source of ``shape`` (N, C, H, W) as its split-bf16 copy (then the producer may
        leave out the fp32 tensor in inference: ops.materialize keep_fp32=False)."""
        n, _, h, w = shape
        if ops.stem_rows_eligible(self.spec) or ops.s2d_eligible(self.spec, h, w):
            return False
        return ops.takes_split(self.spec, n, h, w)

    def s2d_spec(self):
        if self._s2d_spec is None:
            self._s2d_spec = ops.s2d_spec(self.spec)
        return self._s2d_spec

    def packed_s2d(self):
        return self._packed('s2d', self.s2d_spec(), ops.WeightView(self.weight.detach(), s2d_c=self.spec.cin_segments[0]))

    def rows_spec(self):
        if self._rows_spec is None:
            self._rows_spec = ops.stem_rows_spec(self.spec)
        return self._rows_spec

    def packed_rows(self):
        return self._packed('rows', self.rows_spec(), ops.WeightView(self.weight.detach(), rows_c=self.spec.cin_segments[0]))


def _seq(**children):
    """Container whose children are registered under the numeric names of the reference's nn.Sequential."""
    return nn.ModuleDict({k.lstrip('_'): v for k, v in children.items()})


class ResnetBlock(nn.Module):
    """networks.py:2303-2361 (reflect padding, no dropout): x + IN(conv(ReLU(IN(conv(x)))))."""

    def __init__(self, dim):
        super().__init__()
        self.conv_block = _seq(_1=ConvLayer([dim], dim, 3, 1, 1, PAD_REFLECT),
                               _5=ConvLayer([dim], dim, 3, 1, 1, PAD_REFLECT))

    def run(self, x, tape=None, consumer=None):
        """consumer: the layer that reads the block's output when it is not another block of the trunk (the first
        up-convolution) -- the output is kept as fp32 unless that layer stages split copies."""
        c1, c5 = self.conv_block['1'], self.conv_block['5']
        # (raw16: c1's raw output is read by c5's split pass, its own InstanceNorm backward and c5's weight gradient; c5's by the
        # residual pass and its InstanceNorm backward -- all of which read bf16: plain-bf16 training stores them as bf16)
        # inference: the raw outputs leave in the channel-octet layout where their one reader is a split-only norm pass (ops.trunk_octet_ok)
        dim = c1.spec.cout
        keep = consumer is not None and not consumer.stages_split(x.data.shape)
        y = conv_forward(tape, c1, x, norm_act=ACT_RELU, raw16=True, out_octet=tape is None and ops.trunk_octet_ok(dim))
        y = conv_forward(tape, c5, y, norm_act=ACT_NONE, raw16=True,
                         out_octet=tape is None and ops.trunk_octet_ok(dim, residual=x, keep_fp32=keep))
        return materialize_forward(tape, y, residual=x, consumer=consumer)


class ResnetBlock2(nn.Module):
    """networks.py:2363-2421: main branch reflect-padded, shortcut conv zero-padded, both on cat[x,l1,l2]."""

    def __init__(self, segs, dim_out):
        super().__init__()
        self.conv_block = _seq(_1=ConvLayer(segs, dim_out, 3, 1, 1, PAD_REFLECT),
                               _5=ConvLayer([dim_out], dim_out, 3, 1, 1, PAD_REFLECT))
        self.shortcut = _seq(_0=ConvLayer(segs, dim_out, 3, 1, 1, PAD_ZERO))

    def run(self, srcs, tape=None, consumer=None):
        c1, c5, sc = self.conv_block['1'], self.conv_block['5'], self.shortcut['0']
        y = conv_forward(tape, c1, srcs, norm_act=ACT_RELU, raw16=True, out_octet=tape is None and ops.trunk_octet_ok(c1.spec.cout))
        y = conv_forward(tape, c5, y, norm_act=ACT_NONE, raw16=True)
        s = conv_forward(tape, sc, srcs, norm_act=ACT_NONE)            # (the shortcut's raw output is read as a normalised RESIDUAL: fp32)
        return materialize_forward(tape, y, residual=s, consumer=consumer)


class ResnetConditionTriGenerator32_full_ifw(nn.Module):
    """networks.py:1190-1340.  ``norm_layer`` must be instance norm (the only one the model uses,
    geomgm_ifw_fore_model.py:161-209 / base_options.py norm default)."""

    def __init__(self, input_nc, output_nc, ngf=64, norm='instance', use_dropout=False, n_blocks=9,
                 padding_type='reflect', div=3, disp=1):
        super().__init__()
        if norm != 'instance':
            raise NotImplementedError('normalization layer [%s] is not available on the HIP path' % norm)
        if use_dropout:
            raise NotImplementedError('dropout is not available on the HIP path (the model sets no_dropout)')
        if padding_type != 'reflect':
            raise NotImplementedError('padding [%s] is not implemented' % padding_type)
        assert n_blocks >= 0
        self.n_blocks, self.div, self.disp = n_blocks, div, disp
        self.input_nc, self.output_nc, self.ngf = input_nc, output_nc, ngf
        h = ngf // 2
        con_dim = 16
        dim = ngf * 4
        # registration order == reference state_dict order (model_tri_merge is assigned first, :1251)
        self.model_tri_merge = ConvLayer([ngf * 4, ngf * 4, ngf * 4], dim, 3, 1, 1)
        self.model_tri00 = _seq(_1=ConvLayer([input_nc], h, 7, 1, 3, PAD_REFLECT))
        self.model_tri01 = _seq(_0=ConvLayer([ngf], ngf * 2, 3, 2, 1))
        self.model_tri02 = _seq(_0=ConvLayer([ngf * 2], ngf * 4, 3, 2, 1))
        self.model_tri10 = _seq(_1=ConvLayer([input_nc], ngf, 7, 1, 3, PAD_REFLECT))
        self.model_tri11 = _seq(_0=ConvLayer([ngf], ngf, 3, 2, 1))
        self.model_tri12 = _seq(_0=ConvLayer([ngf * 2], ngf * 4, 3, 2, 1))
        self.model_tri20 = _seq(_1=ConvLayer([input_nc], ngf, 7, 1, 3, PAD_REFLECT))
        self.model_tri21 = _seq(_0=ConvLayer([ngf], ngf * 2, 3, 2, 1))
        self.model_tri22 = _seq(_0=ConvLayer([ngf * 2], ngf * 2, 3, 2, 1))
        blocks = {}
        for i in range(n_blocks):
            if (i + disp) % div == 0:
                blocks[str(i)] = ResnetBlock2([dim, con_dim, con_dim], dim)
            else:
                blocks[str(i)] = ResnetBlock(dim)
        self.model2 = nn.ModuleDict(blocks)
        self.model3 = _seq(_0=ConvLayer([ngf * 4], ngf * 2, 3, 2, 1, transposed=True, output_padding=1),
                           _3=ConvLayer([ngf * 2], ngf, 3, 2, 1, transposed=True, output_padding=1),
                           _7=ConvLayer([ngf], output_nc, 7, 1, 3, PAD_REFLECT))
        self.model_landmark_trans = _seq(_0=ConvLayer([1], 8, 3, 1, 1), _3=ConvLayer([8], con_dim, 3, 2, 1),
                                         _6=ConvLayer([con_dim], con_dim, 3, 2, 1))
        self.land1_cache_key = None      # set by a streaming caller: identity of the (constant) land1 tensor, see _run
        self._land1_cache = None

    def is_block2(self, i):
        return (i + self.disp) % self.div == 0

    def double_feature_warping(self, x, motion, flow, ifmask, level, tape=None, consumer=None):
        return warp_forward(tape, x, motion, flow, ifmask, level, consumer=consumer)

    def forward(self, input, land1, land2, motion, flow, ifmask):
        """G(input, land1, land2, motion, flow, ifmask) -> (B, output_nc, S, S)   (networks.py:1315)."""
        if torch.is_grad_enabled() and (input.requires_grad or any(p.requires_grad for p in self.parameters())):
            return generator_apply(self, input, land1, land2, motion, flow, ifmask)
        return self.forward_inference(input, land1, land2, motion, flow, ifmask)

    def forward_inference(self, input, land1, land2, motion, flow, ifmask):
        return self._run(None, False, input, land1, land2, motion, flow, ifmask).data

    def _run(self, tape, input_needs_grad, input, land1, land2, motion, flow, ifmask):
        """The layer schedule.  tape=None: inference; otherwise every step also records its backward."""
        b = input.shape[0]
        inp = Feat(input.contiguous())
        if tape is not None and input_needs_grad:
            tape.track(inp)
        self._last_input_feat = inp if tape is not None else None
        motion, flow, ifmask = motion.contiguous(), flow.contiguous(), ifmask.contiguous()
        cf, dfw = conv_forward, self.double_feature_warping
        # inference: the encoder layers in front of the three warps write the channel-octet layout the warp kernel gathers
        # best (ops.conv2d out_octet); with a tape their outputs stay NCHW for the backward kernels
        oct = tape is None

        def branch1():
            x = cf(tape, self.model_tri00['1'], inp, norm_act=ACT_RELU, out_octet=oct)
            x = dfw(x, motion, flow, ifmask, 0, tape, self.model_tri01['0'])
            x = cf(tape, self.model_tri01['0'], x, norm_act=ACT_RELU)
            return cf(tape, self.model_tri02['0'], x, norm_act=ACT_RELU)

        def branch2():
            x = cf(tape, self.model_tri10['1'], inp, norm_act=ACT_RELU)
            x = cf(tape, self.model_tri11['0'], x, norm_act=ACT_RELU, out_octet=oct)
            x = dfw(x, motion, flow, ifmask, 1, tape, self.model_tri12['0'])
            return cf(tape, self.model_tri12['0'], x, norm_act=ACT_RELU)

        def branch3():
            x = cf(tape, self.model_tri20['1'], inp, norm_act=ACT_RELU)
            x = cf(tape, self.model_tri21['0'], x, norm_act=ACT_RELU)
            x = cf(tape, self.model_tri22['0'], x, norm_act=ACT_RELU, out_octet=oct)
            return dfw(x, motion, flow, ifmask, 2, tape, self.model_tri_merge)

        def landmarks():
            lt = self.model_landmark_trans
            key = self.land1_cache_key
            if tape is None and key is not None:
                # streaming inference: land1 is the photo's landmark map, the same for every frame of a clip -- the caller
                # (GeomCGTIFWTestModel) names it with land1_cache_key and its encoding (networks.py:1331-1332) is reused;
                # only land2 runs through the encoder.  Never on by default: a cached result must not enter a timed step.
                full = (key, tuple(land1.shape), tuple(ops.weight_key(lt[k].weight) for k in ('0', '3', '6')))
                if self._land1_cache is None or self._land1_cache[0] != full:
                    l = cf(None, lt['0'], Feat(land1.contiguous()), norm_act=ACT_RELU)
                    l = cf(None, lt['3'], l, norm_act=ACT_RELU)
                    l = cf(None, lt['6'], l, norm_act=ACT_NONE)
                    l.mean                                           # finalise the statistics once
                    self._land1_cache = (full, l)
                la = self._land1_cache[1]
                lb = cf(None, lt['0'], Feat(land2.contiguous()), norm_act=ACT_RELU)
                lb = cf(None, lt['3'], lb, norm_act=ACT_RELU)
                lb = cf(None, lt['6'], lb, norm_act=ACT_NONE)
                return la, lb
            # land1 / land2 share the encoder weights: one pass over the 2B batch
            lands = Feat(torch.cat([land1, land2], 0).contiguous())
            l = cf(tape, lt['0'], lands, norm_act=ACT_RELU)
            l = cf(tape, lt['3'], l, norm_act=ACT_RELU)
            l = cf(tape, lt['6'], l, norm_act=ACT_NONE)
            return batch_split_forward(tape, l, b)

        # ONE stream: the three branches and the landmark encoder are independent until the merge convolution, but they
        # must not run on side streams -- measured in round 3 (tools/conc_warp.py): a warp kernel that
        # shares compute units with one of the matrix kernels of another stream reads wrong data in lanes 48-63.
        x1, x2, x3 = branch1(), branch2(), branch3()
        l1, l2 = landmarks()
        x = cf(tape, self.model_tri_merge, [x1, x2, x3])
        for i in range(self.n_blocks):
            blk = self.model2[str(i)]
            nxt = self.model3['0'] if i == self.n_blocks - 1 else None
            x = blk.run([x, l1, l2], tape, consumer=nxt) if self.is_block2(i) else blk.run(x, tape, consumer=nxt)
        x = cf(tape, self.model3['0'], x, norm_act=ACT_RELU)
        x = cf(tape, self.model3['3'], x, norm_act=ACT_RELU)
        return cf(tape, self.model3['7'], x, act=ACT_TANH)


class ResnetStyle2Generator(nn.Module):
    """networks.py:573-637 (``resnet_style2_9blocks``): the static drawing generator of the streaming-inference
    model (geomcgt_ifw_test_model.py:225-227, 280-285).  Same ``state_dict`` keys as the reference
    (``model0.{1,4,7}``, ``model.0``, ``model.{3..11}.conv_block.{1,5}``, ``model.{12,15,19}``).  The reference keeps it
    frozen (``.eval()``, loaded from ``checkpoints/static/drawing.pth``), so only the forward pass is built."""

    def __init__(self, input_nc, output_nc, ngf=64, norm='instance', use_dropout=False, n_blocks=6,
                 padding_type='reflect', extra_channel=3, model0_res=0):
        super().__init__()
        if norm != 'instance':
            raise NotImplementedError('normalization layer [%s] is not available on the HIP path' % norm)
        if use_dropout:
            raise NotImplementedError('dropout is not available on the HIP path')
        if padding_type != 'reflect':
            raise NotImplementedError('padding [%s] is not implemented' % padding_type)
        if model0_res != 0:
            raise NotImplementedError('model0_res != 0 is not used by any shipped configuration')
        assert n_blocks >= 0
        self.n_blocks = n_blocks
        dim = ngf * 4
        self.model0 = _seq(_1=ConvLayer([input_nc], ngf, 7, 1, 3, PAD_REFLECT),
                           _4=ConvLayer([ngf], ngf * 2, 3, 2, 1), _7=ConvLayer([ngf * 2], dim, 3, 2, 1))
        layers = {'0': ConvLayer([dim, extra_channel], dim, 3, 1, 1)}
        for i in range(n_blocks):
            layers[str(3 + i)] = ResnetBlock(dim)
        j = 3 + n_blocks
        layers[str(j)] = ConvLayer([dim], dim // 2, 3, 2, 1, transposed=True, output_padding=1)
        layers[str(j + 3)] = ConvLayer([dim // 2], dim // 4, 3, 2, 1, transposed=True, output_padding=1)
        layers[str(j + 7)] = ConvLayer([ngf], output_nc, 7, 1, 3, PAD_REFLECT)
        self.model = nn.ModuleDict(layers)

    def forward(self, input1, input2):
        """G(input1, input2) -> (B, output_nc, S, S): f1 = model0(input1); model(cat[f1, input2]) (networks.py:632)."""
        with torch.no_grad():
            cf = conv_forward
            x = cf(None, self.model0['1'], Feat(input1.contiguous()), norm_act=ACT_RELU)
            x = cf(None, self.model0['4'], x, norm_act=ACT_RELU)
            x = cf(None, self.model0['7'], x, norm_act=ACT_RELU)
            x = cf(None, self.model['0'], [x, Feat(input2.contiguous())], norm_act=ACT_RELU)
            x = materialize_forward(None, x)
            j = 3 + self.n_blocks
            for i in range(self.n_blocks):
                x = self.model[str(3 + i)].run(x, None, consumer=self.model[str(j)] if i == self.n_blocks - 1 else None)
            x = cf(None, self.model[str(j)], x, norm_act=ACT_RELU)
            x = cf(None, self.model[str(j + 3)], x, norm_act=ACT_RELU)
            return cf(None, self.model[str(j + 7)], x, act=ACT_TANH).data


# --------------------------------------------------------------------------- Photo2Cartoon (static cartoon generator)
class P2CConv(ConvLayer):
    """One nn.Conv2d of Module2/models/photo2cartoon.py: as ConvLayer, but most of that file's convolutions have no bias
    (then ``bias`` is not a state_dict key), and every one of them goes through ops.conv2d as it is; the instance norm +
    activation of its source is fused into its loads by the Feat it is handed.

    Arithmetic: exact fp32 whatever the package's default precision.  The generator is some 130 normalised layers deep, and
    an operand error of 2^-17 injected early is amplified past the 1e-3 budget on the way: measured at ngf 32, 256 x 256
    against float64, L-inf 2.7e-3 with the split-bf16 kernels where they apply (1.1e-3 with only the 7x7 stem in fp32) and
    2.5e-4 in fp32 -- what stock fp32 operators give (2.4e-4).  The forward takes 10.5 ms either way: it is bound by its
    several hundred launches, not by the matrix pipe, and runs once per photo."""

    def __init__(self, cin, cout, k, stride=1, pad=0, pad_mode=PAD_ZERO, bias=False):
        super().__init__([cin], cout, k, stride, pad, pad_mode)
        self.spec.precision = ops.PRECISION_FP32
        nn.init.normal_(self.weight.data, 0.0, 0.02)
        if not bias:
            self.register_parameter('bias', None)

    def run(self, src, norm_act=None, act=ACT_NONE):
        """norm_act=None: act(conv [+ bias]), a plain Feat.  norm_act=ACT_*: the raw output with its InstanceNorm statistics,
        to be read as norm_act(IN(raw)) by the consumer."""
        if norm_act is None:
            return ops.conv2d(self.spec, [src], self.packed(), None if self.bias is None else self.bias.detach(), act=act)
        return ops.conv2d(self.spec, [src], self.packed(), None, want_stats=True, out_act=norm_act)


def _in_relu(t):
    """(y, mean, rstd) of a style_ops producer -> the Feat that its consumers read as relu(IN(y)); ``.data`` stays plain y."""
    return Feat(t[0], t[1], t[2], ACT_RELU)


class P2CConvBlock(nn.Module):
    """photo2cartoon.py:293-328: x -> residual + cat(x1, x2, x3), every convolution behind InstanceNorm + ReLU."""

    def __init__(self, dim_in, dim_out):
        super().__init__()
        self.dim_in, self.dim_out = dim_in, dim_out
        self.ConvBlock1 = _seq(_3=P2CConv(dim_in, dim_out // 2, 3, 1, 1, PAD_REFLECT))
        self.ConvBlock2 = _seq(_3=P2CConv(dim_out // 2, dim_out // 4, 3, 1, 1, PAD_REFLECT))
        self.ConvBlock3 = _seq(_3=P2CConv(dim_out // 4, dim_out // 4, 3, 1, 1, PAD_REFLECT))
        self.ConvBlock4 = _seq(_2=P2CConv(dim_in, dim_out, 1))

    def run(self, f, want_stats):
        """f: relu(IN(.)) view of the plain input (see _in_relu).  The result is plain; want_stats: with its statistics."""
        from . import style_ops as so
        x1 = self.ConvBlock1['3'].run(f, norm_act=ACT_RELU)
        x2 = self.ConvBlock2['3'].run(x1, norm_act=ACT_RELU)
        x3 = self.ConvBlock3['3'].run(x2)
        r = f.data if self.dim_in == self.dim_out else self.ConvBlock4['2'].run(f).data
        out = so.join(r, x1.data, x2.data, x3.data, want_stats)
        return _in_relu(out) if want_stats else Feat(out)


class P2CHourGlassBlock(nn.Module):
    """photo2cartoon.py:360-415: four levels of ConvBlock / avg_pool2d down, nearest up-sampling + skip back up."""

    def __init__(self, dim_in, dim_out):
        super().__init__()
        for name in ('1_1', '1_2', '2_1', '2_2', '3_1', '3_2', '4_1', '4_2', '5', '6', '7', '8', '9'):
            setattr(self, 'ConvBlock' + name, P2CConvBlock(dim_in if name == '1_1' else dim_out, dim_out))

    def run(self, x):
        from . import style_ops as so
        skips, down = [], x
        for lvl in '1234':
            skips.append(getattr(self, 'ConvBlock%s_1' % lvl).run(down, False))
            down = getattr(self, 'ConvBlock%s_2' % lvl).run(_in_relu(so.pool2(down.data, True)), True)
        up = self.ConvBlock5.run(down, True)
        for name, skip in zip('6789', reversed(skips)):
            up = _in_relu(so.up2_add(getattr(self, 'ConvBlock' + name).run(up, False).data, skip.data, True))
        return up


class P2CHourGlass(nn.Module):
    """photo2cartoon.py:330-357."""

    def __init__(self, dim_in, dim_out, use_res=True):
        super().__init__()
        self.use_res = use_res
        self.HG = _seq(_0=P2CHourGlassBlock(dim_in, dim_out), _1=P2CConvBlock(dim_out, dim_out), _2=P2CConv(dim_out, dim_out, 1))
        self.Conv1 = P2CConv(dim_out, 3, 1, bias=True)
        if use_res:
            self.Conv2 = P2CConv(dim_out, dim_out, 1, bias=True)
            self.Conv3 = P2CConv(3, dim_out, 1, bias=True)

    def run(self, x, want_stats=False):
        from . import style_ops as so
        ll = self.HG['1'].run(self.HG['0'].run(x), False)
        ll = self.HG['2'].run(ll, norm_act=ACT_RELU)
        tmp_out = self.Conv1.run(ll)
        if not self.use_res:
            return tmp_out
        out = so.sum3(x.data, self.Conv2.run(ll).data, self.Conv3.run(tmp_out).data, want_stats)
        return _in_relu(out) if want_stats else Feat(out)


class P2CResnetBlock(nn.Module):
    """photo2cartoon.py:417-434 (no bias): x + IN(conv(relu(IN(conv(x))))), the fp32 result kept (its plane means are read)."""

    def __init__(self, dim):
        super().__init__()
        self.conv_block = _seq(_1=P2CConv(dim, dim, 3, 1, 1, PAD_REFLECT), _5=P2CConv(dim, dim, 3, 1, 1, PAD_REFLECT))

    def run(self, x):
        y = self.conv_block['1'].run(x, norm_act=ACT_RELU)
        y = self.conv_block['5'].run(y, norm_act=ACT_NONE)
        return ops.materialize(y, residual=x, emit_xs=False)


class P2CLIN(nn.Module):
    """photo2cartoon.py:506-525; the reference's initial values."""

    def __init__(self, c):
        super().__init__()
        self.rho = nn.Parameter(torch.zeros(1, c, 1, 1))
        self.gamma = nn.Parameter(torch.ones(1, c, 1, 1))
        self.beta = nn.Parameter(torch.zeros(1, c, 1, 1))


class P2CAdaLIN(nn.Module):
    """photo2cartoon.py:488-503."""

    def __init__(self, c):
        super().__init__()
        self.rho = nn.Parameter(torch.full((1, c, 1, 1), 0.9))


class P2CSoftAdaLIN(nn.Module):
    """photo2cartoon.py:459-485.  The (N, C)-vector MLPs are stock torch (plumbing); the statistics and the normalisation are
    aps_lin_coeffs + aps_affine_apply."""

    def __init__(self, c):
        super().__init__()
        self.norm = P2CAdaLIN(c)
        self.w_gamma = nn.Parameter(torch.zeros(1, c))
        self.w_beta = nn.Parameter(torch.zeros(1, c))
        self.c_gamma = nn.Sequential(nn.Linear(c, c), nn.ReLU(True), nn.Linear(c, c))
        self.c_beta = nn.Sequential(nn.Linear(c, c), nn.ReLU(True), nn.Linear(c, c))
        self.s_gamma = nn.Linear(c, c)
        self.s_beta = nn.Linear(c, c)

    def coeffs(self, raw, content, style):
        from . import style_ops as so
        gamma = (1. - self.w_gamma) * self.s_gamma(style) + self.w_gamma * self.c_gamma(content)
        beta = (1. - self.w_beta) * self.s_beta(style) + self.w_beta * self.c_beta(content)
        return so.lin_coeffs(raw, self.norm.rho, gamma, beta)


class P2CSoftAdaLINBlock(nn.Module):
    """photo2cartoon.py:436-457."""

    def __init__(self, dim):
        super().__init__()
        self.conv1 = P2CConv(dim, dim, 3, 1, 1, PAD_REFLECT)
        self.norm1 = P2CSoftAdaLIN(dim)
        self.conv2 = P2CConv(dim, dim, 3, 1, 1, PAD_REFLECT)
        self.norm2 = P2CSoftAdaLIN(dim)

    def run(self, x, content, style):
        from . import style_ops as so
        raw = self.conv1.run(x).data
        a, b = self.norm1.coeffs(raw, content, style)
        raw = self.conv2.run(Feat(so.affine_apply(raw, a, b, so.ACT_RELU))).data
        a, b = self.norm2.coeffs(raw, content, style)
        return Feat(so.affine_apply(raw, a, b, so.ACT_NONE, residual=x.data))


class Photo2CartoonGenerator(nn.Module):
    """``ResnetGenerator(ngf, img_size, light=True)`` of Module2/models/photo2cartoon.py:166-291 (the U-GAT-IT-style
    generator of the third-party Photo2Cartoon project), forward only: the static cartoon of the streaming-inference model
    (geomcgt_ifw_test_model.py:228-229, 286-291).  ``state_dict()`` has the reference's key names, order and shapes, so
    ``load_state_dict(torch.load('cartoon.pt')['genA2B'], strict=True)`` works -- including the keys that do not influence
    the image (``gap_fc.bias``, ``gmp_fc.bias``, every ``ConvBlock4``).

    Convolutions: libapamd.so through ops.conv2d, producer InstanceNorm + ReLU fused into the consumer's loads.  LIN /
    adaLIN, joins, pools, up-sampling adds and plane means: libapstyle.so (style_ops).  The class-activation stage needs
    no kernel of its own: ``conv1x1(cat[x w_gap, x w_gmp])`` is a 1x1 convolution of x with the host-folded weight
    ``W[:, :C] w_gap + W[:, C:] w_gmp``; ``cam_logit`` and ``heatmap`` have no reader and are not computed."""

    def __init__(self, ngf=32, img_size=256, light=True):
        super().__init__()
        if not light:
            raise NotImplementedError('Photo2CartoonGenerator: light=False (a fully connected layer over the whole feature map) '
                                      'is not built; the published checkpoint is light=True')
        if ngf < 4 or ngf % 4:
            raise ValueError('Photo2CartoonGenerator: ngf = %d must be a positive multiple of 4' % ngf)
        self.ngf, self.img_size = ngf, img_size
        dim = ngf * 4
        self.ConvBlock1 = _seq(_1=P2CConv(3, ngf, 7, 1, 3, PAD_REFLECT))
        self.HourGlass1 = P2CHourGlass(ngf, ngf)
        self.HourGlass2 = P2CHourGlass(ngf, ngf)
        self.DownBlock1 = _seq(_1=P2CConv(ngf, ngf * 2, 3, 2, 1, PAD_REFLECT))
        self.DownBlock2 = _seq(_1=P2CConv(ngf * 2, dim, 3, 2, 1, PAD_REFLECT))
        for i in '1234':
            setattr(self, 'EncodeBlock' + i, P2CResnetBlock(dim))
        self.gap_fc = nn.Linear(dim, 1)
        self.gmp_fc = nn.Linear(dim, 1)
        self.conv1x1 = P2CConv(dim * 2, dim, 1, bias=True)
        self._cam_spec = ConvSpec([dim], dim, 1)
        self._cam_spec.precision = ops.PRECISION_FP32
        self._cam_packed = None          # (key, packed image of the folded weight)
        self.FC = nn.Sequential(nn.Linear(dim, dim), nn.ReLU(True), nn.Linear(dim, dim), nn.ReLU(True))
        for i in '1234':
            setattr(self, 'DecodeBlock' + i, P2CSoftAdaLINBlock(dim))
        self.UpBlock1 = _seq(_2=P2CConv(dim, ngf * 2, 3, 1, 1, PAD_REFLECT), _3=P2CLIN(ngf * 2))
        self.UpBlock2 = _seq(_2=P2CConv(ngf * 2, ngf, 3, 1, 1, PAD_REFLECT), _3=P2CLIN(ngf))
        self.HourGlass3 = P2CHourGlass(ngf, ngf)
        self.HourGlass4 = P2CHourGlass(ngf, ngf, False)
        self.ConvBlock2 = _seq(_1=P2CConv(3, 3, 7, 1, 3, PAD_REFLECT))

    def _cam(self, x):
        """relu(conv1x1(cat[x w_gap, x w_gmp]) + bias) as ONE 1x1 convolution of x (photo2cartoon.py:257-269)."""
        w, wg, wm = self.conv1x1.weight, self.gap_fc.weight, self.gmp_fc.weight
        key = tuple(ops.weight_key(t) for t in (w, wg, wm))
        if self._cam_packed is None or self._cam_packed[0] != key:
            c = wg.shape[1]
            folded = (w.detach()[:, :c] * wg.detach().view(1, c, 1, 1) + w.detach()[:, c:] * wm.detach().view(1, c, 1, 1)).contiguous()
            self._cam_packed = (key, ops.pack_weights(self._cam_spec, folded))
        return ops.conv2d(self._cam_spec, [x], self._cam_packed[1], self.conv1x1.bias.detach(), act=ACT_RELU)

    def _up_lin(self, blk, x, want_stats):
        """nn.Upsample(2) -> reflect 3x3 convolution -> LIN -> ReLU (photo2cartoon.py:221-231)."""
        from . import style_ops as so
        raw = blk['2'].run(Feat(so.up2_add(x))).data
        lin = blk['3']
        a, b = so.lin_coeffs(raw, lin.rho, lin.gamma, lin.beta)
        return so.affine_apply(raw, a, b, so.ACT_RELU, want_stats=want_stats)

    def forward(self, x):
        """G(x) -> (N, 3, H, W), the tanh image (element [0] of the reference's forward)."""
        from . import style_ops as so
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] % 16 or x.shape[3] % 16 or min(x.shape[2:]) < 32:
            raise ValueError('Photo2CartoonGenerator: input of shape %s; served: (N, 3, H, W) with H and W multiples of 16, at '
                             'least 32 (two stride-2 layers, four pooling levels, reflection pads)' % (tuple(x.shape),))
        with torch.no_grad():
            f = self.ConvBlock1['1'].run(Feat(x.contiguous()), norm_act=ACT_RELU)
            # relu(IN(raw)) is read three ways by the first hourglass (normalised again, pooled, added): written once,
            # as an affine map of the raw output, together with ITS statistics
            rstd = f.rstd
            f = _in_relu(so.affine_apply(f.data, rstd, -f.mean * rstd, so.ACT_RELU, want_stats=True))
            f = self.HourGlass1.run(f, True)
            f = self.HourGlass2.run(f, False)
            f = self.DownBlock1['1'].run(f, norm_act=ACT_RELU)
            f = self.DownBlock2['1'].run(f, norm_act=ACT_RELU)
            f = ops.materialize(f, emit_xs=False)
            content = []
            for i in '1234':
                f = getattr(self, 'EncodeBlock' + i).run(f)
                content.append(so.plane_mean(f.data))
            f = self._cam(f)
            style = self.FC(so.plane_mean(f.data))
            for i, cf in zip('1234', reversed(content)):
                f = getattr(self, 'DecodeBlock' + i).run(f, cf, style)
            y = self._up_lin(self.UpBlock1, f.data, False)
            f = _in_relu(self._up_lin(self.UpBlock2, y, True))
            f = self.HourGlass3.run(f, True)
            f = self.HourGlass4.run(f)
            return self.ConvBlock2['1'].run(f, act=ACT_TANH).data


class NLayerDiscriminator(nn.Module):
    """70x70 PatchGAN, networks.py:2602-2647 (n_layers=3, instance norm)."""

    def __init__(self, input_nc, ndf=64, n_layers=3, norm='instance'):
        super().__init__()
        if norm != 'instance':
            raise NotImplementedError('normalization layer [%s] is not available on the HIP path' % norm)
        if n_layers != 3:
            raise NotImplementedError('only the 3-layer PatchGAN (netD=basic) is on the HIP path')
        self.input_nc, self.ndf = input_nc, ndf
        self.model = _seq(_0=ConvLayer([input_nc], ndf, 4, 2, 1), _2=ConvLayer([ndf], ndf * 2, 4, 2, 1),
                          _5=ConvLayer([ndf * 2], ndf * 4, 4, 2, 1), _8=ConvLayer([ndf * 4], ndf * 8, 4, 1, 1),
                          _11=ConvLayer([ndf * 8], 1, 4, 1, 1))

    def forward(self, input):
        if torch.is_grad_enabled() and (input.requires_grad or any(p.requires_grad for p in self.parameters())):
            return discriminator_apply(self, input)
        return self.forward_inference(input)

    def forward_inference(self, input):
        return self._run(None, False, input).data

    def _run(self, tape, input_needs_grad, input):
        inp = Feat(input.contiguous())
        if tape is not None and input_needs_grad:
            tape.track(inp)
        self._last_input_feat = inp if tape is not None else None
        cf = conv_forward
        x = cf(tape, self.model['0'], inp, act=ACT_LRELU)
        x = cf(tape, self.model['2'], x, norm_act=ACT_LRELU)
        x = cf(tape, self.model['5'], x, norm_act=ACT_LRELU)
        x = cf(tape, self.model['8'], x, norm_act=ACT_LRELU)
        return cf(tape, self.model['11'], x)


# --------------------------------------------------------------------------- registry
def get_norm_layer(norm_type='instance'):
    """networks.py:22-39.  Returned token is what the HIP modules accept as ``norm``."""
    if norm_type in ('batch', 'none'):
        raise NotImplementedError('normalization layer [%s] is not available on the HIP path' % norm_type)
    if norm_type != 'instance':
        raise NotImplementedError('normalization layer [%s] is not found' % norm_type)
    return 'instance'


def get_scheduler(optimizer, opt):
    """networks.py:42-68."""
    if opt.lr_policy == 'linear':
        def lambda_rule(epoch):
            return 1.0 - max(0, epoch + opt.epoch_count - opt.niter) / float(opt.niter_decay + 1)
        return lr_scheduler.LambdaLR(optimizer, lr_lambda=lambda_rule)
    if opt.lr_policy == 'step':
        return lr_scheduler.StepLR(optimizer, step_size=opt.lr_decay_iters, gamma=0.1)
    if opt.lr_policy == 'plateau':
        return lr_scheduler.ReduceLROnPlateau(optimizer, mode='min', factor=0.2, threshold=0.01, patience=5)
    if opt.lr_policy == 'cosine':
        return lr_scheduler.CosineAnnealingLR(optimizer, T_max=opt.niter, eta_min=0)
    raise NotImplementedError('learning rate policy [%s] is not implemented' % opt.lr_policy)


def init_weights(net, init_type='normal', init_gain=0.02):
    """networks.py:71-102: conv weights by ``init_type``, biases 0."""
    for m in net.modules():
        if isinstance(m, ConvLayer):
            if init_type == 'normal':
                nn.init.normal_(m.weight.data, 0.0, init_gain)
            elif init_type == 'xavier':
                nn.init.xavier_normal_(m.weight.data, gain=init_gain)
            elif init_type == 'kaiming':
                nn.init.kaiming_normal_(m.weight.data, a=0, mode='fan_in')
            elif init_type == 'orthogonal':
                nn.init.orthogonal_(m.weight.data, gain=init_gain)
            else:
                raise NotImplementedError('initialization method [%s] is not implemented' % init_type)
            nn.init.constant_(m.bias.data, 0.0)
    print('initialize network with %s' % init_type)


def init_net(net, init_type='normal', init_gain=0.02, gpu_ids=[]):
    """networks.py:105-120.  The reference wraps in nn.DataParallel; here multi-GPU is one process
    per GPU (animateportrait_amd.parallel), so the net goes to gpu_ids[0] unwrapped -- its state_dict
    equals what the reference saves (base_model.py:152-163 saves ``net.module``)."""
    if len(gpu_ids) > 0:
        assert torch.cuda.is_available()
        net.to(gpu_ids[0])
    init_weights(net, init_type, init_gain=init_gain)
    return net


def define_G(input_nc, output_nc, ngf, netG, norm='batch', use_dropout=False, init_type='normal', init_gain=0.02,
             gpu_ids=[], model0_res=0, model1_res=0, extra_channel=3, div=3, disp=1, regarch=4):
    """networks.py:123-201."""
    norm = get_norm_layer(norm_type=norm)
    if netG == 'resnet_9blocks_rcatland32_full_ifw':
        net = ResnetConditionTriGenerator32_full_ifw(input_nc, output_nc, ngf, norm=norm, use_dropout=use_dropout,
                                                     n_blocks=9, div=div, disp=disp)
    elif netG == 'resnet_style2_9blocks':                                   # networks.py:155-156
        net = ResnetStyle2Generator(input_nc, output_nc, ngf, norm=norm, use_dropout=use_dropout, n_blocks=9,
                                    model0_res=model0_res, extra_channel=extra_channel)
    elif netG in _REFERENCE_ONLY_G:
        raise NotImplementedError('Generator model name [%s] is outside the MI355X hot path '
                                  '(only %s is built)' % (netG, ', '.join(GENERATOR_NAMES)))
    else:
        raise NotImplementedError('Generator model name [%s] is not recognized' % netG)
    return init_net(net, init_type, init_gain, gpu_ids)


def define_D(input_nc, ndf, netD, n_layers_D=3, norm='batch', init_type='normal', init_gain=0.02, gpu_ids=[],
             n_class=3):
    """networks.py:204-247."""
    norm = get_norm_layer(norm_type=norm)
    if netD == 'basic':
        net = NLayerDiscriminator(input_nc, ndf, n_layers=3, norm=norm)
    elif netD == 'n_layers':
        net = NLayerDiscriminator(input_nc, ndf, n_layers_D, norm=norm)
    elif netD in ('basic_cls', 'pixel'):
        raise NotImplementedError('Discriminator model name [%s] is outside the MI355X hot path' % netD)
    else:
        raise NotImplementedError('Discriminator model name [%s] is not recognized' % netD)
    return init_net(net, init_type, init_gain, gpu_ids)


class GANLoss(nn.Module):
    """networks.py:407-473.  lsgan: mean((pred - label)^2)."""

    def __init__(self, gan_mode, target_real_label=1.0, target_fake_label=0.0):
        super().__init__()
        self.register_buffer('real_label', torch.tensor(target_real_label))
        self.register_buffer('fake_label', torch.tensor(target_fake_label))
        self.gan_mode = gan_mode
        self._labels = (float(target_fake_label), float(target_real_label))   # host copies: no device sync
        if gan_mode not in ('lsgan', 'vanilla', 'wgangp'):
            raise NotImplementedError('gan mode %s not implemented' % gan_mode)

    def get_target_tensor(self, prediction, target_is_real):
        t = self.real_label if target_is_real else self.fake_label
        return t.expand_as(prediction)

    def __call__(self, prediction, target_is_real):
        if self.gan_mode == 'lsgan':                      # nn.MSELoss vs the expanded label: one fused reduction
            from . import losses
            return losses.lsgan_loss(prediction, self._labels[1 if target_is_real else 0])
        if self.gan_mode == 'vanilla':
            return nn.functional.binary_cross_entropy_with_logits(
                prediction, self.get_target_tensor(prediction, target_is_real))
        return -prediction.mean() if target_is_real else prediction.mean()


class FaceLoss(nn.Module):
    """networks.py:2862-2966 around a frozen feature network: ``forward(imgs1, imgs2, bbox1=, bbox2=)`` crops the
    ``[x1, x2, y1, y2]`` windows into ones-filled squares, resizes them to ``height x width`` (bilinear,
    align_corners=True) and sums the L1 distances of the network's feature list (second argument detached).
    The reference builds Sphere20a from ``checkpoints/sphere20a_20171020.pth`` (absent from its tree); here the
    network is passed in (stock PyTorch-ROCm module), the crop + resize is one HIP launch each way."""

    def __init__(self, net, height=112, width=96):
        super().__init__()
        self.net = net.eval()
        self.height, self.width = height, width

    def crop_head_bbox(self, imgs, bboxs):                                          # :2946-2966
        from . import losses
        n, c = imgs.shape[:2]
        win = bboxs if (torch.is_tensor(bboxs) and bboxs.is_cuda and bboxs.dtype == torch.int32) else \
            losses.windows_to_device(bboxs, n, imgs.device)
        # the reference fills a 3-channel box from the image's channels; a 1-channel drawing was repeated x3 by the
        # caller (geomgm_ifw_fore_model.py:745-750) -- reading channel 0 three times is the same tensor
        return losses.crop_resize(imgs, win, (0, 0, 0) if c == 1 else (0, 1, 2), (self.height, self.width),
                                  losses.RESIZE_BILINEAR_AC)

    def compute_loss(self, img1, img2):                                            # :2926-2940
        f1 = self.net(img1)
        with torch.no_grad():
            f2 = self.net(img2)
        loss = 0.0
        for a, b in zip(f1, f2):
            loss = loss + nn.functional.l1_loss(a, b.detach())
        return loss

    def forward(self, imgs1, imgs2, kps1=None, kps2=None, bbox1=None, bbox2=None):
        if kps1 is not None or kps2 is not None or bbox1 is None or bbox2 is None:
            raise NotImplementedError('FaceLoss on the HIP path takes bbox1 / bbox2 (the only form the model uses, '
                                      'geomgm_ifw_fore_model.py:745-752)')
        return self.compute_loss(self.crop_head_bbox(imgs1, bbox1), self.crop_head_bbox(imgs2, bbox2))
