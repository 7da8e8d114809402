"""Reverse pass of the generator / discriminator as an explicit schedule of HIP launches.

The reference relies on torch.autograd over ATen ops (``loss.backward()``,
Module2/models/geomgm_ifw_fore_model.py:586,610,634,780).  Here each network is ONE
``torch.autograd.Function`` to PyTorch; inside, the forward records a tape of layer closures and the
backward replays it in reverse, launching the data-gradient (the forward conv kernel with swapped
roles), weight-gradient, InstanceNorm/activation-backward and warp-backward kernels of libapamd.so.
PyTorch only carries the resulting tensors to the optimiser / the collective.
"""
import collections

import torch

from . import ops
from .ops import Feat, ConvSpec, ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH, PAD_ZERO, PAD_REFLECT, W_OIHW, W_IOHW


# ctx.needs_input_grad only mirrors requires_grad: a custom Function cannot see whether THIS backward call wants the
# parameter gradients (torch.autograd.grad(loss, [input]) runs the same node and drops them).  Writing them straight into
# the optimiser's flat buffer is therefore opt-in: the train step wraps its ``loss.backward()`` calls in
# ``direct_param_grads()``; everywhere else the gradients go back through autograd.
_DIRECT = 0


class direct_param_grads:
    """``with direct_param_grads(): loss.backward()`` -- the caller states that this backward accumulates into ``p.grad`` of
    every trainable parameter (plain ``.backward()`` of the train step, geomgm_ifw_fore_model.py:586,610,634,780)."""

    def __enter__(self):
        global _DIRECT
        _DIRECT += 1

    def __exit__(self, *exc):
        global _DIRECT
        _DIRECT -= 1
        return False


class Tape:
    def __init__(self):
        self.steps = []
        self.grads = {}          # id(Feat) -> list of (tensor, pad)
        self.keep = []           # keep Feats alive so ids stay unique
        self.param_grads = {}    # Parameter -> tensor
        self.block = None        # contiguous gradient block of the network (see grad_block), or None
        self.block_lo = 0

    def grad_block(self, params, needs=None):
        """When every trainable parameter of the network is a view of ONE optimiser's flat buffer (optim.FlatAdam) and
        the views are adjacent, the backward kernels write the parameter gradients straight into one contiguous block
        laid out like that range; the whole block is then added to the optimiser's flat gradient buffer with one launch
        -- instead of one AccumulateGrad add per parameter and call (~200 launches per train step).

        This bypasses autograd's own accumulation, so it is taken only when that is exactly what autograd would have
        done: the caller opted in (``direct_param_grads()``: a plain ``loss.backward()`` of the train step --
        ``torch.autograd.grad(loss, [input])`` / ``backward(inputs=...)`` must not touch the optimiser's buffers), every
        trainable parameter is wanted (``needs``), and every ``p.grad`` still IS its view of the flat gradient buffer (after
        ``module.zero_grad()`` / ``p.grad = None`` autograd would start from a fresh tensor, not add to stale sums)."""
        if _DIRECT <= 0:
            return False
        live = [p for p in params if p.requires_grad]
        if not live or any(getattr(p, '_flat_owner', None) is None for p in live):
            return False
        if needs is not None and not all(n for p, n in zip(params, needs) if p.requires_grad):
            return False
        owner = live[0]._flat_owner
        if any(p._flat_owner is not owner for p in live):
            return False
        base = owner.flat_grad.data_ptr()
        if any(p.grad is None or p.grad.data_ptr() != base + 4 * p._flat_off for p in live):
            return False
        lo = min(p._flat_off for p in live)
        hi = max(p._flat_off + p.numel() for p in live)
        if hi - lo != sum(p.numel() for p in live):
            return False
        self.block = torch.zeros(hi - lo, dtype=torch.float32, device=owner.flat_grad.device)
        self.block_lo, self.block_owner = lo, owner
        return True

    def slot(self, p):
        """Where the gradient kernel of parameter ``p`` should write (None: allocate; a second contribution to the
        same parameter is computed apart and added)."""
        if self.block is None or p in self.param_grads:
            return None
        o = p._flat_off - self.block_lo
        return self.block[o:o + p.numel()].view(p.shape)

    def flush_block(self):
        if self.block is not None:
            from . import losses
            o = self.block_owner
            losses.axpy_(o.flat_grad[self.block_lo:self.block_lo + self.block.numel()], self.block)
            self.block = None

    def track(self, f):
        self.grads[id(f)] = []
        self.keep.append(f)
        return f

    def tracked(self, f):
        return id(f) in self.grads

    def add(self, f, tensor, pad=0):
        if id(f) in self.grads:
            self.grads[id(f)].append((tensor, pad))

    def take(self, f):
        return self.grads.pop(id(f), [])

    def add_param(self, p, g):
        if p in self.param_grads:
            prev = self.param_grads[p]
            if self.block is not None:
                prev.add_(g)                     # prev is the parameter's slot of the block
            else:
                self.param_grads[p] = prev + g
        else:
            self.param_grads[p] = g

    def backward(self):
        for fn in reversed(self.steps):
            fn()
        self.steps = []


# ------------------------------------------------------------------------------ conv layer
def _dgrad_spec(layer, seg_c):
    """ConvSpec of the operator that computes the data gradient for one input segment (same arithmetic as the
    layer's forward pass)."""
    spec, fold = _dgrad_spec_geometry(layer, seg_c)
    spec.precision = layer.spec.precision
    return spec, fold


def _dgrad_spec_geometry(layer, seg_c):
    s = layer.spec
    k = s.k
    if s.transposed:      # ConvTranspose2d(k, s=2, p): gradient is a stride-2 convolution, weight read as OIHW
        return ConvSpec([s.cout], seg_c, k, 2, s.pad, PAD_ZERO, False, 0, W_OIHW, False), 0
    if s.stride == 1:     # full correlation with flipped taps; reflection-padded layers stay in padded coords
        if s.pad_mode == PAD_REFLECT:
            return ConvSpec([s.cout], seg_c, k, 1, k - 1, PAD_ZERO, False, 0, W_IOHW, True), s.pad
        return ConvSpec([s.cout], seg_c, k, 1, k - 1 - s.pad, PAD_ZERO, False, 0, W_IOHW, True), 0
    # stride 2: transposed convolution; output_padding restores the input size
    return ConvSpec([s.cout], seg_c, k, 2, s.pad, PAD_ZERO, True, 1 if k == 3 else 0, W_IOHW, False), 0


# How one call of a layer's backward runs: decided once per form of the call (_backward_plan) and cached on the layer; the four
# executors below only follow it.  A new backward route is a new value of one of these fields.
#   norm_route     'split' (ops.instnorm_bwd_split writes its consumers' operands, no fp32 dy) | 'instnorm' | 'act_bias' | 'act'
#   dy16           'instnorm' only: dy is stored as bf16 (its one reader is the stems' weight gradient on the bf16 matrix pipe)
#   gt_dims, want_xs, want_strip   'split' only: the operands to write
#   wgrad_route    ops.wgrad_route's answer; None: the weight is frozen
#   wgrad_operand  'own' (the kernel reads dy) | 'g_t' | 'g_xs_from_split' | 'g_xs_presplit' (the split copy is made on the spot)
#   dgrad          per source segment None (not tracked) or (route, fold_pad); route 'final_k7' | 'head' | 'strip' | 'conv'
BackwardPlan = collections.namedtuple('BackwardPlan', 'norm_route dy16 gt_dims want_xs want_strip wgrad_route wgrad_operand dgrad')


def _backward_plan(tape, layer, srcs, out, norm, act, contribs):
    """The BackwardPlan of this call.  The decision depends on shapes, on which copies exist and on who wants a gradient, not on
    values: that form, together with ops.backward_switches(), is the key it is kept under (a dozen C-side plan queries per layer
    and step otherwise)."""
    form = (norm, act, layer.spec.precision, layer.weight.requires_grad, layer.bias.requires_grad, ops.form_of(out),
            tuple(sorted(p for _, p in contribs if p > 0)), tuple((ops.form_of(f), tape.tracked(f)) for f in srcs))
    key = (form, ops.backward_switches())
    cache = layer.__dict__.setdefault('_backward_plans', {})
    if key not in cache:
        cache[key] = _make_backward_plan(layer, *form)
    return cache[key]


def _make_backward_plan(layer, norm, act, precision, w_grad, b_grad, out, pads, srcs):
    """Reads forms (ops.form_of) and asks the C-side plan queries; touches no memory."""
    s = layer.spec
    forms = [f for f, _ in srcs]
    g = ops.Form(out.shape, torch.float32, False, ACT_NONE, False, False, False, False)       # dy: a plain fp32 feature
    dgrad = tuple(_dgrad_route(layer, c, g, f, len(srcs)) if tracked else None for c, (f, tracked) in zip(s.cin_segments, srcs))
    geom = (s.k, s.stride, s.pad, s.pad_mode, out.shape, forms, precision)
    # split-bf16 3x3 layers (and the PatchGAN's 4x4) whose sources carry their forward copies: the weight gradient reads the
    # gradient's split copy itself (ap_conv2d_wgrad_xs) -- no prepared operand; plain bf16 keeps the prepared-operand kernel
    xs_ok = (w_grad and not s.transposed and precision == ops.PRECISION_BF16X3 and ops.DEFAULT_PRECISION == ops.PRECISION_BF16X3 and
             ops.wgrad_xs_ok(*geom))
    split = _split_operands(layer, out, pads, w_grad, xs_ok, geom, dgrad) if norm else None
    if split is not None:
        norm_route, (gt_dims, want_xs) = 'split', split
        operand = 'g_xs_from_split' if xs_ok else ('g_t' if gt_dims is not None else 'own')
    else:
        norm_route = 'instnorm' if norm else ('act_bias' if b_grad and act != ACT_NONE else 'act')
        gt_dims, want_xs = None, False
        # (the split copy the data-gradient convolution stages anyway, cached on the Feat, is the weight gradient's operand too)
        operand = 'g_xs_presplit' if xs_ok and out.shape[1] % 8 == 0 else 'own'
    route = None
    if w_grad and s.transposed:         # dW[ci][co*k*k]: M-role = the layer input (virtual allowed), shifted tensor = dy (stride 2)
        route = ops.wgrad_route(s.k, 2, s.pad, PAD_ZERO, forms[0], [g], layer.weight.shape, precision, False)
    elif w_grad:
        route = ops.wgrad_route(s.k, s.stride, s.pad, s.pad_mode, g, forms, layer.weight.shape, precision, operand != 'own')
    # a stem (no data gradient: its input is an image) whose weight gradient runs on the bf16 matrix pipe: dy has one reader, which
    # rounds it to bf16.  (The package mode is asked here, not by wgrad_route: ops.wgrad takes the route by the layer's precision)
    dy16 = (norm_route == 'instnorm' and route == 'k7_stem' and not any(t for _, t in srcs) and
            ops.DEFAULT_PRECISION == ops.PRECISION_BF16)
    want_strip = norm_route == 'split' and any(d is not None and d[0] == 'strip' for d in dgrad)
    return BackwardPlan(norm_route, dy16, gt_dims, want_xs, want_strip, route, operand, dgrad)


def _dgrad_route(layer, seg_c, g, f, nsrc):
    s = layer.spec
    spec, fold_pad = _dgrad_spec(layer, seg_c)
    if nsrc == 1 and s.cout == 1 and ops.final_dgrad_k7_ok(s, g, f):
        return 'final_k7', fold_pad        # the generator's last layer in plain-bf16 arithmetic: the padded gradient on the bf16 matrix pipe
    if nsrc == 1 and s.cout == 1 and ops.head_dgrad_ok(s, g, f):
        return 'head', fold_pad            # the PatchGAN's output layer in plain-bf16 arithmetic: its gradient as an output stream
    if fold_pad and ops.dgrad_strip_eligible(spec, g):
        return 'strip', fold_pad           # 66-column padded gradient: two whole tile columns + a transposed 2-column strip
    return 'conv', fold_pad


def _split_operands(layer, out, pads, w_grad, xs_ok, geom, dgrad):
    """Can the InstanceNorm backward of ``out`` write the operands of its consumers itself (ops.instnorm_bwd_split)?  Yes when every
    consumer of the gradient is a bf16 matrix kernel: the weight gradient takes the gradient's split copy (xs_ok) or a prepared
    M-role operand (ops.wgrad_gt_dims) and each data gradient stages split copies.  Returns (gt_dims, want_xs) or None."""
    s = layer.spec
    if (s.transposed or s.precision == ops.PRECISION_FP32 or ops.DEFAULT_PRECISION == ops.PRECISION_FP32 or (pads and pads[-1] > 1) or
            not ops.instnorm_bwd_split_ok(out, 1 if pads else 0)):
        return None
    gt_dims = None
    if w_grad and not xs_ok:
        gt_dims = ops.wgrad_gt_dims(*geom)
        if gt_dims is None:
            return None
    n, _, h, w = out.shape
    if not all(d is None or ops.takes_split(_dgrad_spec(layer, c)[0], n, h, w) for c, d in zip(s.cin_segments, dgrad)):
        return None
    want_xs = any(d is not None for d in dgrad)
    return (gt_dims, want_xs or xs_ok) if (w_grad or want_xs) else None


def conv_backward(tape, layer, srcs, out, norm, act):
    """out: Feat produced by layer.run(srcs).  Consumes out's gradient contributions."""
    contribs = tape.take(out)
    if not contribs:
        return
    plan = _backward_plan(tape, layer, srcs, out, norm, act, contribs)
    gfeat, gt, strip, db = _backward_norm(tape, plan, layer, out, act, contribs)
    _backward_weight(tape, plan, layer, srcs, gfeat, gt)
    _backward_bias(tape, layer, norm, gfeat, db)
    _backward_data(tape, plan, layer, srcs, gfeat, strip)


def _backward_norm(tape, plan, layer, out, act, contribs):
    """The gradient w.r.t. the raw convolution output as (Feat, prepared M-role operand, column strip, bias gradient); the last
    three None where the route does not make them."""
    if plan.norm_route == 'split':
        return ops.instnorm_bwd_split(ops._split_contribs(contribs), out, plan.gt_dims, plan.want_xs, plan.want_strip) + (None,)
    if out.data.dtype != torch.float32:      # (a bf16 raw output whose backward takes the fp32 route after all: convert once)
        out = Feat(out.data.float(), out._mean, out._rstd, out.act)
        contribs = [(g.float() if g.dtype != torch.float32 else g, pd) for g, pd in contribs]
    db = None
    if plan.norm_route == 'instnorm':
        dy = ops.instnorm_bwd(contribs, out, out_bf16=plan.dy16)
    elif plan.norm_route == 'act_bias':
        # a plain layer with an activation (the PatchGAN's first): the bias gradient's block sums are formed while dy is written
        dy, db = ops.act_bwd_bias(contribs, out.data, act, tape.slot(layer.bias))
    else:
        dy = ops.act_bwd(contribs, out.data, act)
    gfeat = Feat(dy)
    if plan.wgrad_operand == 'g_xs_presplit':
        ops.presplit(gfeat, layer.spec.precision)
    return gfeat, None, None, db


def _backward_weight(tape, plan, layer, srcs, gfeat, gt):
    if plan.wgrad_route is None:
        return
    s = layer.spec
    if s.transposed:
        dw = ops.wgrad(s.k, 2, s.pad, PAD_ZERO, srcs[0], [gfeat], layer.weight.shape, precision=s.precision,
                       out=tape.slot(layer.weight), route=plan.wgrad_route)
    else:
        g_xs = gfeat.xs if plan.wgrad_operand in ('g_xs_from_split', 'g_xs_presplit') else None
        dw = ops.wgrad(s.k, s.stride, s.pad, s.pad_mode, gfeat, srcs, layer.weight.shape, precision=s.precision,
                       out=tape.slot(layer.weight), g_t=gt, g_xs=g_xs, route=plan.wgrad_route)
    tape.add_param(layer.weight, dw)


def _backward_bias(tape, layer, norm, gfeat, db):
    if not layer.bias.requires_grad:
        return
    slot = tape.slot(layer.bias)
    if norm:     # a bias in front of InstanceNorm has an exactly-zero gradient (it is removed by the mean subtraction)
        tape.add_param(layer.bias, slot if slot is not None else torch.zeros_like(layer.bias))   # block is zero-filled
    else:
        tape.add_param(layer.bias, db if db is not None else ops.bias_grad(gfeat.data, out=slot))


def _backward_data(tape, plan, layer, srcs, gfeat, strip):
    """One launch (the strip route: two) per input segment that needs a gradient."""
    s = layer.spec
    c0 = 0
    for i, (f, c, route) in enumerate(zip(srcs, s.cin_segments, plan.dgrad)):
        if route is not None and route[0] == 'final_k7':
            tape.add(f, ops.final_dgrad_k7(gfeat, layer.weight), route[1])
        elif route is not None and route[0] == 'head':
            tape.add(f, ops.head_dgrad(gfeat, layer.weight, f.data.shape[2], f.data.shape[3]), route[1])
        elif route is not None:
            spec, _ = _dgrad_spec(layer, c)
            w = layer.weight.detach()
            if len(srcs) > 1:
                w = w[c0:c0 + c] if s.transposed else w[:, c0:c0 + c]       # a view: the packer takes strides
            packed = layer.packed_dgrad(i, spec, w)
            if route[0] == 'strip':
                packed_t = layer.packed_dgrad((i, 'T'), spec, w.transpose(2, 3))
                # (a source whose raw output is stored as bf16 has this gradient as its ONLY contribution and its InstanceNorm
                # backward on the operand-writing route: the gradient is stored as bf16 too)
                g = ops.conv2d_dgrad_strip(spec, gfeat, packed, packed_t, strip, out_bf16=f.data.dtype == torch.bfloat16)
            else:
                g = ops.conv2d(spec, [gfeat], packed, None).data
            tape.add(f, g, route[1])
        c0 += c


def conv_forward(tape, layer, srcs, norm_act=None, act=ACT_NONE, out_octet=False, raw16=False):
    """raw16: the raw output may be STORED as bf16 (plain-bf16 train step; the caller vouches that every reader of it is one of
    ap_norm_apply_split, ap_instnorm_bwd_split and the padded-row operand kernel of the weight gradient: the main-branch
    convolutions of the ResNet blocks)."""
    if not isinstance(srcs, (list, tuple)):
        srcs = [srcs]
    raw16 = (raw16 and tape is not None and norm_act is not None and ops.BF16_RAW and ops.DEFAULT_PRECISION == ops.PRECISION_BF16 and
             layer.spec.precision == ops.PRECISION_BF16)
    out = layer.run(srcs, norm_act=norm_act, act=act, out_octet=out_octet and tape is None, out_bf16=raw16)
    if tape is not None:
        tape.track(out)
        norm = norm_act is not None
        tape.steps.append(lambda: conv_backward(tape, layer, srcs, out, norm, act))
    return out


def _reduced(tape, f):
    """The gradient of ``f`` as ONE plain tensor: its contributions taken off the tape, summed, the padded ones folded.  None
    when nothing contributed."""
    contribs = tape.take(f)
    if not contribs:
        return None
    g1, pad, g2 = ops._split_contribs(contribs)
    return g1 if (pad == 0 and g2 is None) else ops.fold_add(g1, pad, g2)


def materialize_forward(tape, f, residual=None, consumer=None):
    """consumer: a ConvLayer that reads the result and is not a c -> c trunk layer; the fp32 tensor is dropped (inference)
    only if that layer, too, stages split copies (at ngf = 16 the first up-convolution, 64 -> 32, reads fp32)."""
    keep = tape is not None or (consumer is not None and not consumer.stages_split(f.data.shape))
    out = ops.materialize(f, residual=residual, keep_fp32=keep)
    if tape is not None:
        tape.track(out)

        def bwd():
            g = _reduced(tape, out)
            if g is None:
                return
            tape.add(f, g, 0)
            if residual is not None:
                tape.add(residual, g, 0)
        tape.steps.append(bwd)
    return out


def warp_forward(tape, f, motion, flow, ifmask, level, consumer=None):
    """consumer: the ConvLayer that reads the warped concat.  When it stages split-bf16 sources the warp writes that
    copy itself; in inference (no tape) the fp32 concat is then not written at all."""
    n, _, h, w = f.data.shape
    emit_xs = consumer is not None and ops.takes_split(consumer.spec, n, h, w)
    s2d = emit_xs and len(consumer.spec.cin_segments) == 1 and ops.s2d_eligible(consumer.spec, h, w)
    out = ops.warp_concat(f, motion, flow, ifmask, level, emit_xs=emit_xs, keep_fp32=tape is not None or not emit_xs, s2d=s2d)
    if tape is not None:
        tape.track(out)

        def bwd():
            g = _reduced(tape, out)
            if g is None or not tape.tracked(f):
                return
            tape.add(f, ops.warp_concat_bwd(g, motion, flow, ifmask, level), 0)
        tape.steps.append(bwd)
    return out


def batch_split_forward(tape, f, b):
    """l -> (l[:b], l[b:]) for the shared landmark encoder run on the stacked 2B batch."""
    l1, l2 = f.batch_slice(0, b), f.batch_slice(b, 2 * b)
    if tape is not None:
        tape.track(l1)
        tape.track(l2)

        def bwd():
            tape.add(f, torch.cat([_reduced(tape, l1), _reduced(tape, l2)], 0), 0)
        tape.steps.append(bwd)
    return l1, l2


# ------------------------------------------------------------------------------ autograd.Function wrappers
def _weights_stamp(params):
    """What the backward pass assumes unchanged since forward: it reads ``layer.weight`` live (the packed copies are
    rebuilt from it), so an optimiser step in between would silently give gradients of a different network, where
    torch.autograd raises its saved-tensor version error."""
    return tuple(ops.weight_key(p) for p in params)


class _NetFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, net, n_inputs, input_needs_grad, *tensors):
        inputs, params = tensors[:n_inputs], tensors[n_inputs:]
        tape = Tape()
        with torch.no_grad():
            out = net._run(tape, input_needs_grad, *inputs)
        ctx.tape, ctx.net, ctx.out_feat = tape, net, out
        ctx.n_inputs, ctx.params = n_inputs, params
        ctx.stamp = _weights_stamp(params)
        ctx.in_feat = getattr(net, '_last_input_feat', None)
        return out.data

    @staticmethod
    def backward(ctx, gout):
        tape = ctx.tape
        if tape is None:
            raise RuntimeError('animateportrait_amd: backward through this network a second time: the layer tape is '
                               'freed after the first pass (retain_graph is not supported); run forward again')
        if _weights_stamp(ctx.params) != ctx.stamp:
            raise RuntimeError('animateportrait_amd: a parameter of %s was modified (optimizer.step / in-place write) '
                               'between forward and backward; its gradients would belong to different weights'
                               % type(ctx.net).__name__)
        with torch.no_grad():
            direct = tape.grad_block(ctx.params, ctx.needs_input_grad[3 + ctx.n_inputs:])
            tape.add(ctx.out_feat, gout.contiguous(), 0)
            tape.backward()
            gin = [None] * ctx.n_inputs
            if ctx.in_feat is not None and tape.tracked(ctx.in_feat):
                gin[0] = _reduced(tape, ctx.in_feat)
            if direct:       # already summed into the optimiser's flat gradient buffer (p.grad is a view of it)
                tape.flush_block()
                gp = [None] * len(ctx.params)
            else:
                gp = [tape.param_grads.get(p) for p in ctx.params]
        ctx.tape = None
        return (None, None, None, *gin, *gp)


def generator_apply(net, input, land1, land2, motion, flow, ifmask):
    """The reference generator is differentiable w.r.t. every input; this path defines the gradient w.r.t. the image
    ``input`` (the three stems' data gradients) and refuses the others instead of silently returning zeros: no caller
    on the hot path asks for them (land / motion / flow / ifmask come from the data layer and netF under no_grad,
    geomgm_ifw_fore_model.py:443-505), and ap_warp_concat_bwd has no gradient w.r.t. the sampling grid."""
    for t, name in ((land1, 'land1'), (land2, 'land2'), (motion, 'motion'), (flow, 'flow'), (ifmask, 'ifmask')):
        if t.requires_grad:
            raise NotImplementedError('animateportrait_amd generator: gradient w.r.t. %s is not defined on the HIP '
                                      'path (detach it)' % name)
    params = [p for p in net.parameters()]
    return _NetFn.apply(net, 6, bool(input.requires_grad), input, land1, land2, motion, flow, ifmask, *params)


def discriminator_apply(net, input):
    params = [p for p in net.parameters()]
    return _NetFn.apply(net, 1, bool(input.requires_grad), input, *params)
