"""The 2D side of face_alignment's 3D-FAN landmark network on the MI355X: a stack of pre-activation hourglasses (BatchNorm ->
ReLU -> conv) that turns a (B, 3, 256, 256) face crop into 68 heat maps of 64 x 64.  The reference reads the photo's landmarks
from ``face_alignment.FaceAlignment(LandmarksType._3D, flip_input=True).get_landmarks`` (main_end2end_module2.py:186-193); its
depth column is overwritten downstream (module1.adjust_and_norm_input_face), so the package's depth network is not built.

``FAN`` keeps the package's ``state_dict`` keys (its own modules only store the parameters).  ``prepare()`` turns them into what
the forward runs on:

* every convolution goes through ops.conv2d in exact fp32, as networks.P2CConv does;
* an eval-mode BatchNorm + ReLU IN FRONT of a convolution is the per-channel pair (m', s) with
  relu(g (y - mu) / sqrt(var + eps) + b) = relu((y - m') s),  s = g / sqrt(var + eps),  m' = mu - b / s,
  replicated over N and handed to the convolution as ``ops.Feat(y, m', s, ACT_RELU)``: the normalisation happens in the
  consumer's loads (the loads compute (y - mean) * rstd and nothing in them needs rstd > 0: conv_igemm.h commit_x,
  conv_small.h).  A layer that has a channel with |s| < S_MIN (g = 0 among them: m' does not exist) is materialised instead
  through style_ops.affine_apply(y, s, b - mu s, ACT_RELU);
* a BatchNorm BEHIND a convolution (the stem's bn1, bn_end<i>) is folded into that convolution's weight and bias;
* joins, pools, up-sampling adds and the three-way sum are style_ops.join / pool2 / up2_add / sum3.

A layer the convolution library has no kernel for (its plan refuses the descriptor; DESIGN.md section 4c-9 lists them: the 7x7
stride-2 stem at every width) runs through torch.nn.functional.conv2d on the materialised input.

Parity with the package and with its published checkpoint is UNPINNED: neither is part of this repository; the contract is the
float64 statement tests/fan_reference.py.
"""
import ctypes
import re
import zipfile

import torch
import torch.nn as nn

from . import _capi as C
from . import ops
from .ops import Feat, ConvSpec, ACT_NONE, ACT_RELU, PAD_ZERO

BN_EPS = 1e-5
# Below this |s| a channel does not take the Feat route.  With |s| >= S_MIN, m' = mu - b / s is at most |mu| + 1e6 |b|: finite
# in fp32 for any trained b, and the rounding of (y - m') s is 2^-23 |b - mu s| however large m' is -- the rounding of the
# affine form's own sum.  Below it (s = 0 first of all) m' overflows or does not exist.
S_MIN = 1e-6
POINTS = 68


def bn_constants(weight, bias, mean, var, eps=BN_EPS):
    """(s, b') of an eval-mode BatchNorm in float64: BN(y) = s y + b',  s = g / sqrt(var + eps),  b' = b - mu s."""
    g, b, mu, var = (t.detach().double().cpu() for t in (weight, bias, mean, var))
    s = g / torch.sqrt(var + eps)
    return s, b - mu * s


def feat_constants(weight, bias, mean, var, eps=BN_EPS):
    """(m', s, direct) in float64: relu(BN(y)) = relu((y - m') s) where ``direct``; m' of a channel below S_MIN is 0."""
    s, _ = bn_constants(weight, bias, mean, var, eps)
    small = s.abs() < S_MIN
    safe = torch.where(small, torch.ones_like(s), s)
    m = mean.detach().double().cpu() - bias.detach().double().cpu() / safe
    m = torch.where(small, torch.zeros_like(m), m)
    direct = not bool(small.any()) and bool(torch.isfinite(m.float()).all())
    return m, s, direct


def fold_post_bn(conv_w, conv_b, weight, bias, mean, var, eps=BN_EPS):
    """BN(conv(x) + cb) = conv'(x) + cb' in float64: w' = s w per output channel, cb' = s cb + b'."""
    s, b2 = bn_constants(weight, bias, mean, var, eps)
    w = conv_w.detach().double().cpu() * s.view(-1, 1, 1, 1)
    cb = torch.zeros_like(s) if conv_b is None else conv_b.detach().double().cpu()
    return w, cb * s + b2


def conv_served(spec, n, h, w):
    """whether libapamd has a kernel for this layer at this size (the plan is made on the host: no device is touched)"""
    d = spec.desc(n, h, w)
    ho, wo = ctypes.c_int32(), ctypes.c_int32()
    return C.lib().ap_conv2d_out_size(ctypes.byref(d), ctypes.byref(ho), ctypes.byref(wo)) == 0


class _PreBN:
    """BatchNorm + ReLU in front of a convolution, as constants on the device"""

    def __init__(self, bn, device):
        m, s, self.direct = feat_constants(bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)
        _, b2 = bn_constants(bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)
        self._c = [t.float().to(device) for t in ((m, s) if self.direct else (s, b2))]
        self._rep = {}

    def _replicated(self, n):
        if n not in self._rep:
            self._rep[n] = [t.repeat(n).contiguous() for t in self._c]
        return self._rep[n]

    def feat(self, y):
        """the Feat a convolution reads as relu(BN(y))"""
        from . import style_ops as so
        p, q = self._replicated(y.shape[0])
        if self.direct:
            return Feat(y, p, q, ACT_RELU)
        return Feat(so.affine_apply(y, p, q, ACT_RELU))


class _Conv:
    """one convolution with its (folded) fp32 weights on the device"""

    def __init__(self, name, w, b, stride, pad, device):
        self.name = name
        self.w = w.float().to(device).contiguous()
        self.b = None if b is None else b.float().to(device).contiguous()
        cout, cin, k, _ = self.w.shape
        self.stride, self.pad = stride, pad
        self.spec = ConvSpec([cin], cout, k, stride, pad, PAD_ZERO)
        self.spec.precision = ops.PRECISION_FP32
        self._packed = None
        self._served = {}

    def served(self, n, h, w):
        key = (n, h, w)
        if key not in self._served:
            self._served[key] = conv_served(self.spec, n, h, w)
        return self._served[key]

    def run(self, f, act=ACT_NONE):
        """act(conv(f) + bias) as a plain tensor; f: a Feat (plain, or the relu(BN(.)) view of a raw tensor)"""
        n, _, h, w = f.data.shape
        if self.served(n, h, w):
            if self._packed is None:
                self._packed = ops.pack_weights(self.spec, self.w)
            return ops.conv2d(self.spec, [f], self._packed, self.b, act=act).data
        x = f.data
        if f.virtual:
            from . import style_ops as so
            x = so.affine_apply(x, f.rstd, -f.mean * f.rstd, f.act)       # (y - m') s as s y + (-m' s)
        y = torch.nn.functional.conv2d(x, self.w, self.b, self.stride, self.pad)
        return torch.relu_(y) if act == ACT_RELU else y


def _bn(c):
    return nn.BatchNorm2d(c)


class ConvBlock(nn.Module):
    """in -> cat(out/2, out/4, out/4) + residual, every convolution behind BatchNorm + ReLU"""

    def __init__(self, cin, cout):
        super().__init__()
        self.bn1, self.conv1 = _bn(cin), nn.Conv2d(cin, cout // 2, 3, 1, 1, bias=False)
        self.bn2, self.conv2 = _bn(cout // 2), nn.Conv2d(cout // 2, cout // 4, 3, 1, 1, bias=False)
        self.bn3, self.conv3 = _bn(cout // 4), nn.Conv2d(cout // 4, cout // 4, 3, 1, 1, bias=False)
        self.downsample = None
        if cin != cout:
            self.downsample = nn.Sequential(_bn(cin), nn.ReLU(True), nn.Conv2d(cin, cout, 1, bias=False))
        self._rt = None

    def prepare(self, name, device):
        rt = [(_PreBN(getattr(self, 'bn%d' % i), device),
               _Conv('%s.conv%d' % (name, i), getattr(self, 'conv%d' % i).weight.detach(), None, 1, 1, device)) for i in (1, 2, 3)]
        ds = None
        if self.downsample is not None:
            ds = (_PreBN(self.downsample[0], device), _Conv(name + '.downsample.2', self.downsample[2].weight.detach(), None, 1, 0, device))
        self._rt = (rt, ds)

    def convs(self):
        rt, ds = self._rt
        return [c for _, c in rt] + ([ds[1]] if ds else [])

    def run(self, x):
        from . import style_ops as so
        rt, ds = self._rt
        o1 = rt[0][1].run(rt[0][0].feat(x))
        o2 = rt[1][1].run(rt[1][0].feat(o1))
        o3 = rt[2][1].run(rt[2][0].feat(o2))
        r = x if ds is None else ds[1].run(ds[0].feat(x))
        return so.join(r, o1, o2, o3)


class HourGlass(nn.Module):
    def __init__(self, depth, features):
        super().__init__()
        self.depth = depth
        for level in range(depth, 0, -1):
            for b in ('b1', 'b2', 'b3'):
                self.add_module('%s_%d' % (b, level), ConvBlock(features, features))
        self.add_module('b2_plus_1', ConvBlock(features, features))

    def blocks(self):
        return [(n, m) for n, m in self.named_children()]

    def _level(self, level, x):
        from . import style_ops as so
        up1 = getattr(self, 'b1_%d' % level).run(x)
        low1 = getattr(self, 'b2_%d' % level).run(so.pool2(x))
        low2 = self._level(level - 1, low1) if level > 1 else self.b2_plus_1.run(low1)
        low3 = getattr(self, 'b3_%d' % level).run(low2)
        return so.up2_add(low3, up1)

    def run(self, x):
        return self._level(self.depth, x)


class FAN(nn.Module):
    """face_alignment's FAN(num_modules) with every channel count scaled by width / 256 (tests run narrow ones)."""

    def __init__(self, num_modules=4, width=256, depth=4):
        super().__init__()
        if width % 16 or width < 16:
            raise ValueError('FAN: width %d, served: multiples of 16 (a ConvBlock of width / 4 splits into quarters)' % width)
        self.num_modules, self.width, self.depth = num_modules, width, depth
        c1, c2 = width // 4, width // 2
        self.conv1 = nn.Conv2d(3, c1, 7, 2, 3)
        self.bn1 = _bn(c1)
        self.conv2 = ConvBlock(c1, c2)
        self.conv3 = ConvBlock(c2, c2)
        self.conv4 = ConvBlock(c2, width)
        for i in range(num_modules):
            self.add_module('m%d' % i, HourGlass(depth, width))
            self.add_module('top_m_%d' % i, ConvBlock(width, width))
            self.add_module('conv_last%d' % i, nn.Conv2d(width, width, 1))
            self.add_module('bn_end%d' % i, _bn(width))
            self.add_module('l%d' % i, nn.Conv2d(width, POINTS, 1))
            if i < num_modules - 1:
                self.add_module('bl%d' % i, nn.Conv2d(width, width, 1))
                self.add_module('al%d' % i, nn.Conv2d(POINTS, width, 1))
        self._rt = None

    def _blocks(self):
        out = [('conv2', self.conv2), ('conv3', self.conv3), ('conv4', self.conv4)]
        for i in range(self.num_modules):
            out += [('m%d.%s' % (i, n), b) for n, b in getattr(self, 'm%d' % i).blocks()]
            out.append(('top_m_%d' % i, getattr(self, 'top_m_%d' % i)))
        return out

    def prepare(self, device=None):
        """Make the device-side constants from the current parameters (again after they change)."""
        device = torch.device(device) if device is not None else self.conv1.weight.device
        for name, blk in self._blocks():
            blk.prepare(name, device)
        w, b = fold_post_bn(self.conv1.weight, self.conv1.bias, self.bn1.weight, self.bn1.bias, self.bn1.running_mean, self.bn1.running_var)
        rt = {'stem': _Conv('conv1', w, b, 2, 3, device), 'heads': []}
        for i in range(self.num_modules):
            g = lambda n: getattr(self, n + str(i))                                      # noqa: E731
            bn = g('bn_end')
            w, b = fold_post_bn(g('conv_last').weight, g('conv_last').bias, bn.weight, bn.bias, bn.running_mean, bn.running_var)
            plain = lambda n: _Conv(n + str(i), g(n).weight.detach(), g(n).bias.detach(), 1, 0, device)   # noqa: E731
            rt['heads'].append({'last': _Conv('conv_last%d' % i, w, b, 1, 0, device), 'l': plain('l'),
                                'bl': plain('bl') if i < self.num_modules - 1 else None,
                                'al': plain('al') if i < self.num_modules - 1 else None})
        self._rt = rt
        return self

    def convs(self):
        """every convolution of the prepared network, in forward order of their blocks (for the fall-back listing)"""
        out = [self._rt['stem']]
        for _, blk in self._blocks():
            out += blk.convs()
        for h in self._rt['heads']:
            out += [c for c in (h['last'], h['l'], h['bl'], h['al']) if c is not None]
        return out

    def forward(self, x):
        """(B, 3, H, W) fp32 in [0, 1] on the device, H and W multiples of 4 * 2^depth -> the LAST stack's heat maps
        (B, 68, H / 4, W / 4)."""
        from . import style_ops as so
        if self._rt is None:
            raise RuntimeError('FAN: call prepare() after loading the parameters')
        ops._require_device(x, 'FAN input')
        unit = 4 << self.depth
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] % unit or x.shape[3] % unit:
            raise ValueError('FAN: input %s, served: (B, 3, H, W) with H and W multiples of %d' % (tuple(x.shape), unit))
        with torch.no_grad():
            x = self._rt['stem'].run(Feat(x), ACT_RELU)
            x = so.pool2(self.conv2.run(x))
            previous = self.conv4.run(self.conv3.run(x))
            for i, h in enumerate(self._rt['heads']):
                ll = getattr(self, 'top_m_%d' % i).run(getattr(self, 'm%d' % i).run(previous))
                ll = h['last'].run(Feat(ll), ACT_RELU)
                maps = h['l'].run(Feat(ll))
                if h['bl'] is not None:
                    previous = so.sum3(previous, h['bl'].run(Feat(ll)), h['al'].run(Feat(maps)))
            return maps


def seeded_state_dict(num_modules=4, width=256, depth=4, seed=0):
    """A state_dict with non-trivial BatchNorm statistics (benchmarks and tests; the published checkpoint is not here):
    convolution weights ~ N(0, 1.5 / fan_in), BatchNorm g in 0.5 .. 1.5, b and mu ~ 0.1 N(0, 1), var in 0.5 .. 1.5."""
    net = FAN(num_modules, width, depth)
    gen = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in net.state_dict().items():
        if k.endswith('num_batches_tracked'):
            continue
        if v.dim() == 4:
            fan_in = v.shape[1] * v.shape[2] * v.shape[3]
            sd[k] = torch.randn(v.shape, generator=gen) * (1.5 / fan_in) ** 0.5
        elif k.endswith('running_var') or (k.endswith('.weight') and _is_bn_key(k, net)):
            sd[k] = 0.5 + torch.rand(v.shape, generator=gen)
        else:
            sd[k] = 0.1 * torch.randn(v.shape, generator=gen)
    return sd


def _is_bn_key(key, net):
    mod = net
    for part in key.split('.')[:-1]:
        mod = getattr(mod, part) if not part.isdigit() else mod[int(part)]
    return isinstance(mod, nn.BatchNorm2d)


def architecture_of(sd):
    """(num_modules, width, depth) a face_alignment FAN state_dict was saved from"""
    stacks = {int(m.group(1)) for k in sd for m in [re.match(r'l(\d+)\.weight$', k)] if m}
    levels = {int(m.group(1)) for k in sd for m in [re.match(r'm0\.b1_(\d+)\.', k)] if m}
    if not stacks or not levels or 'l0.weight' not in sd:
        raise ValueError('load_fan: no FAN state_dict (it has no l<i>.weight / m0.b1_<level> entries); first keys: %s' % sorted(sd)[:5])
    return max(stacks) + 1, int(sd['l0.weight'].shape[1]), max(levels)


def read_state_dict(path):
    """A plain state_dict (.pth / .pth.tar, possibly under 'state_dict') or that of a TorchScript archive."""
    scripted = False
    if zipfile.is_zipfile(path):
        with zipfile.ZipFile(path) as z:
            scripted = any('/code/' in n or n.endswith('constants.pkl') for n in z.namelist())
    if scripted:
        sd = torch.jit.load(path, map_location='cpu').state_dict()
    else:
        sd = torch.load(path, map_location='cpu', weights_only=True)
        if isinstance(sd, dict) and 'state_dict' in sd and not torch.is_tensor(sd['state_dict']):
            sd = sd['state_dict']
    return {k: v for k, v in sd.items() if not k.endswith('num_batches_tracked')}


def load_fan(path, device):
    """The FAN of the checkpoint at ``path``, prepared on ``device``.  Strict: missing or unexpected keys are an error that
    names them (num_batches_tracked entries aside)."""
    sd = read_state_dict(path)
    net = FAN(*architecture_of(sd))
    own = {k for k in net.state_dict() if not k.endswith('num_batches_tracked')}
    missing, unexpected = sorted(own - set(sd)), sorted(set(sd) - own)
    if missing or unexpected:
        raise RuntimeError('load_fan: %s does not hold a FAN(num_modules=%d, width=%d, depth=%d): missing keys %s, unexpected keys %s'
                           % (path, net.num_modules, net.width, net.depth, missing, unexpected))
    net.load_state_dict(sd, strict=False)               # (the counters num_batches_tracked stay at their initial value)
    return net.to(device).eval().prepare(device)
