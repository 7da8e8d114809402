"""Reference of the static cartoon generator and of the libapstyle.so kernels -- a plain helper module of the tests, CPU only.

``generator_forward`` restates ``ResnetGenerator(ngf, img_size, light=True)`` of the Photo2Cartoon project (the U-GAT-IT-style
generator the streaming-inference model uses for experiment names that contain 'cartoon') from its formulas, as a function of a
state dict with that class's key names; evaluated in float64 it is what the HIP path is compared with.  The recorded outputs of the
class itself (tests/golden/photo2cartoon.npz, written by tests/golden/make_photo2cartoon_golden.py) pin this restatement.

``lin`` / ``lin_coeffs`` restate LIN and adaLIN (both are ``rho IN(x) + (1 - rho) LN(x)`` with UNBIASED variances, scaled and
shifted), ``join`` / ``pool2`` / ``up2_add`` / ``sum3`` / ``instnorm_stats`` the hourglass's element-wise producers, and
``quantize_u8`` the uint8 round trip of the photo.  ``param_shapes`` lists the keys in state_dict order, ``init_params`` draws
seeded weights under which no part of the net is asleep."""
import math

import torch
import torch.nn.functional as F

EPS = 1e-5


# ------------------------------------------------------------------------------------------------------------ kernels
def lin_moments(x):
    """(mean_in, var_in) per plane and (mean_ln, var_ln) per sample, variances unbiased (torch.var's default)."""
    return (x.mean(dim=(2, 3), keepdim=True), x.var(dim=(2, 3), keepdim=True),
            x.mean(dim=(1, 2, 3), keepdim=True), x.var(dim=(1, 2, 3), keepdim=True))


def lin(x, rho, gamma, beta, eps=EPS):
    """LIN (gamma / beta of shape [C]) or adaLIN ([N, C]) as the layer is written: normalise, mix, scale, shift."""
    n, c = x.shape[:2]
    mi, vi, ml, vl = lin_moments(x)
    rho = rho.reshape(1, c, 1, 1).to(x.dtype)
    out = rho * (x - mi) / torch.sqrt(vi + eps) + (1 - rho) * (x - ml) / torch.sqrt(vl + eps)
    gamma = gamma.to(x.dtype).reshape(-1, c, 1, 1)
    beta = beta.to(x.dtype).reshape(-1, c, 1, 1)
    return out * gamma + beta


def lin_coeffs(x, rho, gamma, beta, eps=EPS):
    """The same layer folded to (a, b) of shape [N, C]: lin(x) = a x + b."""
    n, c = x.shape[:2]
    mi, vi, ml, vl = (t.reshape(n, -1) for t in lin_moments(x))
    rho = rho.reshape(1, c).to(x.dtype)
    gamma = gamma.to(x.dtype).reshape(-1, c)
    beta = beta.to(x.dtype).reshape(-1, c)
    ri, rl = 1 / torch.sqrt(vi + eps), 1 / torch.sqrt(vl + eps)
    a = gamma * (rho * ri + (1 - rho) * rl)
    b = beta - gamma * (rho * mi * ri + (1 - rho) * ml * rl)
    return a.expand(n, c), b.expand(n, c)


def affine_apply(x, a, b, relu=False, residual=None):
    n, c = x.shape[:2]
    y = a.reshape(n, c, 1, 1).to(x.dtype) * x + b.reshape(n, c, 1, 1).to(x.dtype)
    if relu:
        y = torch.relu(y)
    return y if residual is None else y + residual


def instnorm_stats(y, eps=EPS):
    """Biased InstanceNorm2d statistics (mean, rstd) of shape [N * C]."""
    m = y.mean(dim=(2, 3))
    v = y.var(dim=(2, 3), unbiased=False)
    return m.reshape(-1), (1 / torch.sqrt(v + eps)).reshape(-1)


def join(r, p0, p1, p2):
    return r + torch.cat((p0, p1, p2), 1)


def pool2(x):
    return F.avg_pool2d(x, 2)


def up2_add(x, skip=None):
    up = F.interpolate(x, scale_factor=2, mode='nearest')
    return up if skip is None else skip + up


def sum3(x, a, b):
    return x + a + b


def quantize_u8(x):
    """floor((x + 1) 127.5) / 127.5 - 1 in float32, the byte clamped to [0, 255]."""
    return torch.floor((x.float() + 1) * 127.5).clamp(0, 255) / 127.5 - 1


# ------------------------------------------------------------------------------------------------------------ the generator
def _conv_block_shapes(p, cin, cout):
    return [(p + '.ConvBlock1.3.weight', (cout // 2, cin, 3, 3)), (p + '.ConvBlock2.3.weight', (cout // 4, cout // 2, 3, 3)),
            (p + '.ConvBlock3.3.weight', (cout // 4, cout // 4, 3, 3)), (p + '.ConvBlock4.2.weight', (cout, cin, 1, 1))]


def _hourglass_shapes(p, g, use_res):
    s = []
    for name in ('1_1', '1_2', '2_1', '2_2', '3_1', '3_2', '4_1', '4_2', '5', '6', '7', '8', '9'):
        s += _conv_block_shapes('%s.HG.0.ConvBlock%s' % (p, name), g, g)
    s += _conv_block_shapes(p + '.HG.1', g, g)
    s += [(p + '.HG.2.weight', (g, g, 1, 1)), (p + '.Conv1.weight', (3, g, 1, 1)), (p + '.Conv1.bias', (3,))]
    if use_res:
        s += [(p + '.Conv2.weight', (g, g, 1, 1)), (p + '.Conv2.bias', (g,)), (p + '.Conv3.weight', (g, 3, 1, 1)),
              (p + '.Conv3.bias', (g,))]
    return s


def _linear_shapes(p, cin, cout):
    return [(p + '.weight', (cout, cin)), (p + '.bias', (cout,))]


def _soft_adalin_shapes(p, c):
    s = [(p + '.w_gamma', (1, c)), (p + '.w_beta', (1, c)), (p + '.norm.rho', (1, c, 1, 1))]
    for m in ('c_gamma', 'c_beta'):
        s += _linear_shapes('%s.%s.0' % (p, m), c, c) + _linear_shapes('%s.%s.2' % (p, m), c, c)
    return s + _linear_shapes(p + '.s_gamma', c, c) + _linear_shapes(p + '.s_beta', c, c)


def param_shapes(ngf):
    """[(key, shape)] of ResnetGenerator(ngf, light=True).state_dict(), in its order."""
    g, d = ngf, ngf * 4
    s = [('ConvBlock1.1.weight', (g, 3, 7, 7))]
    s += _hourglass_shapes('HourGlass1', g, True) + _hourglass_shapes('HourGlass2', g, True)
    s += [('DownBlock1.1.weight', (2 * g, g, 3, 3)), ('DownBlock2.1.weight', (d, 2 * g, 3, 3))]
    for i in range(1, 5):
        s += [('EncodeBlock%d.conv_block.1.weight' % i, (d, d, 3, 3)), ('EncodeBlock%d.conv_block.5.weight' % i, (d, d, 3, 3))]
    s += _linear_shapes('gap_fc', d, 1) + _linear_shapes('gmp_fc', d, 1)
    s += [('conv1x1.weight', (d, 2 * d, 1, 1)), ('conv1x1.bias', (d,))]
    s += _linear_shapes('FC.0', d, d) + _linear_shapes('FC.2', d, d)
    for i in range(1, 5):
        p = 'DecodeBlock%d' % i
        s += [(p + '.conv1.weight', (d, d, 3, 3))] + _soft_adalin_shapes(p + '.norm1', d)
        s += [(p + '.conv2.weight', (d, d, 3, 3))] + _soft_adalin_shapes(p + '.norm2', d)
    for p, cin, cout in (('UpBlock1', d, 2 * g), ('UpBlock2', 2 * g, g)):
        s += [(p + '.2.weight', (cout, cin, 3, 3))] + [('%s.3.%s' % (p, k), (1, cout, 1, 1)) for k in ('rho', 'gamma', 'beta')]
    s += _hourglass_shapes('HourGlass3', g, True) + _hourglass_shapes('HourGlass4', g, False)
    return s + [('ConvBlock2.1.weight', (3, 3, 7, 7))]


def init_params(shapes, seed, gain=1.5):
    """Seeded weights with every path of the net awake; draw order == ``shapes`` order, on a dedicated CPU generator.
    rho, w_gamma, w_beta ~ U[0, 1] (w_* = 0, the class's default, would switch the content path off); LIN gamma ~ U[0.5, 1.5],
    LIN beta ~ N(0, 0.3); biases ~ N(0, 0.1); convolution and linear weights ~ N(0, gain / sqrt(fan_in))."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for key, shape in shapes:
        t = torch.empty(shape, dtype=torch.float32)
        last = key.rsplit('.', 1)[-1]
        if last in ('rho', 'w_gamma', 'w_beta'):
            t.uniform_(0, 1, generator=g)
        elif last == 'gamma':
            t.uniform_(0.5, 1.5, generator=g)
        elif last == 'beta':
            t.normal_(0.0, 0.3, generator=g)
        elif last == 'bias':
            t.normal_(0.0, 0.1, generator=g)
        else:
            t.normal_(0.0, gain / math.sqrt(t[0].numel()), generator=g)
        sd[key] = t
    return sd


def _in_relu(x):
    return torch.relu(F.instance_norm(x, eps=EPS))


def _rconv(x, w, pad, stride=1):
    return F.conv2d(F.pad(x, (pad,) * 4, mode='reflect'), w, stride=stride)


def _conv_block(sd, p, x):
    x1 = _rconv(_in_relu(x), sd[p + '.ConvBlock1.3.weight'], 1)
    x2 = _rconv(_in_relu(x1), sd[p + '.ConvBlock2.3.weight'], 1)
    x3 = _rconv(_in_relu(x2), sd[p + '.ConvBlock3.3.weight'], 1)
    r = x if x.shape[1] == sd[p + '.ConvBlock4.2.weight'].shape[0] else F.conv2d(_in_relu(x), sd[p + '.ConvBlock4.2.weight'])
    return join(r, x1, x2, x3)


def _hourglass(sd, p, x, use_res):
    b = p + '.HG.0.ConvBlock'
    skips, down = [], x
    for lvl in '1234':
        skips.append(_conv_block(sd, b + lvl + '_1', down))
        down = _conv_block(sd, b + lvl + '_2', pool2(down))
    up = _conv_block(sd, b + '5', down)
    for name, skip in zip('6789', reversed(skips)):
        up = up2_add(_conv_block(sd, b + name, up), skip)
    ll = _in_relu(F.conv2d(_conv_block(sd, p + '.HG.1', up), sd[p + '.HG.2.weight']))
    tmp = F.conv2d(ll, sd[p + '.Conv1.weight'], sd[p + '.Conv1.bias'])
    if not use_res:
        return tmp
    return sum3(x, F.conv2d(ll, sd[p + '.Conv2.weight'], sd[p + '.Conv2.bias']), F.conv2d(tmp, sd[p + '.Conv3.weight'], sd[p + '.Conv3.bias']))


def _mlp(sd, p, x):
    return F.linear(torch.relu(F.linear(x, sd[p + '.0.weight'], sd[p + '.0.bias'])), sd[p + '.2.weight'], sd[p + '.2.bias'])


def _soft_adalin(sd, p, x, content, style):
    sg = F.linear(style, sd[p + '.s_gamma.weight'], sd[p + '.s_gamma.bias'])
    sb = F.linear(style, sd[p + '.s_beta.weight'], sd[p + '.s_beta.bias'])
    wg, wb = sd[p + '.w_gamma'], sd[p + '.w_beta']
    gamma = (1 - wg) * sg + wg * _mlp(sd, p + '.c_gamma', content)
    beta = (1 - wb) * sb + wb * _mlp(sd, p + '.c_beta', content)
    return lin(x, sd[p + '.norm.rho'], gamma, beta)


def generator_forward(sd, x, dtype=torch.float64, device='cpu'):
    """The tanh image (N, 3, H, W) of the generator with parameters ``sd`` for the input ``x``, evaluated in ``dtype`` on
    ``device`` (the tests: float64 on the CPU; tools/bench_cartoon_static.py: float32 through the stock operators on the GPU)."""
    sd = {k: v.detach().to(device, dtype) for k, v in sd.items()}
    x = x.detach().to(device, dtype)
    with torch.no_grad():
        x = _in_relu(_rconv(x, sd['ConvBlock1.1.weight'], 3))
        x = _hourglass(sd, 'HourGlass1', x, True)
        x = _hourglass(sd, 'HourGlass2', x, True)
        x = _in_relu(_rconv(x, sd['DownBlock1.1.weight'], 1, 2))
        x = _in_relu(_rconv(x, sd['DownBlock2.1.weight'], 1, 2))
        content = []
        for i in range(1, 5):
            p = 'EncodeBlock%d.conv_block' % i
            y = _in_relu(_rconv(x, sd[p + '.1.weight'], 1))
            x = x + F.instance_norm(_rconv(y, sd[p + '.5.weight'], 1), eps=EPS)
            content.append(x.mean(dim=(2, 3)))
        c = x.shape[1]
        cam = torch.cat((x * sd['gap_fc.weight'].view(1, c, 1, 1), x * sd['gmp_fc.weight'].view(1, c, 1, 1)), 1)
        x = torch.relu(F.conv2d(cam, sd['conv1x1.weight'], sd['conv1x1.bias']))
        style = torch.relu(_mlp(sd, 'FC', x.mean(dim=(2, 3))))
        for i, cf in zip(range(1, 5), reversed(content)):
            p = 'DecodeBlock%d' % i
            y = torch.relu(_soft_adalin(sd, p + '.norm1', _rconv(x, sd[p + '.conv1.weight'], 1), cf, style))
            x = x + _soft_adalin(sd, p + '.norm2', _rconv(y, sd[p + '.conv2.weight'], 1), cf, style)
        for p in ('UpBlock1', 'UpBlock2'):
            y = _rconv(up2_add(x), sd[p + '.2.weight'], 1)
            x = torch.relu(lin(y, sd[p + '.3.rho'], sd[p + '.3.gamma'], sd[p + '.3.beta']))
        x = _hourglass(sd, 'HourGlass3', x, True)
        x = _hourglass(sd, 'HourGlass4', x, False)
        return torch.tanh(_rconv(x, sd['ConvBlock2.1.weight'], 3))
