"""GPU (-m gpu): every kernel csrc/instnorm_bwd.hip and csrc/act_bwd.hip can launch for ap_instnorm_bwd, ap_act_bwd, ap_act_bwd_bias, ap_bias_grad
and ap_bias_grad_ws, against fp64 autograd / fp64 sums, at the shapes where the dispatch changes kernels.

Each case states the route it is meant for and first asserts that ap_instnorm_bwd_route / ap_act_bwd_route name it, so the list
cannot drift off its kernels.  The C API is called through ctypes: every output (dy, db, the workspaces) is a NaN-filled window
between sentinel guards; after a call the guards are intact and the window is finite (the kernels load from clamped indices and mask
their stores: this checks the masks).  Every case has three or more planes with their own mean and scale, so a wrong plane stride --
the padded stride (H + 2p)(W + 2p) of g1 included -- moves the result.

The inputs are built on the CPU by the functions below; tests/test_elementwise_routes_cpu.py imports them and checks, without a GPU,
that every case's normalised activations stay away from the activation's kink and that the fp32 formula meets the bars used here.

Tolerances (the project's own, tests/test_gpu_parity.py): 2e-5 max|dy| for instnorm_bwd, 1e-5 max|dy| for act_bwd -- asserted per
plane here, which is stricter for the planes with a small gradient; 2e-6 sum|dy_c| for the one-pass bias gradient; the bf16 store is
bit-equal to the rounded fp32 route (tests/test_bf16_gpu.py::test_stem_gradient_stored_as_bf16).  The bare bias sum has no bar in the
project: 4 e_ref + 1e-6 sum|dy_c| with e_ref = |torch's fp32 CPU sum - fp64 sum|.  Measured on the MI355X, both relative to sum|dy_c|, worst channel (e_ref / kernel):
(2, 3, 1000) 3.0e-8 / 6.2e-8; (1, 1, 1) 0 / 0; C = 1024 of 2 x 2: 1.2e-7 / 1.0e-7; two-stage (1, 1, 65536) 5.1e-9 / 5.1e-9;
(2, 3, 12293) 4.4e-8 / 4.4e-8; (1, 1, 8191) 1.3e-8 / 1.3e-8; (2, 256, 8192) 1.4e-7 / 1.4e-7; (4, 200, 16) 1.2e-7 / 1.1e-7 -- the
1e-6 term is some eight ulp of the summed magnitudes.  No instnorm_bwd / act_bwd case needed more than the existing bars: the worst
plane is at 3.5e-7 max|dy| (2 x 2) resp. 1.2e-7 max|dy|."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from conftest import linf

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 4096, -7777.0
NAN = float('nan')
SCALES, OFFSETS = (0.3, 1.3, 4.0), (-2.0, 0.4, 7.0)        # per plane: y * scale + offset
ACT_SCALES, ACT_OFFSETS = (0.3, 1.3, 4.0), (-0.1, 0.4, 1.0)    # pre-activations of act_bwd: both signs in every plane
AP_ERR_INVALID, AP_ERR_UNSUPPORTED = -1, -2


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    return torch.device('cuda:0')


# ---------------------------------------------------------------- case lists

def route_name(base, two):
    """the name the route functions give a form that is instantiated with / without a second gradient"""
    if not two or base.split('<')[0] not in ('small', 'vec', 'fold1'):
        return base
    return 'small<g2>' if base == 'small' else base[:-1] + ',g2>'


def _inbwd_cases():
    rows = []

    def add(base, h, w, pad=0, g2=(False, True), act=None, nc=3):
        for two in g2:
            rows.append((route_name(base, two), h, w, pad, len(rows) % 3 if act is None else act, two, nc))
    add('small', 1, 1, g2=(False,), act=0)                  # x^ = 0, dy = 0 exactly
    add('small', 3, 3, g2=(False,))
    add('small', 31, 31)                                    # the PatchGAN's maps
    add('small', 1, 1023, g2=(True,))                       # one short of the vector kernel
    add('vec<256>', 2, 2)                                   # Q = 1: every lane but one clamps to group 0
    add('vec<256>', 40, 36, nc=5)
    add('vec<256>', 64, 64)                                 # no idle lane
    add('vec<1024>', 41, 100)                               # 4100: the smallest
    add('vec<1024>', 128, 128)
    add('fold1<256>', 3, 8, 1)                              # rows 1 and H - 2 coincide, minimal W
    add('fold1<256>', 5, 12, 1)
    add('fold1<256>', 64, 64, 1)
    add('fold1<1024>', 65, 64, 1)
    add('fold1<1024>', 128, 128, 1)
    add('general<256>', 25, 41, 0, g2=(True,))              # odd H W > 1024
    add('general<256>', 30, 30, 1, g2=(False,))
    add('general<256>', 5, 4, 1, g2=(True,))                # W = 4: both column borders in one group
    add('general<256>', 2, 8, 1, g2=(False,))               # H < 3
    add('general<256>', 9, 10, 2, g2=(True,))
    add('general<256>', 40, 44, 3, g2=(False,))
    add('general<1024>', 65, 65, 0, g2=(True,))
    add('general<1024>', 70, 70, 1, g2=(False,))
    add('general<1024>', 96, 96, 3, g2=(True,))
    add('general<1024>', 127, 129, 0, g2=(False,))          # 16383
    add('big', 4097, 4)                                     # 16388: the smallest, one group per row
    add('big', 132, 128)
    add('big', 256, 256)
    add('big<fold>', 132, 128, 1, g2=(True,))
    add('big<fold>', 256, 256, 1, g2=(False,))
    add('big<fold>', 130, 128, 2, g2=(True,))
    add('big<fold>', 256, 256, 3, g2=(False,))
    add('big<fold>', 2100, 8, 3, g2=(True,))                # W < 4 + 2 p: the per-pixel FoldReader fallback
    add('reduce_apply', 130, 127, 0, g2=(False,))
    add('reduce_apply', 130, 127, 1, g2=(True,))
    add('reduce_apply', 130, 127, 3, g2=(False,))
    add('reduce_apply', 257, 256, 0, g2=(False,))           # 65792: beyond the big kernel, 16-byte lanes
    add('reduce_apply', 300, 300, 0, g2=(True,))            # the apply grid at its cap of 32
    return rows


# (route, H, W, fold pad, act, second gradient, planes)
INBWD_CASES = _inbwd_cases()
# the bf16 store: (route, H, W, act, second gradient, planes) -- unfolded by definition
INBWD_BF16_CASES = [('big<bf16>', 132, 128, 1, False, 3), ('big<bf16>', 256, 256, 2, True, 3)]

# (route, H, W, fold pad, act, second gradient, planes, out given)
ACT_CASES = [
    ('act_fold1', 3, 4, 1, 1, True, 3, True),
    ('act_fold1', 64, 64, 1, 2, False, 4, True),
    ('act_fold1', 256, 256, 1, 3, True, 3, True),
    ('act_fold1', 5, 8, 1, 0, True, 3, True),
    ('act_generic', 16, 16, 0, 2, True, 3, True),           # 16-byte lanes
    ('act_generic', 256, 256, 0, 3, False, 3, True),        # the generator's tanh output: the strided loop, H W > 32768
    ('act_generic', 182, 184, 0, 1, True, 3, True),         # 33488: the second sweep is partial
    ('act_generic', 9, 10, 2, 1, True, 3, True),            # element-wise with the fold
    ('act_generic', 12, 16, 3, 0, True, 3, True),
    ('act_generic', 182, 181, 3, 2, False, 3, True),        # 32942: strided loop with a fold
    ('act_generic', 9, 10, 2, 0, True, 3, False),           # act NONE, out = NULL: the fold-and-add form
]

# ap_act_bwd_bias: (N, C, H, W, fold pad, act, second gradient)
ACT_BIAS_CASES = [(2, 3, 256, 256, 0, 3, False), (2, 3, 182, 181, 3, 2, True), (2, 3, 70, 61, 0, 1, True)]

# ap_bias_grad_ws: (N, C, HW, expected split)
BIAS_WS_CASES = [(1, 1, 65536, 16), (2, 3, 12293, 3), (1, 1, 8191, 1), (2, 256, 8192, 1), (4, 200, 16, 1)]
BIAS_DIRECT_CASES = [(2, 3, 1000), (1, 1, 1)]


def inbwd_id(case):
    return '%s %dx%d p%d act%d%s' % (case[0], case[1], case[2], case[3], case[4], ' g2' if case[5] else '')


# ---------------------------------------------------------------- inputs and references (CPU)

def _plane_affine(t, scales, offsets):
    nc = t.shape[1]
    s = torch.tensor([scales[i % 3] for i in range(nc)], dtype=t.dtype).view(1, nc, 1, 1)
    o = torch.tensor([offsets[i % 3] for i in range(nc)], dtype=t.dtype).view(1, nc, 1, 1)
    return t * s + o


def plane_stats(y32):
    """mean and sqrt(var + eps) of every plane of an fp32 tensor, in fp64"""
    yd = y32.double()
    return yd.mean((2, 3), keepdim=True), torch.sqrt(yd.var((2, 3), unbiased=False, keepdim=True) + 1e-5)


def xhat_min(y32):
    m, s = plane_stats(y32)
    return float(((y32.double() - m) / s).abs().min())


def off_the_kink(y32):
    """Move every element with |x^| < 2e-3 to |x^| = 4e-3 (sign kept) and recompute the statistics, until none is left: whether an
    fp32 x^ of 1e-7 and its fp64 value fall on the same side of ReLU's kink is then not left to the seed."""
    if y32.shape[2] * y32.shape[3] == 1:
        return y32                                           # x^ = 0 by definition (used with act NONE only)
    for _ in range(16):
        m, s = plane_stats(y32)
        xh = (y32.double() - m) / s
        near = xh.abs() < 2e-3
        if not bool(near.any()):
            break
        sign = torch.where(xh < 0, -1.0, 1.0).double()
        y32 = torch.where(near, m + sign * 4e-3 * s, y32.double()).float()
    return y32


def _act(x, act):
    return x if act == 0 else (F.relu(x) if act == 1 else (F.leaky_relu(x, 0.2) if act == 2 else torch.tanh(x)))


def fold_sum(g1, pad, g2, dtype=torch.float64):
    """fold(g1) + g2 in `dtype`: the gradient of sum(reflection_pad(z) * g1) + sum(z * g2) w.r.t. z"""
    n, c, hp, wp = g1.shape
    z = torch.zeros(n, c, hp - 2 * pad, wp - 2 * pad, dtype=dtype, requires_grad=True)
    zp = F.pad(z, (pad,) * 4, mode='reflect') if pad else z
    loss = (zp * g1.to(dtype)).sum()
    if g2 is not None:
        loss = loss + (z * g2.to(dtype)).sum()
    loss.backward()
    return z.grad


@functools.lru_cache(maxsize=None)
def inbwd_problem(h, w, pad, act, two, nc):
    """inputs of ap_instnorm_bwd (fp32) and the fp64 autograd gradient through act(instance_norm(y)) [and ReflectionPad2d]"""
    gen = torch.Generator().manual_seed(100003 * h + 101 * w + 7 * pad + 3 * act + int(two))
    y = off_the_kink(_plane_affine(torch.randn(1, nc, h, w, generator=gen, dtype=torch.float64), SCALES, OFFSETS).float())
    g1 = torch.randn(1, nc, h + 2 * pad, w + 2 * pad, generator=gen)
    g2 = torch.randn(1, nc, h, w, generator=gen) if two else None
    m, s = plane_stats(y)
    yv = y.double().requires_grad_(True)
    if h * w > 1:
        xh = F.instance_norm(yv)
    else:       # (F.instance_norm refuses one-element planes: the same function written out)
        xh = (yv - yv.mean((2, 3), keepdim=True)) * torch.rsqrt(yv.var((2, 3), unbiased=False, keepdim=True) + 1e-5)
    out = _act(xh, act)
    outp = F.pad(out, (pad,) * 4, mode='reflect') if pad else out
    ((outp * g1.double()).sum() + ((out * g2.double()).sum() if two else 0.0)).backward()
    return {'y': y, 'g1': g1, 'g2': g2, 'mean': m.reshape(-1).float(), 'rstd': (1.0 / s).reshape(-1).float(), 'ref': yv.grad.detach()}


def inbwd_formula_fp32(p, pad, act):
    """dy = rstd (g' - mean g' - x^ mean(g' x^)), g' = (fold(g1) + g2) act'(x^), evaluated in fp32 on the CPU"""
    y, m, r = p['y'], p['mean'].view(1, -1, 1, 1), p['rstd'].view(1, -1, 1, 1)
    xh = (y - m) * r
    g = fold_sum(p['g1'], pad, p['g2'], torch.float32)
    if act == 1:
        g = g * (xh > 0).float()
    elif act == 2:
        g = g * torch.where(xh > 0, 1.0, 0.2).float()
    a1, a2 = g.mean((2, 3), keepdim=True), (g * xh).mean((2, 3), keepdim=True)
    return r * (g - a1 - xh * a2)


@functools.lru_cache(maxsize=None)
def act_problem(n, c, h, w, pad, act, two, with_out=True):
    """inputs of ap_act_bwd (fp32) and dy = (fold(g1) + g2) act'(out) in fp64 from the SAME stored fp32 `out` the kernel reads:
    out > 0 decides ReLU / LeakyReLU (exact zeros and a negative zero included), 1 - out^2 is tanh's derivative."""
    gen = torch.Generator().manual_seed(7919 * h + 13 * w + 5 * pad + act + 2 * int(two) + 17 * n)
    pre = _plane_affine(torch.randn(1, n * c, h, w, generator=gen, dtype=torch.float64), ACT_SCALES, ACT_OFFSETS)
    out = _act(pre, act).float().reshape(n, c, h, w)
    if act in (1, 2):
        flat = out.view(-1)
        flat[::5] = 0.0
        flat[1::11] = -0.0
    g1 = torch.randn(n, c, h + 2 * pad, w + 2 * pad, generator=gen)
    g2 = torch.randn(n, c, h, w, generator=gen) if two else None
    g = fold_sum(g1, pad, g2)
    od = out.double()
    if act == 1:
        ref = g * (od > 0).double()
    elif act == 2:
        ref = g * torch.where(od > 0, 1.0, 0.2).double()
    elif act == 3:
        ref = g * (1.0 - od * od)
    else:
        ref = g
    return {'out': out if with_out else None, 'g1': g1, 'g2': g2, 'ref': ref}


def bias_problem(n, c, hw):
    """dy = 3 randn + a per-channel offset: a dropped or doubled slice moves db by far more than rounding"""
    gen = torch.Generator().manual_seed(31 * n + 7 * c + hw)
    dy = torch.randn(n, c, hw, generator=gen) * 3.0 + (2.0 + torch.arange(c, dtype=torch.float32) % 7).view(1, c, 1)
    ref = dy.double().sum((0, 2))
    e_ref = (dy.sum((0, 2)).double() - ref).abs()
    return dy, ref, e_ref, dy.double().abs().sum((0, 2))


# ---------------------------------------------------------------- harness

class Window:
    """`count` elements of NaN between two guards of GUARD sentinels"""

    def __init__(self, dev, count, dtype=torch.float32):
        self.count = count
        self.buf = torch.full((count + 2 * GUARD,), SENTINEL, dtype=dtype, device=dev)
        self.buf[GUARD:GUARD + count] = NAN
        self.sentinel = float(torch.tensor(SENTINEL, dtype=dtype))
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + GUARD * self.buf.element_size())

    @property
    def data(self):
        return self.buf[GUARD:GUARD + self.count]

    def guards_intact(self):
        return bool((self.buf[:GUARD] == self.sentinel).all()) and bool((self.buf[GUARD + self.count:] == self.sentinel).all())

    def finite(self):
        return bool(torch.isfinite(self.data).all())

    def untouched(self):
        return bool(torch.isnan(self.data).all())


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _lib():
    from animateportrait_amd import _capi
    return _capi.lib()


def _route(fn, *args):
    buf = ctypes.create_string_buffer(64)
    rc = fn(*args, buf, 64)
    return rc, buf.value.decode()


def _to(dev, *ts):
    return [None if t is None else t.contiguous().to(dev) for t in ts]


def call_instnorm_bwd(dev, p, pad, act_bits, nc, h, w, bf16=False, spoil=None):
    """(rc, dy window, workspace window); spoil: argument name -> replacement (refusal tests)"""
    keep = dict(zip(('g1', 'g2', 'y', 'mean', 'rstd'), _to(dev, p['g1'], p['g2'], p['y'], p['mean'], p['rstd'])))
    keep.update(spoil or {})
    dy = Window(dev, nc * h * w, torch.bfloat16 if bf16 else torch.float32)
    ws = Window(dev, nc * 2)
    rc = _lib().ap_instnorm_bwd(_p(keep['g1']), pad, _p(keep['g2']), _p(keep['y']), _p(keep['mean']), _p(keep['rstd']), act_bits,
                                nc, h, w, ws.ptr, dy.ptr, _stream(dev))
    torch.cuda.synchronize(dev)
    return rc, dy, ws


def call_act_bwd(dev, p, pad, act, nc, h, w):
    g1, g2, out = _to(dev, p['g1'], p['g2'], p['out'])
    dy = Window(dev, nc * h * w)
    rc = _lib().ap_act_bwd(_p(g1), pad, _p(g2), _p(out), act, nc, h, w, dy.ptr, _stream(dev))
    torch.cuda.synchronize(dev)
    return rc, dy


def per_plane_errors(got, ref):
    """[(L-inf error, max |ref|)] per plane of (.., H, W) tensors"""
    g, r = got.detach().double().cpu().reshape(-1, ref.shape[-2] * ref.shape[-1]), ref.double().reshape(-1, ref.shape[-2] * ref.shape[-1])
    return list(zip((g - r).abs().max(1).values.tolist(), r.abs().max(1).values.tolist()))


# ---------------------------------------------------------------- ap_instnorm_bwd

@pytest.mark.parametrize('case', INBWD_CASES, ids=inbwd_id)
def test_instnorm_bwd_on_its_route(dev, case):
    route, h, w, pad, act, two, nc = case
    lib = _lib()
    assert _route(lib.ap_instnorm_bwd_route, pad, int(two), act, h, w) == (0, route)
    p = inbwd_problem(h, w, pad, act, two, nc)
    rc, dy, ws = call_instnorm_bwd(dev, p, pad, act, nc, h, w)
    assert rc == 0, lib.ap_last_error()
    assert dy.guards_intact() and ws.guards_intact()
    assert dy.finite()
    # the plane sums go through the workspace on the reduce / apply route only
    assert ws.finite() if route == 'reduce_apply' else ws.untouched()
    got = dy.data.view(1, nc, h, w)
    if h * w == 1:
        assert bool((got == 0).all()) and bool((p['ref'] == 0).all())
        return
    errs = per_plane_errors(got, p['ref'])
    print('instnorm_bwd', inbwd_id(case), 'worst plane error / max|dy| = %.3g' % max(e / s for e, s in errs))
    for e, s in errs:
        assert e < 2e-5 * s, (e, s)
    assert linf(got, p['ref']) < 2e-5 * float(p['ref'].abs().max())


@pytest.mark.parametrize('case', INBWD_BF16_CASES, ids=lambda c: '%s %dx%d act%d%s' % (c[0], c[1], c[2], c[3], ' g2' if c[4] else ''))
def test_instnorm_bwd_bf16_store(dev, case):
    """dy stored as bf16 (act bit 8): pack_bf16x2 converts with (__bf16), round to nearest even -- the bits of the fp32 route's dy
    rounded by torch, which itself meets the fp32 bar."""
    route, h, w, act, two, nc = case
    lib = _lib()
    assert _route(lib.ap_instnorm_bwd_route, 0, int(two), act | 0x100, h, w) == (0, route)
    assert _route(lib.ap_instnorm_bwd_route, 0, int(two), act, h, w) == (0, 'big')
    p = inbwd_problem(h, w, 0, act, two, nc)
    rc32, dy32, ws32 = call_instnorm_bwd(dev, p, 0, act, nc, h, w)
    rc16, dy16, ws16 = call_instnorm_bwd(dev, p, 0, act | 0x100, nc, h, w, bf16=True)
    assert rc32 == 0 and rc16 == 0, lib.ap_last_error()
    for win in (dy32, dy16, ws32, ws16):
        assert win.guards_intact()
    assert dy32.finite() and dy16.finite() and ws32.untouched() and ws16.untouched()
    for e, s in per_plane_errors(dy32.data.view(1, nc, h, w), p['ref']):
        assert e < 2e-5 * s, (e, s)
    assert torch.equal(dy16.data, dy32.data.bfloat16())


# ---------------------------------------------------------------- ap_act_bwd, ap_act_bwd_bias

def act_id(case):
    return '%s %dx%d p%d act%d%s%s' % (case[0], case[1], case[2], case[3], case[4], ' g2' if case[5] else '', '' if case[7] else ' no out')


@pytest.mark.parametrize('case', ACT_CASES, ids=act_id)
def test_act_bwd_on_its_route(dev, case):
    route, h, w, pad, act, two, nc, with_out = case
    lib = _lib()
    assert _route(lib.ap_act_bwd_route, pad, h, w) == (0, route)
    p = act_problem(1, nc, h, w, pad, act, two, with_out)
    rc, dy = call_act_bwd(dev, p, pad, act, nc, h, w)
    assert rc == 0, lib.ap_last_error()
    assert dy.guards_intact() and dy.finite()
    errs = per_plane_errors(dy.data.view(1, nc, h, w), p['ref'])
    print('act_bwd', act_id(case), 'worst plane error / max|dy| = %.3g' % max(e / s for e, s in errs))
    for e, s in errs:
        assert e < 1e-5 * s, (e, s)


@pytest.mark.parametrize('case', ACT_BIAS_CASES, ids=lambda c: 'N%d C%d %dx%d p%d act%d%s' % (c[:6] + (' g2' if c[6] else '',)))
def test_act_bwd_bias_one_pass(dev, case):
    """dy bit-equal to ap_act_bwd's, db[c] against the fp64 sum of the reference dy, the block sums laid out [c][n][block] in a
    workspace of exactly ap_act_bwd_bias_workspace_floats floats, the same bits on a second call."""
    n, c, h, w, pad, act, two = case
    lib = _lib()
    assert _route(lib.ap_act_bwd_route, pad, h, w) == (0, 'act_generic')
    p = act_problem(n, c, h, w, pad, act, two)
    g1, g2, out = _to(dev, p['g1'], p['g2'], p['out'])
    nws = lib.ap_act_bwd_bias_workspace_floats(n, c, h, w)
    assert nws == n * c * min(32, (h * w + 1023) // 1024)
    ref_db, ref_abs = p['ref'].sum((0, 2, 3)), p['ref'].abs().sum((0, 2, 3))
    dbs = []
    for _ in range(2):
        dy, ws, db = Window(dev, n * c * h * w), Window(dev, nws), Window(dev, c)
        rc = lib.ap_act_bwd_bias(_p(g1), pad, _p(g2), _p(out), act, n, c, h, w, dy.ptr, ws.ptr, db.ptr, _stream(dev))
        torch.cuda.synchronize(dev)
        assert rc == 0, lib.ap_last_error()
        for win in (dy, ws, db):
            assert win.guards_intact() and win.finite()
        dbs.append(db.data.clone())
    rc, plain = call_act_bwd(dev, p, pad, act, n * c, h, w)
    assert rc == 0 and torch.equal(dy.data, plain.data)
    for e, s in per_plane_errors(dy.data.view(n, c, h, w), p['ref']):
        assert e < 1e-5 * s, (e, s)
    err = (dbs[0].double().cpu() - ref_db).abs()
    print('act_bwd_bias db error / sum|dy_c| =', (err / ref_abs).tolist())
    assert bool((err <= 2e-6 * ref_abs).all()), (err, ref_abs)
    assert torch.equal(dbs[0], dbs[1])


# ---------------------------------------------------------------- ap_bias_grad, ap_bias_grad_ws

def _check_db(tag, db, ref, e_ref, ref_abs):
    err = (db.double().cpu() - ref).abs()
    print(tag, 'e_ref / sum|dy_c| = %.3g, kernel error / sum|dy_c| = %.3g' % (float((e_ref / ref_abs).max()), float((err / ref_abs).max())))
    assert bool((err <= 4 * e_ref + 1e-6 * ref_abs).all()), (err, e_ref, ref_abs)


@pytest.mark.parametrize('case', BIAS_DIRECT_CASES, ids=lambda c: 'N%d C%d HW%d' % c)
def test_bias_grad_one_stage(dev, case):
    n, c, hw = case
    dy, ref, e_ref, ref_abs = bias_problem(n, c, hw)
    dyd = dy.to(dev)
    dbs = []
    for _ in range(2):
        db = Window(dev, c)
        rc = _lib().ap_bias_grad(_p(dyd), n, c, hw, db.ptr, _stream(dev))
        torch.cuda.synchronize(dev)
        assert rc == 0 and db.guards_intact() and db.finite()
        dbs.append(db.data.clone())
    _check_db('bias_grad N%d C%d HW%d' % case, dbs[0], ref, e_ref, ref_abs)
    assert torch.equal(dbs[0], dbs[1])


def test_bias_grad_many_channels_through_ops(dev):
    """ops.bias_grad takes the one-workgroup-per-channel kernel from 1024 channels on"""
    from animateportrait_amd import ops
    n, c, hw = 2, 1024, 4
    dy, ref, e_ref, ref_abs = bias_problem(n, c, hw)
    dyd = dy.view(n, c, 2, 2).to(dev)
    db = ops.bias_grad(dyd)
    _check_db('ops.bias_grad C1024 2x2', db, ref, e_ref, ref_abs)
    assert torch.equal(db, ops.bias_grad(dyd))


@pytest.mark.parametrize('case', BIAS_WS_CASES, ids=lambda c: 'N%d C%d HW%d split%d' % c)
def test_bias_grad_two_stages(dev, case):
    """The sliced stage: per = ceil(HW / split) elements per slice with a ragged last one, partials at ws[(c N + n) split + slice]."""
    n, c, hw, split = case
    lib = _lib()
    nws = lib.ap_bias_grad_workspace_floats(n, c, hw)
    assert nws == n * c * split
    dy, ref, e_ref, ref_abs = bias_problem(n, c, hw)
    dyd = dy.to(dev)
    dbs = []
    for _ in range(2):
        ws, db = Window(dev, nws), Window(dev, c)
        rc = lib.ap_bias_grad_ws(_p(dyd), n, c, hw, ws.ptr, db.ptr, _stream(dev))
        torch.cuda.synchronize(dev)
        assert rc == 0, lib.ap_last_error()
        for win in (ws, db):
            assert win.guards_intact() and win.finite()
        dbs.append(db.data.clone())
    _check_db('bias_grad_ws N%d C%d HW%d split%d' % case, dbs[0], ref, e_ref, ref_abs)
    assert torch.equal(dbs[0], dbs[1])
    # the partials themselves: slice sp of plane (n, c) sums elements [sp per, min((sp + 1) per, HW))
    per = (hw + split - 1) // split
    parts = torch.stack([dy.double()[:, :, sp * per:min((sp + 1) * per, hw)].sum(2) for sp in range(split)], 2)      # [n][c][sp]
    want = parts.permute(1, 0, 2).reshape(-1)
    tol = 1e-6 * dy.double().abs().sum(2).permute(1, 0).reshape(-1, 1).expand(-1, split).reshape(-1) + 1e-30
    assert bool(((ws.data.double().cpu() - want).abs() <= tol).all())


# ---------------------------------------------------------------- refusals

def _refused(rc, *windows):
    assert rc < 0
    for win in windows:
        assert win.guards_intact() and win.untouched()


def test_refused_calls_write_nothing(dev):
    lib = _lib()
    small = inbwd_problem(4, 8, 0, 1, False, 3)
    # fold pad >= H
    pad4 = dict(small, g1=torch.zeros(1, 3, 12, 16))
    rc, dy, ws = call_instnorm_bwd(dev, pad4, 4, 1, 3, 4, 8)
    assert rc == AP_ERR_INVALID
    _refused(rc, dy, ws)
    # tanh is no activation of a normalised layer
    rc, dy, ws = call_instnorm_bwd(dev, small, 0, 3, 3, 4, 8)
    assert rc == AP_ERR_INVALID
    _refused(rc, dy, ws)
    # null y
    keep = _to(dev, small['g1'], small['mean'], small['rstd'])
    dy, ws = Window(dev, 3 * 32), Window(dev, 6)
    rc = lib.ap_instnorm_bwd(_p(keep[0]), 0, None, None, _p(keep[1]), _p(keep[2]), 1, 3, 4, 8, ws.ptr, dy.ptr, _stream(dev))
    torch.cuda.synchronize(dev)
    assert rc == AP_ERR_INVALID
    _refused(rc, dy, ws)
    # the bf16 bit with a fold, and outside the big-plane band
    folded = inbwd_problem(132, 128, 1, 1, True, 3)
    rc, dy, ws = call_instnorm_bwd(dev, folded, 1, 1 | 0x100, 3, 132, 128)
    assert rc == AP_ERR_UNSUPPORTED
    _refused(rc, dy, ws)
    plain = inbwd_problem(64, 64, 0, 0, False, 3)
    rc, dy, ws = call_instnorm_bwd(dev, plain, 0, 0 | 0x100, 3, 64, 64)
    assert rc == AP_ERR_UNSUPPORTED
    _refused(rc, dy, ws)
    # N * C = 65536 planes (of 2 x 2)
    nc = 65536
    many = {'g1': torch.zeros(1, nc, 2, 2), 'g2': None, 'y': torch.zeros(1, nc, 2, 2), 'mean': torch.zeros(nc), 'rstd': torch.ones(nc),
            'out': torch.zeros(1, nc, 2, 2)}
    rc, dy, ws = call_instnorm_bwd(dev, many, 0, 1, nc, 2, 2)
    assert rc == AP_ERR_UNSUPPORTED
    _refused(rc, dy, ws)
    rc, dy = call_act_bwd(dev, many, 0, 1, nc, 2, 2)
    assert rc == AP_ERR_UNSUPPORTED
    _refused(rc, dy)
    # ap_act_bwd: act 4, fold pad >= H
    ap = act_problem(1, 3, 4, 8, 0, 1, False)
    rc, dy = call_act_bwd(dev, ap, 0, 4, 3, 4, 8)
    assert rc == AP_ERR_INVALID
    _refused(rc, dy)
    rc, dy = call_act_bwd(dev, dict(ap, g1=torch.zeros(1, 3, 12, 16)), 4, 1, 3, 4, 8)
    assert rc == AP_ERR_INVALID
    _refused(rc, dy)
    # ... and its activated output missing where the activation needs it
    rc, dy = call_act_bwd(dev, dict(ap, out=None), 0, 1, 3, 4, 8)
    assert rc == AP_ERR_INVALID
    _refused(rc, dy)
