"""Reference of the feature-warp kernels (csrc/warp_fwd.hip, csrc/warp_bwd.hip) for ANY N, C, H, W, S -- a plain helper module of the tests, CPU only.

``warp_concat_ref`` restates double_feature_warping (oracle/warp.py, which is tied to 256 / 128 / 64) with the same torch calls on
independent H, W and S; its backward is torch autograd through it.  Evaluated in float64 it is what the kernels are compared with,
evaluated in float32 it measures how far honest fp32 arithmetic on the same inputs strays from that (the ``e_ref`` of the bars).

The only discontinuity of the operator is the threshold ``mask > 0.5`` on the RESIZED mask: ``ambiguous`` names the pixels where an
fp32 evaluation may legitimately fall on the other side.  ``make_maps`` is the seeded factory of sampling maps, by kind; ``tile_boxes``
is a model of the backward kernel's per-tile bounding box, used by the CPU test that keeps every named case on the branch it is
named for."""
import math

import torch
import torch.nn.functional as F

MAX_EXCLUDED = 0.005          # a case may exclude at most this share of its pixels as ambiguous (asserted, not measured)

# geometry of warp_concat_bwd_tiled_kernel (csrc/warp_bwd.hip: kBwdTileW, kBwdTileH, kBwdWin, kBwdWinW)
TILE_W, TILE_H, WIN, WIN_W = 32, 16, 1344, 48


# ------------------------------------------------------------------------------------------------------------ the operator

def resized_maps(motion, flow, ifmask, H, W, flow_scale, dtype):
    """(motion_L [N,H,W,2], flow_L [N,2,H,W], mask_L [N,1,H,W]) in ``dtype``: the three maps at the feature resolution."""
    mo, fl, mk = motion.to(dtype), flow.to(dtype) * flow_scale, ifmask.to(dtype)
    S = mo.shape[1]
    if (H, W) != (S, S):
        def rs(t):
            return F.interpolate(t, size=(H, W), mode='bilinear', align_corners=True)
        mo, fl, mk = rs(mo.permute(0, 3, 1, 2)).permute(0, 2, 3, 1), rs(fl), rs(mk)
    return mo, fl, mk


def flow_grid(fl):
    """warp_acc_flow: 2 * (pixel + flow) / max(size - 1, 1) - 1 as a grid_sample grid [N,H,W,2]."""
    n, _, h, w = fl.shape
    xx = torch.arange(w, dtype=fl.dtype).view(1, 1, w)
    yy = torch.arange(h, dtype=fl.dtype).view(1, h, 1)
    gx = 2.0 * (xx + fl[:, 0]) / max(w - 1, 1) - 1.0
    gy = 2.0 * (yy + fl[:, 1]) / max(h - 1, 1) - 1.0
    return torch.stack([gx, gy], dim=-1)


def _gs(x, grid):
    return F.grid_sample(x, grid, mode='bilinear', padding_mode='zeros', align_corners=False)


def warp_concat_ref(x, motion, flow, ifmask, H, W, flow_scale, dtype):
    """(out [N,2C,H,W], resized mask [N,1,H,W]) in ``dtype`` for x [N,C,H,W], motion [N,S,S,2], flow [N,2,S,S], ifmask [N,1,S,S]."""
    assert tuple(x.shape[2:]) == (H, W)
    mo, fl, mk = resized_maps(motion, flow, ifmask, H, W, flow_scale, dtype)
    xd = x.to(dtype)
    x1 = _gs(xd, mo)
    x2 = torch.where(mk > 0.5, _gs(xd, flow_grid(fl)), torch.full((), -1.0, dtype=dtype))
    return torch.cat([x1, x2], 1), mk


def warp_concat_bwd_ref(gout, motion, flow, ifmask, flow_scale, dtype):
    """dx [N,C,H,W] in ``dtype``: autograd of warp_concat_ref w.r.t. x for the output gradient gout [N,2C,H,W]."""
    n, c2, H, W = gout.shape
    x = torch.zeros(n, c2 // 2, H, W, dtype=dtype, requires_grad=True)          # (the operator is linear in x)
    out, _ = warp_concat_ref(x, motion, flow, ifmask, H, W, flow_scale, dtype)
    out.backward(gout.to(dtype))
    return x.grad.detach()


def abs_mass(gout, motion, flow, ifmask, flow_scale):
    """A [N,C,H,W], float64: per element of dx the sum of the ABSOLUTE contributions |gout * weight| it receives.  The bilinear
    weights are non-negative, so this is the same backward applied to |gout|."""
    return warp_concat_bwd_ref(gout.abs(), motion, flow, ifmask, flow_scale, torch.float64)


def ambiguous(resized_mask64, band=1e-4):
    """Pixels [N,1,H,W] whose float64 resized mask lies within ``band`` of the 0.5 threshold."""
    return (resized_mask64 - 0.5).abs() <= band


def instance_norm_act(x, mean, rstd, act, dtype):
    """act((x - mean) * rstd) in ``dtype`` with per-(n, c) statistics [N*C]; act 0 none, 1 ReLU, 2 LeakyReLU(0.2)."""
    n, c = x.shape[:2]
    v = (x.to(dtype) - mean.to(dtype).view(n, c, 1, 1)) * rstd.to(dtype).view(n, c, 1, 1)
    if act == 1:
        v = F.relu(v)
    elif act == 2:
        v = F.leaky_relu(v, 0.2)
    return v


# ------------------------------------------------------------------------------------------------------------ the maps

KINDS = ('smooth', 'noise', 'out', 'fits', 'clip2d', 'whitenoise', 'far', 'nothing', 'halfout', 'rowcollapse', 'colcollapse',
         'border', 'maskoff')


def _identity(N, S):
    """The grid that samples every pixel of an S x S map at its own centre (align_corners=False): (2 i + 1) / S - 1."""
    c = (2.0 * torch.arange(S, dtype=torch.float32) + 1.0) / S - 1.0
    yy, xx = torch.meshgrid(c, c, indexing='ij')
    return torch.stack([xx, yy], -1).unsqueeze(0).repeat(N, 1, 1, 1)


def _pixels(N, S):
    """(x, y) pixel indices of an S x S map as [N,S,S] float tensors."""
    i = torch.arange(S, dtype=torch.float32)
    yy, xx = torch.meshgrid(i, i, indexing='ij')
    return xx.unsqueeze(0).repeat(N, 1, 1), yy.unsqueeze(0).repeat(N, 1, 1)


def make_maps(kind, N, H, W, S, flow_scale, seed):
    """(motion [N,S,S,2], flow [N,2,S,S], ifmask [N,1,S,S]) float32, a pure function of its arguments.

    The maps live at S x S and are resized to H x W by the operator; ``flow`` is in pixels of the S-resolution pyramid base, i.e.
    ``flow * flow_scale`` is in pixels of the feature map.  Amplitudes given in px below are feature-map pixels.

    smooth       0.9 * identity + 0.1 * sin, sinusoidal flow of 4 px, rand mask
    noise        identity + 5 / S of white noise, white-noise flow of 2.5 px, rand mask
    out          1.6 * identity, flow of + S px: most taps out of frame, rand mask
    fits         smooth with a 2 px flow: every tile's box fits the backward window
    clip2d       0.3 * identity motion (a 10 x 5 patch per tile) and a flow branch that samples 1.9 * pixel (61 x 31 per tile): the
                 union box of a tile is wider than the window's 48 columns AND taller than its 28 rows; mask of ones
    whitenoise   motion uniform in [-1.2, 1.2] per pixel, white-noise flow of 20 px, rand mask: the box is the whole map
    far          motion samples the top-left 4 x 4 pixels, the flow branch (mask of ones) the bottom-right 4 x 4
    nothing      every tap of both branches out of frame
    halfout      smooth, but the left half of the map samples out of frame in both branches
    rowcollapse  motion a function of x only and pixel + flow_y constant: all rows of a column hit one source row
    colcollapse  motion a function of y only and pixel + flow_x constant: all pixels of a row hit one source column
    border       motion samples exactly ix in {-1, -0.5, 0, integers, W - 1, W - 0.5, W} (H = W = S, a power of two), integer flow
    maskoff      smooth with an all-zero mask: the flow branch is dead
    """
    assert kind in KINDS, kind
    g = torch.Generator().manual_seed(seed)
    ident = _identity(N, S)
    px, py = _pixels(N, S)
    u = 1.0 / flow_scale                     # one feature-map pixel of flow, in the units of ``flow``
    tx, ty = (px + 0.5) / S, (py + 0.5) / S      # position in [0, 1]
    mask = torch.rand(N, 1, S, S, generator=g)
    ones = torch.ones(N, 1, S, S)

    def smooth(amp_px):
        ph = torch.rand(4, generator=g) * 2 * math.pi
        wob = torch.stack([torch.sin(2 * math.pi * ty + ph[0]), torch.sin(2 * math.pi * tx + ph[1])], -1)
        mo = 0.9 * ident + 0.1 * wob
        fl = amp_px * u * torch.stack([torch.sin(2 * math.pi * (tx + ty) + ph[2]), torch.cos(2 * math.pi * (tx - ty) + ph[3])], 1)
        return mo, fl

    if S == 1 and kind in ('smooth', 'noise', 'out'):
        # a one-pixel map has no extent to scale or shake: motion 0 is the centre of the frame, so the samples land in it
        mo = torch.zeros(N, 1, 1, 2)
        fl = {'smooth': 0.25, 'noise': -0.4, 'out': 1000.0}[kind] * u * torch.ones(N, 2, 1, 1)
        return mo, fl, mask
    if kind == 'smooth':
        mo, fl = smooth(4.0)
    elif kind == 'noise':
        mo = ident + (5.0 / S) * torch.randn(N, S, S, 2, generator=g)
        fl = 2.5 * u * torch.randn(N, 2, S, S, generator=g)
    elif kind == 'out':
        mo = 1.6 * ident
        fl = float(S) * torch.ones(N, 2, S, S)
    elif kind == 'fits':
        mo, fl = smooth(2.0)
    elif kind == 'clip2d':
        mo = 0.3 * ident
        # pixel + flow = 1.9 * pixel at the feature resolution; linear in the position, so the align_corners resize keeps it exact
        fl = 0.9 * u * torch.stack([px * (W - 1) / max(S - 1, 1), py * (H - 1) / max(S - 1, 1)], 1)
        mask = ones
    elif kind == 'whitenoise':
        mo = torch.rand(N, S, S, 2, generator=g) * 2.4 - 1.2
        fl = 20.0 * u * torch.randn(N, 2, S, S, generator=g)
    elif kind == 'far':
        mo = -1.0 + (0.25 + 3.5 * torch.rand(N, S, S, 2, generator=g)) * 2.0 / torch.tensor([W, H], dtype=torch.float32)
        # flow branch: pixel + flow uniform in [size - 4.5, size - 1.25]
        tgt = torch.stack([W - 4.5 + 3.25 * torch.rand(N, S, S, generator=g), H - 4.5 + 3.25 * torch.rand(N, S, S, generator=g)], 1)
        pos = torch.stack([px * (W - 1) / max(S - 1, 1), py * (H - 1) / max(S - 1, 1)], 1)
        fl = (tgt - pos) * u
        mask = ones
    elif kind == 'nothing':
        mo = 3.0 + torch.rand(N, S, S, 2, generator=g)
        fl = -(4.0 * max(H, W)) * u * torch.ones(N, 2, S, S)
    elif kind == 'halfout':
        mo, fl = smooth(4.0)
        left = (px < S // 2)
        mo = torch.where(left.unsqueeze(-1), torch.full_like(mo, -3.0), mo)
        fl = torch.where(left.unsqueeze(1), torch.full_like(fl, -(4.0 * max(H, W)) * u), fl)
    elif kind == 'rowcollapse':
        row = torch.rand(N, 1, 1, generator=g) * 1.6 - 0.8
        mo = torch.stack([0.9 * ident[..., 0] + 0.05 * torch.sin(2 * math.pi * tx), row.expand(N, S, S)], -1)
        ytgt = (H - 1) * (0.2 + 0.6 * torch.rand(N, 1, 1, generator=g))
        fl = u * torch.stack([1.5 * torch.sin(2 * math.pi * tx), ytgt - py * (H - 1) / max(S - 1, 1)], 1)
    elif kind == 'colcollapse':
        col = torch.rand(N, 1, 1, generator=g) * 1.6 - 0.8
        mo = torch.stack([col.expand(N, S, S), 0.9 * ident[..., 1] + 0.05 * torch.sin(2 * math.pi * ty)], -1)
        xtgt = (W - 1) * (0.2 + 0.6 * torch.rand(N, 1, 1, generator=g))
        fl = u * torch.stack([xtgt - px * (W - 1) / max(S - 1, 1), 1.5 * torch.sin(2 * math.pi * ty)], 1)
    elif kind == 'border':
        assert H == S and W == S and S & (S - 1) == 0, 'border: exact coordinates need H = W = S = 2^k'
        # ix = ((g + 1) * S - 1) / 2  <=>  g = (2 ix + 1) / S - 1, exact in fp32 for half-integer ix and S a power of two
        special = torch.tensor([-1.0, -0.5, 0.0, 0.5, 1.0, S / 2.0, S - 2.0, S - 1.5, S - 1.0, S - 0.5, float(S), 3.0, 7.0, 2.5])
        ix = special[torch.randint(0, len(special), (N, S, S), generator=g)]
        iy = special[torch.randint(0, len(special), (N, S, S), generator=g)]
        mo = torch.stack([(2 * ix + 1) / S - 1, (2 * iy + 1) / S - 1], -1)
        fl = u * torch.randint(-3, 4, (N, 2, S, S), generator=g).float()
    elif kind == 'maskoff':
        mo, fl = smooth(4.0)
        mask = torch.zeros(N, 1, S, S)
    return mo.contiguous().float(), fl.contiguous().float(), mask.contiguous().float()


# ------------------------------------------------------------------------------------------------------------ tile-box model

def taps64(motion, flow, ifmask, H, W, flow_scale):
    """Float64 north-west taps of both branches: dict with x0, y0 [2,N,H,W] (long; the kernel's clamp to [-2, size + 1] applied),
    inr [2,4,N,H,W] (tap k = nw, ne, sw, se in range) and live [2,N,H,W] (branch carries gradient: always / mask > 0.5)."""
    mo, fl, mk = resized_maps(motion, flow, ifmask, H, W, flow_scale, torch.float64)
    grids = (mo, flow_grid(fl))
    x0s, y0s, inrs = [], [], []
    for gr in grids:
        ix = (((gr[..., 0] + 1) * W - 1) / 2).clamp(-2.0, W + 1.0)
        iy = (((gr[..., 1] + 1) * H - 1) / 2).clamp(-2.0, H + 1.0)
        x0, y0 = ix.floor().long(), iy.floor().long()
        x0s.append(x0)
        y0s.append(y0)
        inr = []
        for k in range(4):
            xx, yy = x0 + (k & 1), y0 + (k >> 1)
            w = ((ix - x0) if (k & 1) else (x0 + 1 - ix)) * ((iy - y0) if (k >> 1) else (y0 + 1 - iy))
            inr.append((xx >= 0) & (xx < W) & (yy >= 0) & (yy < H) & (w != 0))
        inrs.append(torch.stack(inr))
    live = torch.stack([torch.ones_like(mk[:, 0], dtype=torch.bool), mk[:, 0] > 0.5])
    return dict(x0=torch.stack(x0s), y0=torch.stack(y0s), inr=torch.stack(inrs), live=live)


def tile_boxes(motion, flow, ifmask, H, W, flow_scale):
    """What warp_concat_bwd_tiled_kernel derives per 32 x 16 tile, from the float64 taps.  A list of dicts, one per (n, tile):
    empty (no branch with an in-range tap: the tile returns early), bw, bh (the box around the corners, clamped to the frame, of the
    branches that have one), clipped (bw * bh > WIN), win = (x, y, w, h) of the window the kernel keeps, inside / outside (number of
    in-range taps of live branches in / beyond that window)."""
    t = taps64(motion, flow, ifmask, H, W, flow_scale)
    N = t['x0'].shape[1]
    out = []
    for n in range(N):
        for ty in range(0, H, TILE_H):
            for tx in range(0, W, TILE_W):
                sl = (slice(None), n, slice(ty, min(ty + TILE_H, H)), slice(tx, min(tx + TILE_W, W)))
                x0, y0, live = t['x0'][sl], t['y0'][sl], t['live'][sl]
                inr = t['inr'][:, :, n, ty:ty + TILE_H, tx:tx + TILE_W] & live.unsqueeze(1)
                on = inr.any(1)
                d = dict(n=n, ty=ty, tx=tx, empty=not bool(on.any()))
                if not d['empty']:
                    xa, xb = x0[on].clamp(min=0), (x0[on] + 1).clamp(max=W - 1)
                    ya, yb = y0[on].clamp(min=0), (y0[on] + 1).clamp(max=H - 1)
                    bx0, by0 = int(xa.min()), int(ya.min())
                    bw, bh = int(xb.max()) - bx0 + 1, int(yb.max()) - by0 + 1
                    d.update(bw=bw, bh=bh, clipped=bw * bh > WIN)
                    if d['clipped']:
                        nw = min(bw, WIN_W)
                        nh = min(bh, WIN // nw)
                        bx0, by0, bw, bh = bx0 + (bw - nw) // 2, by0 + (bh - nh) // 2, nw, nh
                    xs = torch.cat([(x0 + (k & 1))[inr[:, k]] for k in range(4)])
                    ys = torch.cat([(y0 + (k >> 1))[inr[:, k]] for k in range(4)])
                    ins = (xs >= bx0) & (xs < bx0 + bw) & (ys >= by0) & (ys < by0 + bh)
                    d.update(win=(bx0, by0, bw, bh), inside=int(ins.sum()), outside=int((~ins).sum()))
                out.append(d)
    return out


def lane_pixels(lane):
    """(row, column) inside a tile of the 8 pixels lane ``lane`` of a wave walks: p = i * 64 + lane, row p >> 5, column p & 31."""
    return [((i * 64 + lane) >> 5, (i * 64 + lane) & 31) for i in range(TILE_W * TILE_H // 64)]


# ------------------------------------------------------------------------------------------------------------ the cases
# (N, C, H, W, S, flow_scale).  Shared by tests/test_warp_contract_gpu.py (which launches them) and tests/test_warp_reference_cpu.py
# (which checks, without a GPU, that each excludes at most MAX_EXCLUDED of its pixels and reaches the branch it is named for).

SHAPES = {
    'direct40':  (2, 9, 40, 40, 40, 1.0),      # H == S direct; forward untiled, ragged last block (1600 = 6 * 256 + 64); 7 * 2 * 2 = 28 blocks
                                               # (not a multiple of 8); backward 2 x 3 partial tiles; tail group of 1 channel
    'level1':    (2, 9, 20, 20, 40, 0.5),      # level 1 of an S = 40 model (through ops)
    'level2':    (2, 3, 10, 10, 40, 0.25),     # level 2 of an S = 40 model (through ops)
    'wide':      (2, 8, 24, 64, 48, 0.5),      # non-square; forward tiled mapping with the lerp path
    'overhang':  (3, 5, 17, 33, 40, 0.5),      # one pixel of overhang in both tile directions; C < 8
    'halflerp':  (2, 8, 32, 64, 32, 1.0),      # H == S, W != S: the lerp path
    'h1':        (1, 4, 1, 37, 16, 1.0),
    'w1':        (1, 4, 5, 1, 16, 1.0),
    's1':        (1, 8, 8, 8, 1, 1.0),
    'upsample':  (1, 7, 48, 48, 16, 1.0),      # S < H; odd nc
}
LEVEL_OF = {'level1': 1, 'level2': 2}          # the shapes that go through ops.warp_concat / ops.warp_concat_bwd
FWD_KINDS = ('smooth', 'noise', 'out')
VARIANT_SHAPES = ('direct40', 'wide', 'overhang', 'upsample')     # the forward variants run on these at least

SPLIT_SHAPES = {'c16': (2, 16, 40, 40, 40, 1.0), 'wide': (2, 8, 24, 64, 48, 0.5)}
S2D_SHAPES = {'small': (2, 8, 6, 10, 16, 1.0), 'wide': (2, 8, 24, 64, 48, 0.5)}
OCTET_SHAPES = {'c16': (2, 16, 40, 40, 40, 1.0), 'wide': (1, 8, 24, 64, 48, 0.5)}
QUAD_SHAPES = {'w4': (1, 8, 64, 4, 64, 1.0 / 16), 'tiled': (1, 8, 8, 32, 32, 0.25)}

# the named backward cases: kind of map and shape; C in {10, 7, 1} so that the last wave of a block has two channels or one
BWD_CASES = {
    'fits':        ('fits', (2, 10, 64, 64, 64, 1.0)),
    'clip2d':      ('clip2d', (1, 7, 64, 64, 16, 1.0)),
    'whitenoise':  ('whitenoise', (2, 10, 64, 64, 64, 1.0)),
    'whitenoise_ragged': ('whitenoise', (1, 7, 40, 40, 40, 1.0)),
    'far':         ('far', (1, 1, 64, 64, 64, 1.0)),
    'nothing':     ('nothing', (1, 7, 40, 40, 40, 1.0)),
    'halfout':     ('halfout', (2, 7, 48, 64, 64, 1.0)),
    'rowcollapse': ('rowcollapse', (1, 10, 64, 64, 64, 1.0)),
    'colcollapse': ('colcollapse', (1, 7, 64, 64, 64, 1.0)),
    'border':      ('border', (2, 1, 32, 32, 32, 1.0)),
    'maskoff':     ('maskoff', (1, 10, 40, 40, 40, 1.0)),
}


def case_seed(name, kind):
    """A fixed seed per (shape or case name, kind)."""
    return 1000 + 17 * sum(ord(ch) for ch in name) + 3 * KINDS.index(kind)


def all_cases():
    """Every (label, kind, shape) the GPU file launches maps for."""
    out = [('%s-%s' % (name, kind), kind, shp, case_seed(name, kind)) for name, shp in SHAPES.items() for kind in FWD_KINDS]
    for group, table in (('split', SPLIT_SHAPES), ('s2d', S2D_SHAPES), ('octet', OCTET_SHAPES), ('quad', QUAD_SHAPES)):
        for name, shp in table.items():
            kinds = ('noise', 'out') if group == 'quad' else ('noise',)
            out += [('%s-%s-%s' % (group, name, kind), kind, shp, case_seed(group + name, kind)) for kind in kinds]
    out += [('bwd-' + name, kind, shp, case_seed(name, kind)) for name, (kind, shp) in BWD_CASES.items()]
    return out


def case_maps(kind, shape, seed):
    N, C, H, W, S, fs = shape
    return make_maps(kind, N, H, W, S, fs, seed)


def excluded_share(kind, shape, seed):
    """Share of the case's pixels that ``ambiguous`` excludes."""
    N, C, H, W, S, fs = shape
    mo, fl, mk = case_maps(kind, shape, seed)
    _, _, m64 = resized_maps(mo, fl, mk, H, W, fs, torch.float64)
    return float(ambiguous(m64).double().mean())
