"""CPU: the float64 reference of the warp kernels (tests/warp_reference.py) and the cases of tests/test_warp_contract_gpu.py.

(a) the reference equals the oracle where the oracle is defined (S = 256, levels 0 / 1 / 2), which the goldens pin;
(b) no case excludes more than 0.5 % of its pixels as ambiguous (a condition on the inputs, fixed before any kernel runs);
(c) every named backward case reaches the branch of warp_concat_bwd_tiled_kernel it is named for, by a model of the kernel's
    per-tile box evaluated on the float64 taps -- so that a retuned tile or window constant cannot quietly turn a hard case into an
    easy one (update warp_reference.TILE_W / TILE_H / WIN / WIN_W with the kernel and see which cases need new maps)."""
import re
import os

import pytest
import torch

import warp_reference as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_equals_the_oracle_at_256():
    from animateportrait_amd.synthetic import make_generator_inputs
    from oracle import warp as ow
    d = make_generator_inputs(1, seed=3)
    for level in (0, 1, 2):
        h = 256 >> level
        x = torch.randn(1, 3, h, h, generator=torch.Generator().manual_seed(40 + level)) * 3 + 1
        want = ow.double_feature_warping(x, d['motion'], d['flow'], d['ifmask'], level)
        got, _ = wr.warp_concat_ref(x, d['motion'], d['flow'], d['ifmask'], h, h, 1.0 / (1 << level), torch.float32)
        # one unit in the last place of the larger operand
        ulp = torch.maximum(got.abs(), want.abs()).clamp(min=2.0 ** -126) * 2.0 ** -23
        assert bool(((got - want).abs() <= ulp).all()), (level, float((got - want).abs().max()))


def test_reference_handles_degenerate_sizes():
    """H = 1, W = 1, S = 1 and S < H: finite, the right shapes, and a backward that is the transpose of the forward."""
    for name in ('h1', 'w1', 's1', 'upsample'):
        N, C, H, W, S, fs = wr.SHAPES[name]
        mo, fl, mk = wr.make_maps('smooth', N, H, W, S, fs, 5)
        g = torch.Generator().manual_seed(1)
        x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
        gout = torch.randn(N, 2 * C, H, W, generator=g, dtype=torch.float64)
        out, m = wr.warp_concat_ref(x, mo, fl, mk, H, W, fs, torch.float64)
        assert out.shape == (N, 2 * C, H, W) and m.shape == (N, 1, H, W) and bool(torch.isfinite(out).all())
        gout[:, C:] *= (m > 0.5)                        # the masked-out half is the constant -1: not linear in x
        dx = wr.warp_concat_bwd_ref(gout, mo, fl, mk, fs, torch.float64)
        lhs, rhs = float((out * gout).sum()), float((x * dx).sum())
        assert abs(lhs - rhs) <= 1e-12 * float((x.abs() * wr.abs_mass(gout, mo, fl, mk, fs)).sum()) + 1e-300, (name, lhs, rhs)


@pytest.mark.parametrize('label,kind,shape,seed', wr.all_cases(), ids=[c[0] for c in wr.all_cases()])
def test_excluded_share_stays_under_the_cap(label, kind, shape, seed):
    share = wr.excluded_share(kind, shape, seed)
    print('%s: excluded share %.3e' % (label, share))
    assert share <= wr.MAX_EXCLUDED, (label, share)


def test_box_model_has_the_kernels_constants():
    src = open(os.path.join(ROOT, 'animateportrait_amd', 'csrc', 'warp_bwd.hip')).read()

    def const(name):
        return int(re.search(r'\b%s = (\d+)' % name, src).group(1))
    assert (const('kBwdTileW'), const('kBwdTileH'), const('kBwdWin'), const('kBwdWinW')) == (wr.TILE_W, wr.TILE_H, wr.WIN, wr.WIN_W)


def _boxes(name):
    kind, shape = wr.BWD_CASES[name]
    N, C, H, W, S, fs = shape
    mo, fl, mk = wr.case_maps(kind, shape, wr.case_seed(name, kind))
    return wr.tile_boxes(mo, fl, mk, H, W, fs), (mo, fl, mk), shape


def test_backward_cases_reach_their_branches():
    b, _, _ = _boxes('fits')
    assert all(not t['empty'] and not t['clipped'] for t in b), 'fits: a box exceeds the window'

    b, _, shape = _boxes('clip2d')
    assert any(t['bw'] > wr.WIN_W and t['bh'] > wr.WIN // wr.WIN_W and t['inside'] > 0 and t['outside'] > 0 for t in b)
    assert shape[1] % 8 % 2 == 1, 'clip2d: the last wave must own ONE channel (nc odd)'

    for name in ('whitenoise', 'whitenoise_ragged'):
        b, _, (N, C, H, W, S, fs) = _boxes(name)
        assert all(t['clipped'] and t['bw'] >= W - 2 and t['bh'] >= H - 2 and t['outside'] > 0 and t['inside'] > 0 for t in b), name

    b, _, _ = _boxes('far')
    assert all(t['clipped'] and t['inside'] == 0 and t['outside'] > 0 for t in b), 'far: the centre window catches a tap'

    b, _, _ = _boxes('nothing')
    assert all(t['empty'] for t in b)

    b, _, _ = _boxes('halfout')
    assert any(t['empty'] for t in b) and any(not t['empty'] for t in b)
    assert all(t['empty'] == (t['tx'] == 0) for t in b), 'halfout: exactly the left tiles return early'

    b, _, _ = _boxes('maskoff')
    assert all(not t['empty'] for t in b)

    # partial tiles: the ragged shapes have overhang in both directions
    for name in ('whitenoise_ragged', 'nothing', 'maskoff'):
        _, shape = wr.BWD_CASES[name]
        assert shape[2] % wr.TILE_H != 0 and shape[3] % wr.TILE_W != 0


def _lane_addresses(name):
    """[2 branches, N, tiles, 64 lanes, 8 pixels] linear address of the north-west tap, from the float64 taps."""
    kind, shape = wr.BWD_CASES[name]
    N, C, H, W, S, fs = shape
    assert H % wr.TILE_H == 0 and W % wr.TILE_W == 0
    mo, fl, mk = wr.case_maps(kind, shape, wr.case_seed(name, kind))
    t = wr.taps64(mo, fl, mk, H, W, fs)
    addr = t['y0'] * 65536 + t['x0']                                         # [2, N, H, W]
    tiles = addr.view(2, N, H // wr.TILE_H, wr.TILE_H, W // wr.TILE_W, wr.TILE_W).permute(0, 1, 2, 4, 3, 5)
    tiles = tiles.reshape(2, N, -1, wr.TILE_H, wr.TILE_W)
    lanes = torch.stack([torch.stack([tiles[..., r, c] for r, c in wr.lane_pixels(lane)], -1) for lane in range(64)], -2)
    return lanes, t


def test_collapse_cases_collide_as_named():
    lanes, t = _lane_addresses('rowcollapse')
    # same-lane duplicates: the 8 pixels of every lane (one column, 8 rows) share one address, in both branches
    assert bool((lanes == lanes[..., :1]).all())
    # ... and lane / lane + 32 (the same column, the next row) collide as well
    assert bool((lanes[..., :32, :] == lanes[..., 32:, :]).all())
    assert bool(t['live'][1].any()) and bool(t['inr'][1].any()), 'rowcollapse: the flow branch is dead'

    lanes, t = _lane_addresses('colcollapse')
    # full-wave same-address batches: the 32 lanes of a row share one address
    assert bool((lanes[..., :32, :] == lanes[..., :1, :]).all()) and bool((lanes[..., 32:, :] == lanes[..., 32:33, :]).all())
    assert bool(t['live'][1].any()) and bool(t['inr'][1].any())


def test_border_case_samples_the_exact_edges():
    kind, (N, C, H, W, S, fs) = wr.BWD_CASES['border']
    mo, fl, mk = wr.case_maps(kind, wr.BWD_CASES['border'][1], wr.case_seed('border', kind))
    ix = ((mo[..., 0].double() + 1) * W - 1) / 2
    for v in (-1.0, -0.5, 0.0, W - 1.0, W - 0.5, float(W)):
        assert bool((ix == v).any()), v                                       # exact in fp32 and in fp64
    assert bool((ix == ix.round()).any())
    # integer coordinates: zero weights on taps INSIDE the frame (and so inside the window)
    t = wr.taps64(mo, fl, mk, H, W, fs)
    x1_in = (t['x0'][0] + 1 >= 0) & (t['x0'][0] + 1 < W) & (t['y0'][0] >= 0) & (t['y0'][0] < H)
    assert bool((x1_in & ~t['inr'][0, 1]).any())
