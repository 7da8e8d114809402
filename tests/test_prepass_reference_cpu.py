"""CPU: the restatements of tests/prepass_reference.py, which tests/test_prepass_gpu.py holds the forward streaming passes to, are
themselves checked here against torch in float64 -- and the bound that file puts on the statistics is shown to hold for the
finalizers' unrefined formula exactly where they may use it (mean^2 <= 32 var), and to be missed by far where they may not."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import prepass_reference as pr

STAT_BOUND = 2.0 ** -17
EPS = 1e-5


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize('act', [0, 1, 2])
def test_norm_act_fp64_is_instance_norm(act):
    x = (torch.randn(3, 8, 5, 7, generator=_gen(1)) * 2 + 1.5)
    mean, _, rstd = pr.stats64(x, EPS)
    got = pr.norm_act(x, mean, rstd, act, dtype=torch.float64)
    want = F.instance_norm(x.double(), eps=EPS)
    want = F.relu(want) if act == 1 else (F.leaky_relu(want, 0.2) if act == 2 else want)
    assert float((got - want).abs().max()) <= 1e-12
    # the fp32 flavour is the same formula: it stays within a few fp32 roundings of it
    got32 = pr.norm_act(x, mean.float(), rstd.float(), act)
    assert got32.dtype == torch.float32 and float((got32.double() - want).abs().max()) <= 1e-5
    assert torch.equal(pr.norm_act(x, None, None, 0), x)


def test_split_encode_is_round_to_nearest_even_head_and_fp32_tail():
    # 1 + 2^-8 lies half-way between the bf16 neighbours 1 and 1 + 2^-7: ties go to the even mantissa (1); 1 + 3 * 2^-8 to 1 + 2^-6
    v = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 3.0e-39, 0.0], dtype=torch.float32)
    head, tail = pr.split_encode(v)
    assert head.float().tolist()[:3] == [1.0, 1.0 + 2.0 ** -6, -1.0]
    assert tail.float().tolist()[:3] == [2.0 ** -8, -(2.0 ** -8), -(2.0 ** -8)]
    assert float(head[4]) == 0.0 and float(tail[4]) == 0.0


@pytest.mark.parametrize('shape', [(1, 8, 1, 1), (3, 24, 3, 5), (2, 16, 4, 4)])
def test_pack_unpack_round_trip(shape):
    n, c, h, w = shape
    v = torch.randn(shape, generator=_gen(2)) * 3
    raw = pr.pack_xs(v)
    assert raw.dtype == torch.uint8 and raw.numel() == n * 2 * (c // 8) * (h * w + 1) * 16
    head, tail, closing = pr.unpack_xs(raw, n, c, h, w)
    assert float(((head + tail - v).abs() - v.abs() * 2.0 ** -16).max()) <= 0.0
    assert torch.equal(head, v.to(torch.bfloat16).float())
    assert closing.shape == (n, 2, c // 8, 8) and int(closing.abs().max()) == 0
    # the layout itself, by hand: channel c of pixel p of image i sits at bf16 index (((i*2 + part)*C/8 + c/8)*(HW + 1) + p)*8 + c%8
    words = raw.view(torch.bfloat16)
    for (i, ch, p) in [(0, 0, 0), (n - 1, c - 1, h * w - 1), (n - 1, 3, (h * w) // 2)]:
        for part, plane in enumerate((head, tail)):
            at = (((i * 2 + part) * (c // 8) + ch // 8) * (h * w + 1) + p) * 8 + ch % 8
            assert float(words[at]) == float(plane.reshape(n, c, -1)[i, ch, p])


def test_to_octet_layout():
    x = torch.arange(2 * 16 * 3 * 2, dtype=torch.float32).reshape(2, 16, 3, 2)
    o = pr.to_octet(x)
    assert o.shape == (2, 2, 6, 8)
    assert float(o[1, 1, 4, 5]) == float(x[1, 13, 2, 0])


@pytest.mark.parametrize('c,h,w', [(1, 4, 9), (3, 9, 6), (4, 7, 5)])
def test_rows_expand_reproduces_the_reflect_padded_stem(c, h, w):
    from animateportrait_amd import ops
    g = _gen(3)
    x = torch.randn(2, c, h, w, generator=g).double()
    wt = torch.randn(5, c, 7, 7, generator=g).double()
    want = F.conv2d(F.pad(x, (3, 3, 3, 3), mode='reflect'), wt)
    # the 1 x 7 convolution over the row channels applies the horizontal taps and the horizontal reflection
    rows = F.pad(pr.rows_expand(x, 1), (3, 3, 0, 0), mode='reflect')
    got = F.conv2d(rows, ops.stem_rows_weight(wt))
    assert float((got - want).abs().max()) <= 1e-12
    assert float(pr.rows_expand(x, 1)[:, 7 * c:].abs().max()) == 0.0


@pytest.mark.parametrize('c,h,w', [(2, 1, 5), (3, 3, 4), (4, 7, 3)])
def test_rows_expand_zero_padding(c, h, w):
    from animateportrait_amd import ops
    g = _gen(4)
    x = torch.randn(2, c, h, w, generator=g).double()
    wt = torch.randn(3, c, 7, 7, generator=g).double()
    want = F.conv2d(x, wt, padding=3)
    got = F.conv2d(pr.rows_expand(x, 0), ops.stem_rows_weight(wt), padding=(0, 3))
    assert float((got - want).abs().max()) <= 1e-12


@pytest.mark.parametrize('k', [4, 3])
@pytest.mark.parametrize('h,w', [(2, 2), (6, 10), (14, 4)])
def test_s2d_expand_reproduces_the_stride_2_conv(k, h, w):
    from animateportrait_amd import ops
    g = _gen(5)
    x = torch.randn(2, 8, h, w, generator=g).double()
    wt = torch.randn(4, 8, k, k, generator=g).double()
    want = F.conv2d(x, wt, stride=2, padding=1)
    xe = pr.s2d_expand(x)
    assert xe.shape == (2, 32, h // 2 + 1, w // 2 + 1)
    got = F.conv2d(xe, ops.s2d_weight(wt))
    assert got.shape == want.shape and float((got - want).abs().max()) <= 1e-12


def test_tile_edges_are_uneven_and_cover_the_plane():
    for hw, tiles in [(1, 1), (1, 7), (3, 9), (255, 7), (513, 130), (1024, 23), (4, 8), (130, 130)]:
        e = pr.tile_edges(hw, tiles)
        assert len(e) == tiles + 1 and e[0] == 0 and e[-1] == hw and all(b >= a for a, b in zip(e, e[1:]))
        if hw >= tiles:
            assert all(b > a for a, b in zip(e, e[1:]))
            if tiles > 1:
                assert e[-1] - e[-2] == 1
        if hw >= 4 * tiles and tiles > 2:
            assert len({b - a for a, b in zip(e, e[1:])}) > 1
    x = torch.randn(2, 8, 9, 7, generator=_gen(6))
    p = pr.make_partials(x, 9)
    assert p.shape == (16, 9, 2) and p.dtype == torch.float32
    assert float((p[:, :, 0].double().sum(1) - x.double().reshape(16, -1).sum(1)).abs().max()) <= 1e-5


def _planes(ratio, hw, nplanes, seed):
    """Planes with mean^2 / var = ratio to the rounding of the fp32 data: unit-variance noise around a constant."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((nplanes, hw))
    z = (z - z.mean(1, keepdims=True)) / z.std(1, keepdims=True)
    x = (np.sqrt(ratio) * 1.00037 + z).astype(np.float32)        # (not a round number: a round mean makes the one-tile sums exact)
    return torch.from_numpy(x).reshape(1, nplanes, 1, hw)


@pytest.mark.parametrize('tiles', [1, 9, 130])
@pytest.mark.parametrize('hw', [513, 4096])
def test_unrefined_statistics_hold_the_bound_where_no_recompute_is_due(tiles, hw):
    """mean^2 / var just under the threshold of 32: q / HW carries (1 + 32) var and mean^2 carries 32 var, each known to 2^-24
    relative per fp32 tile sum, so var is off by at most (33 + 2 * 32) * 2^-24 var and rstd by half of that, 0.38 * 2^-17."""
    x = _planes(31.5, hw, 64, 7)
    mean64, var64, rstd64 = pr.stats64(x, EPS)
    assert float((mean64 ** 2 / var64).max()) < pr.REFINE_RATIO and float((mean64 ** 2 / var64).min()) > 31.0
    mean_u, rstd_u = pr.unrefined_stats(pr.make_partials(x, tiles), hw, EPS)
    rel = ((rstd_u - rstd64).abs() / rstd64).numpy()
    assert rel.max() < STAT_BOUND
    assert float(((mean_u - mean64).abs() / mean64.abs()).max()) <= 2.0 ** -24


@pytest.mark.parametrize('tiles', [1, 9, 130])
def test_unrefined_statistics_miss_the_bound_on_ill_conditioned_planes(tiles):
    """mean^2 / var = 1e6: the same formula is wrong by more than 100 bounds, so a kernel that skipped the recompute from the data
    (or read the data at a wrong stride) cannot pass the GPU test's 2^-17.  The miss of a single plane is a sum of rounding errors
    of either sign and can happen to be small, so the statement is about the set: the worst plane misses by more than 100 bounds
    and nine planes in ten miss the bound itself.  (The GPU test asserts the first on the very planes it uses.)"""
    hw = 4096
    x = _planes(1.0e6, hw, 64, 8)
    _, _, rstd64 = pr.stats64(x, EPS)
    _, rstd_u = pr.unrefined_stats(pr.make_partials(x, tiles), hw, EPS)
    rel = ((rstd_u - rstd64).abs() / rstd64).numpy()
    assert rel.max() > 100 * STAT_BOUND
    assert (rel > STAT_BOUND).mean() >= 0.9
