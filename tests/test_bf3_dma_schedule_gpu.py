"""GPU: the split-bf16 3x3 kernel spreads the LDS-DMA pieces of a stage's refill over the taps of the following stage
(csrc/conv_bf3_dma.h ``bf3_dma_sched``; profiles/r07_dma_spread.md).  The change reorders loads only, so a layer's output,
mean and rstd are bit-identical however the persistent workgroups walk the tile list, and agree with an fp64 convolution
on the host within the bar of test_gpu_parity.py::test_conv_bf16x3_persistent_walk (InstanceNorm-ed output within 2e-3).

The cases walk every branch of the schedule: every chunk count that changes what a stage's deferred pieces are (a single
chunk padded to two -- every stage is the tile's tail stage; two chunks -- the deferred pieces of stage 0 already belong to
the next tile; an odd count padded; two source segments; many chunks), one workgroup walking every tile (every tile boundary
carries deferred pieces, the next tile's chunk 1 included), workgroups with no tile or a single tile (nothing to carry), and
the 16-row and 4-row tiles.  No further instantiation took the schedule (profiles/r07_dma_spread.md), so there is no case
for one."""
import functools

import pytest
import torch
import torch.nn.functional as F

from conftest import linf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def _problem(segs, cout, n, H, W):
    """Inputs, weights and the InstanceNorm-ed fp64 reference of one layer (host tensors; computed once per shape)."""
    g = torch.Generator().manual_seed(1000 + sum(segs) + cout + H)
    xs = tuple(torch.randn(n, c, H, W, generator=g) * 2 for c in segs)
    w = torch.randn(cout, sum(segs), 3, 3, generator=g) * 0.05
    ref = F.conv2d(F.pad(torch.cat(xs, 1).double(), (1,) * 4, mode='reflect'), w.double())
    return xs, w, F.instance_norm(ref.float())


def _run_walks(dev, monkeypatch, segs, cout, n, H, W, blocks, tall):
    from animateportrait_amd import ops
    from animateportrait_amd.networks import ConvLayer
    monkeypatch.setenv('APAMD_NO_SMALL_TILES', str(tall))
    xs, w, refn = _problem(tuple(segs), cout, n, H, W)
    feats = [ops.Feat(x.to(dev)) for x in xs]
    layer = ConvLayer(list(segs), cout, 3, 1, 1, ops.PAD_REFLECT).to(dev)
    layer.spec.precision = ops.PRECISION_BF16X3
    with torch.no_grad():
        layer.weight.copy_(w)
    monkeypatch.delenv('APAMD_BF3_BLOCKS', raising=False)
    want = layer.run(feats, norm_act=ops.ACT_NONE)
    if blocks is not None:
        monkeypatch.setenv('APAMD_BF3_BLOCKS', str(blocks))
    got = layer.run(feats, norm_act=ops.ACT_NONE)
    assert torch.equal(got.data, want.data)
    assert torch.equal(got.mean, want.mean) and torch.equal(got.rstd, want.rstd)
    gotn = (got.data - got.mean.view(n, cout, 1, 1)) * got.rstd.view(n, cout, 1, 1)
    err = linf(gotn, refn)
    print('segs %s cout %d %dx%dx%d blocks %s tall %d: L-inf of the normalised output vs fp64 = %.3e' % (segs, cout, n, H, W, blocks, tall, err))
    assert err < 2e-3


@pytest.mark.parametrize('tall', [0, 1])
@pytest.mark.parametrize('segs', [(16,), (32,), (48,), (64, 48), (288,)])
def test_dma_schedule_chunk_counts(dev, segs, tall, monkeypatch):
    """1 (padded to 2), 2, 3 (padded to 4), 4 + 3 (padded) and 18 chunks; one workgroup walks all tiles against the default."""
    _run_walks(dev, monkeypatch, segs, 72, 2, 18, 36, 1, tall)


@pytest.mark.parametrize('tall', [0, 1])
@pytest.mark.parametrize('blocks', [1, 3, None])
def test_dma_schedule_tile_walks(dev, blocks, tall, monkeypatch):
    """Partial cout tile (136), partial rows and columns (50 x 70), three images: one workgroup walking every tile, three
    workgroups (fewer than the 8 XCDs), and the default grid."""
    _run_walks(dev, monkeypatch, (64, 48), 136, 3, 50, 70, blocks, tall)


@pytest.mark.parametrize('tall', [0, 1])
def test_dma_schedule_no_next_tile(dev, tall, monkeypatch):
    """One image of 16 x 32 and one cout tile on four workgroups: a workgroup gets no tile, or exactly one with no next tile."""
    _run_walks(dev, monkeypatch, (32,), 64, 1, 16, 32, 4, tall)
