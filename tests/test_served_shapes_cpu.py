"""CPU (-m "not gpu"): the regions the bf16 edge-layer kernels serve, as their C-ABI predicates state them.  ops.py trusts every
*_ok() answer and calls the kernel with no other check, so a predicate that accepts a shape its kernel cannot compute is a silently
wrong gradient.  Each table lists shapes just inside and just outside every limit of one predicate; tests/test_served_shapes_gpu.py
runs the kernels at the corners.  Also: the cached answer of ops.wgrad_xs_ok follows every input the uncached one depends on."""
import ctypes

import pytest
import torch


@pytest.fixture(scope='module')
def lib():
    from animateportrait_amd import _capi
    return _capi.lib()


# ap_conv_head_dgrad_bf16_ok(N, C, H, W): C a multiple of 32, H, W >= 2, H W <= 1156 (the 32 output planes in LDS) and
# (H + 3) (W + 8) <= 7 * 256 (the zero-framed gradient rows dgrad_head_kernel stages with 7 loads per thread)
HEAD_DGRAD = [
    ((2, 512, 31, 31), 1),     # the PatchGAN's maps
    ((40, 96, 34, 34), 1),
    ((1, 32, 2, 2), 1),        # smallest map
    ((1, 32, 1, 2), 0),
    ((1, 32, 2, 1), 0),
    ((1, 32, 33, 35), 1),      # H W = 1155
    ((1, 32, 17, 68), 1),      # H W = 1156
    ((1, 32, 17, 69), 0),      # H W = 1173
    ((1, 32, 2, 350), 1),      # (H + 3) (W + 8) = 1790
    ((1, 32, 2, 351), 0),      # 1795
    ((1, 32, 4, 248), 1),      # 1792
    ((1, 32, 4, 249), 0),      # 1799
    ((1, 32, 6, 191), 1),      # 1791
    ((1, 32, 6, 192), 0),      # 1800: H W = 1152 passes the plane bound, the staging does not fit
    ((1, 32, 4, 289), 0),      # 2079, H W = 1156
    ((1, 32, 289, 4), 0),      # 3504
    ((1, 64, 34, 34), 1),
    ((1, 16, 34, 34), 0),      # C not a multiple of 32
    ((1, 48, 34, 34), 0),
    ((0, 32, 34, 34), 0),
]

# ap_wgrad_d0_bf16_ok(N, M, Cin, H, W): M = 64, Cin 1 | 2, even H >= 2, W a multiple of 32, W <= 512, and the two new input rows of
# a tile in two 16-byte loads per thread: Cin * 4 * ((W / 2 + 16) / 8) * 2 <= 512 -- W <= 480 for two channels
WGRAD_D0 = [
    ((1, 64, 2, 2, 448), 1),
    ((1, 64, 2, 2, 480), 1),   # the load budget met exactly
    ((1, 64, 2, 2, 512), 0),
    ((1, 64, 1, 2, 512), 1),
    ((1, 64, 1, 2, 544), 0),
    ((1, 64, 1, 2, 32), 1),
    ((1, 64, 1, 2, 16), 0),
    ((1, 64, 1, 2, 496), 0),   # not a multiple of 32
    ((1, 64, 1, 1, 32), 0),    # odd H
    ((1, 64, 1, 3, 32), 0),
    ((1, 64, 1, 0, 32), 0),
    ((1, 64, 3, 2, 32), 0),
    ((1, 32, 1, 2, 32), 0),
    ((0, 64, 1, 2, 32), 0),
    ((257, 64, 2, 256, 256), 1),
]

# ap_conv_d0_fwd_bf16_ok(N, Cin, Cout, H, W): Cin 1 | 2 -> 64, even H >= 2, W a multiple of 4 in 8..256
CONV_D0 = [
    ((1, 1, 64, 2, 8), 1),
    ((1, 2, 64, 2, 256), 1),
    ((1, 2, 64, 2, 252), 1),   # W / 4 odd
    ((1, 1, 64, 2, 4), 0),
    ((1, 1, 64, 2, 260), 0),
    ((1, 1, 64, 2, 10), 0),
    ((1, 1, 64, 3, 8), 0),     # odd H
    ((1, 1, 64, 1, 8), 0),
    ((1, 1, 64, 0, 8), 0),
    ((1, 3, 64, 2, 8), 0),
    ((1, 1, 32, 2, 8), 0),
    ((0, 1, 64, 2, 8), 0),
]

# ap_conv_final_dgrad_bf16_ok(N, C, H, W): C 32 | 64, H >= 1, W a multiple of 16 in 16..256
FINAL_DGRAD = [
    ((1, 32, 1, 16), 1),
    ((1, 64, 1, 256), 1),
    ((1, 64, 3, 16), 1),
    ((1, 32, 0, 16), 0),
    ((1, 32, 4, 8), 0),
    ((1, 32, 4, 24), 0),
    ((1, 32, 4, 272), 0),
    ((1, 48, 4, 16), 0),
    ((1, 16, 4, 16), 0),
    ((0, 32, 4, 16), 0),
]

# ap_wgrad_k7_bf16_ok(N, wide C, narrow C, H, W, final form): wide 32 | 64, narrow 1 | 3 (stem) or 1 (final), H >= 4,
# W a multiple of 16 in 16..256
WGRAD_K7 = [
    ((1, 64, 3, 4, 16, 0), 1),
    ((1, 32, 1, 4, 256, 0), 1),
    ((257, 64, 3, 4, 16, 0), 1),
    ((1, 64, 3, 3, 16, 0), 0),
    ((1, 64, 3, 4, 8, 0), 0),
    ((1, 64, 3, 4, 24, 0), 0),
    ((1, 64, 3, 4, 272, 0), 0),
    ((1, 48, 3, 4, 16, 0), 0),
    ((1, 64, 2, 4, 16, 0), 0),
    ((1, 64, 1, 4, 16, 1), 1),
    ((1, 32, 1, 4, 256, 1), 1),
    ((1, 64, 3, 4, 16, 1), 0),
    ((1, 64, 1, 3, 16, 1), 0),
    ((0, 64, 1, 4, 16, 1), 0),
]

# ap_instnorm_bwd_split_ok(C, H, W, fold): C % 8 == 0, W % 8 == 0, H * W <= 4096, H >= 3 unfolded, H >= 4 with the pad-1 fold
# (the fold of padded rows 0 and H + 1 is done by the lanes of rows 1 and H - 2, one border row each: with H = 3 they coincide)
INBWD_SPLIT = [
    ((64, 8, 512, 0), 1),      # H W = 4096 either way round
    ((64, 512, 8, 0), 1),
    ((64, 64, 64, 1), 1),
    ((64, 9, 456, 0), 0),      # 4104
    ((64, 64, 72, 0), 0),
    ((64, 2, 8, 0), 0),
    ((8, 3, 8, 0), 1),
    ((8, 3, 8, 1), 0),
    ((8, 4, 8, 1), 1),
    ((64, 32, 32, 1), 1),      # 1024 pixels: the 256-thread kernel
    ((64, 13, 80, 1), 1),      # 1040: the 1024-thread kernel
    ((4, 32, 32, 0), 0),
    ((12, 32, 32, 0), 0),
    ((64, 32, 12, 0), 0),
    ((64, 32, 4, 0), 0),
    ((64, 32, 32, 2), 0),
]


def _ids(rows):
    return ['x'.join(map(str, a)) + '->%d' % e for a, e in rows]


@pytest.mark.parametrize('args,expect', HEAD_DGRAD, ids=_ids(HEAD_DGRAD))
def test_head_dgrad_served_region(lib, args, expect):
    assert lib.ap_conv_head_dgrad_bf16_ok(*args) == expect


@pytest.mark.parametrize('args,expect', WGRAD_D0, ids=_ids(WGRAD_D0))
def test_wgrad_d0_served_region(lib, args, expect):
    assert lib.ap_wgrad_d0_bf16_ok(*args) == expect


@pytest.mark.parametrize('args,expect', CONV_D0, ids=_ids(CONV_D0))
def test_conv_d0_served_region(lib, args, expect):
    assert lib.ap_conv_d0_fwd_bf16_ok(*args) == expect


@pytest.mark.parametrize('args,expect', FINAL_DGRAD, ids=_ids(FINAL_DGRAD))
def test_final_dgrad_served_region(lib, args, expect):
    assert lib.ap_conv_final_dgrad_bf16_ok(*args) == expect


@pytest.mark.parametrize('args,expect', WGRAD_K7, ids=_ids(WGRAD_K7))
def test_wgrad_k7_served_region(lib, args, expect):
    assert lib.ap_wgrad_k7_bf16_ok(*args) == expect


@pytest.mark.parametrize('args,expect', INBWD_SPLIT, ids=_ids(INBWD_SPLIT))
def test_instnorm_bwd_split_served_region(lib, monkeypatch, args, expect):
    monkeypatch.delenv('APAMD_NO_INBWD_SPLIT', raising=False)
    assert lib.ap_instnorm_bwd_split_ok(*args) == expect


def test_workspace_queries_refuse_what_the_predicates_refuse(lib):
    """The workspace sizes are planned by the same code as the predicates: a shape outside the region has no size."""
    assert lib.ap_wgrad_d0_bf16_workspace_floats(1, 64, 2, 2, 480) > 0
    assert lib.ap_wgrad_d0_bf16_workspace_floats(1, 64, 2, 2, 512) < 0
    assert lib.ap_wgrad_k7_bf16_workspace_floats(1, 64, 3, 4, 256, 0) > 0
    assert lib.ap_wgrad_k7_bf16_workspace_floats(1, 64, 3, 3, 256, 0) < 0
    assert lib.ap_conv_final_dgrad_bf16_workspace_floats(1, 32, 1, 16) > 0
    assert lib.ap_conv_final_dgrad_bf16_workspace_floats(1, 32, 1, 8) < 0


def test_wgrad_xs_route_cache_follows_every_input(monkeypatch, lib):
    """ops.wgrad_xs_ok caches the C-side answer per layer geometry.  The package mode (DEFAULT_PRECISION when precision is None),
    the sources' head-only copies, the module switches and the environment switches the library reads per call all change that
    answer: flipped one by one in one process, the cached answer is the uncached one of a fresh descriptor."""
    from animateportrait_amd import ops
    # descriptors only: the plan reads shapes and which pointers are set, never the memory behind them
    monkeypatch.setattr(ops, '_require_device', lambda *a, **k: None)
    monkeypatch.setattr(ops, '_WGRAD_XS_OK', {})
    for v in ops.plan_switch_names():
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setattr(ops, 'DEFAULT_PRECISION', ops.PRECISION_BF16X3)
    monkeypatch.setattr(ops, 'XS_WGRAD', True)
    monkeypatch.setattr(ops, 'XS_DIRECT', True)
    n, c, h, w = 2, 64, 32, 32
    src = ops.Feat(torch.zeros(n, c, h, w))
    src.xs = torch.zeros(16, dtype=torch.uint8)        # the forward pass's split copy (its pointer is all the plan reads)
    geom = (3, 1, 1, ops.PAD_ZERO, (n, 64, h, w))

    def check(precision, expect):
        cached = ops.wgrad_xs_ok(*geom, [src], precision)
        d = ops._wgrad_desc(*geom, None, [src], precision)
        fresh = ops.XS_DIRECT and lib.ap_conv2d_wgrad_xs_ok(ctypes.byref(d)) == 1
        assert cached == fresh == expect, (precision, ops.DEFAULT_PRECISION, cached, fresh, expect)

    check(None, True)
    check(ops.PRECISION_BF16X3, True)
    monkeypatch.setattr(ops, 'DEFAULT_PRECISION', ops.PRECISION_FP32)
    check(None, False)                                  # the package mode is the precision
    monkeypatch.setattr(ops, 'DEFAULT_PRECISION', ops.PRECISION_BF16)
    check(ops.PRECISION_BF16X3, False)                  # plain-bf16 package mode: head-only copies, which bf16x3 cannot read
    monkeypatch.setattr(ops, 'DEFAULT_PRECISION', ops.PRECISION_BF16X3)
    check(None, True)
    src.xs_heads_only = True
    check(None, False)
    src.xs_heads_only = False
    check(None, True)
    monkeypatch.setenv('APAMD_NO_XS_DIRECT', '1')
    check(None, False)
    monkeypatch.setenv('APAMD_NO_XS_DIRECT', '0')
    check(None, True)
    monkeypatch.setenv('APAMD_NO_XS_WGRAD', '1')
    check(None, True)                                   # (read by the re-tiling route, not by this one)
    monkeypatch.delenv('APAMD_NO_XS_WGRAD')
    monkeypatch.setenv('APAMD_NO_BF16X3', '1')
    check(None, False)
    monkeypatch.delenv('APAMD_NO_BF16X3')
    check(None, True)
    monkeypatch.setattr(ops, 'XS_WGRAD', False)         # the descriptor then carries no forward copies
    check(None, False)
    monkeypatch.setattr(ops, 'XS_WGRAD', True)
    check(None, True)
    monkeypatch.setattr(ops, 'XS_DIRECT', False)
    check(None, False)
    monkeypatch.setattr(ops, 'XS_DIRECT', True)
    check(None, True)


# ---------------------------------------------------------------- the bf16-stored trunk outputs and the strip data gradient
# (tests/test_bf16_store_gpu.py runs the kernels at these shapes)

TALL, SHORT = 'Bf3Cfg<1, 3, 1, 2, 4, 4> bf16', 'Bf3Cfg<1, 3, 1, 2, 4, 1> bf16'

# ap_conv2d_bf16out_ok(d): plain-bf16 arithmetic on the dense 3x3 stride-1 tiles (Bf3Cfg::OB16, both tile heights), one launch
# (precision, segments, cout, k, stride, pad, pad mode, transposed, output_padding, N, H, W, tall tiles forced, expected, kernel)
BF16OUT = [
    ('bf16', (64,), 64, 3, 1, 1, 'reflect', 0, 0, 2, 64, 64, 1, 1, TALL),
    ('bf16', (64,), 64, 3, 1, 1, 'reflect', 0, 0, 1, 8, 37, 0, 1, SHORT),
    ('bf16', (32, 32), 80, 3, 1, 1, 'zero', 0, 0, 3, 19, 66, 1, 1, TALL),
    ('bf16', (48, 16, 32), 64, 3, 1, 1, 'reflect', 0, 0, 1, 5, 45, 0, 1, SHORT),
    ('bf16', (128,), 40, 3, 1, 1, 'zero', 0, 0, 1, 6, 32, 0, 1, SHORT),       # 40 outputs: served with >= 128 inputs
    ('bf16', (64,), 64, 3, 1, 2, 'zero', 0, 0, 1, 4, 32, 0, 1, SHORT),        # the data-gradient form (full correlation, pad 2)
    ('bf16', (64,), 32, 3, 1, 1, 'zero', 0, 0, 1, 8, 32, 0, 0, None),        # 32 outputs from 64 inputs: fp32 path
    ('bf16', (16,), 64, 3, 1, 1, 'zero', 0, 0, 1, 8, 32, 0, 0, None),        # 16 inputs: fp32 path
    ('bf16x3', (64,), 64, 3, 1, 1, 'reflect', 0, 0, 1, 8, 32, 0, 0, SHORT[:-5]),
    ('fp32', (64,), 64, 3, 1, 1, 'reflect', 0, 0, 1, 8, 32, 0, 0, None),
    ('bf16', (64,), 64, 3, 2, 1, 'zero', 0, 0, 1, 16, 64, 0, 0, None),        # stride 2
    ('bf16', (64,), 64, 4, 1, 1, 'zero', 0, 0, 1, 16, 64, 0, 0, None),        # 4x4
    ('bf16', (64,), 64, 7, 1, 3, 'reflect', 0, 0, 1, 16, 64, 0, 0, None),     # 7x7 (the stem's size)
    ('bf16', (64,), 64, 3, 2, 1, 'zero', 1, 1, 1, 16, 32, 0, 0, None),        # transposed
]


def _bf16out_ids(rows):
    return ['%s %s->%d k%d s%d%s %dx%dx%d%s' % (r[0], '+'.join(map(str, r[1])), r[2], r[3], r[4], ' T' if r[7] else '',
                                               r[9], r[10], r[11], ' tall' if r[12] else '') for r in rows]


@pytest.mark.parametrize('row', BF16OUT, ids=_bf16out_ids(BF16OUT))
def test_bf16out_served_region(lib, monkeypatch, row):
    from animateportrait_amd import ops
    prec, segs, cout, k, stride, pad, mode, tr, op, n, h, w, tall, expect, kern = row
    if tall:
        monkeypatch.setenv('APAMD_NO_SMALL_TILES', '1')
    else:
        monkeypatch.delenv('APAMD_NO_SMALL_TILES', raising=False)
    spec = ops.ConvSpec(segs, cout, k, stride, pad, ops.PAD_REFLECT if mode == 'reflect' else ops.PAD_ZERO, bool(tr), op,
                        ops.W_IOHW if tr else ops.W_OIHW)
    spec.precision = ops.PRECISION_BY_NAME[prec]
    d = spec.desc(n, h, w)
    assert lib.ap_conv2d_bf16out_ok(ctypes.byref(d)) == expect
    if kern is not None:
        buf = ctypes.create_string_buffer(96)
        assert lib.ap_conv2d_kernel_name(ctypes.byref(d), buf, 96) == 0
        assert buf.value.decode() == kern


def _strip_spec(c, cout, prec):
    """the data-gradient operator of Conv2d(cout, c, 3) after ReflectionPad2d(1) (autograd._dgrad_spec): a gradient of c channels
    in, the padded-coordinate gradient of cout channels out"""
    from animateportrait_amd import ops
    spec = ops.ConvSpec([c], cout, 3, 1, 2, ops.PAD_ZERO, False, 0, ops.W_IOHW, True)
    spec.precision = ops.PRECISION_BY_NAME[prec]
    return spec


# ops.dgrad_strip_eligible(spec, g): W = 32 m (padded width 32 m + 2), H >= 4, C % 8 == 0, a plain gradient, and the operator on the
# split-bf16 path -- which takes sources of 32 or more channels in multiples of 16 (ap_conv2d_wants_presplit), so 32 is the
# smallest gradient width served and C % 8 never decides alone
# (precision, N, C, H, W, output channels, virtual gradient, expected)
STRIP = [
    ('bf16', 1, 32, 4, 32, 64, 0, 1),
    ('bf16x3', 3, 32, 4, 32, 64, 0, 1),
    ('bf16', 1, 64, 4, 256, 64, 0, 1),
    ('bf16', 2, 256, 5, 96, 72, 0, 1),
    ('bf16', 1, 128, 7, 128, 16, 0, 1),      # 16 outputs from 128 inputs (the landmark segment of a ResnetBlock2 layer)
    ('bf16', 1, 64, 64, 64, 64, 0, 1),
    ('bf16', 1, 64, 4, 30, 64, 0, 0),
    ('bf16', 1, 64, 4, 34, 64, 0, 0),
    ('bf16', 1, 64, 4, 48, 64, 0, 0),
    ('bf16', 1, 64, 4, 16, 64, 0, 0),        # W < 32
    ('bf16', 1, 64, 3, 32, 64, 0, 0),
    ('bf16', 1, 12, 4, 32, 64, 0, 0),
    ('bf16', 1, 16, 4, 32, 64, 0, 0),        # C % 8 == 0, but below the split path's 32 inputs
    ('bf16', 1, 24, 4, 32, 64, 0, 0),
    ('bf16', 1, 64, 4, 32, 8, 0, 0),         # 8 outputs from 64 inputs: fp32 path
    ('fp32', 1, 64, 4, 32, 64, 0, 0),
    ('bf16', 1, 64, 4, 32, 64, 1, 0),
]


@pytest.mark.parametrize('row', STRIP, ids=['%s N%d C%d %dx%d ->%d%s->%d' % (r[:6] + (' virtual' if r[6] else '', r[7])) for r in STRIP])
def test_dgrad_strip_eligible_region(lib, monkeypatch, row):
    from animateportrait_amd import ops
    monkeypatch.delenv('APAMD_NO_BF16X3', raising=False)
    prec, n, c, h, w, cout, virt, expect = row
    spec = _strip_spec(c, cout, prec)
    g = torch.zeros(n, c, h, w)
    feat = ops.Feat(g, torch.zeros(n * c), torch.ones(n * c)) if virt else ops.Feat(g)
    assert ops.dgrad_strip_eligible(spec, feat) == bool(expect)
    if expect:
        # ... and the two launches it stands for exist: the padded map's main window and the transposed column strip
        d = spec.desc(n, h, w)
        assert lib.ap_conv2d_wants_presplit(ctypes.byref(d)) == 1
        t = spec.desc(n, 2, h)
        assert lib.ap_conv2d_wants_presplit(ctypes.byref(t)) == 1
        assert spec.out_size(h, w) == (h + 2, w + 2) and spec.out_size(2, h) == (4, h + 2)


AP_ERR_INVALID, AP_ERR_UNSUPPORTED = -1, -2
_DUMMY = 1 << 20        # never dereferenced: every call below is refused before anything is launched


def _view_desc(spec, n, h, w):
    d = spec.desc(n, h, w)
    d.presplit = 1 if spec.precision != 0 else 0
    for i in range(d.nsrc):
        d.src[i].data = _DUMMY
    return d


def _view(nstride, cstride, rstride, xstride, y_off, x_off, oh, ow):
    from animateportrait_amd import _capi
    v = _capi.ApOutView()
    v.nstride, v.cstride, v.rstride, v.xstride, v.y_off, v.x_off, v.OH, v.OW = nstride, cstride, rstride, xstride, y_off, x_off, oh, ow
    return v


# windows outside the 8 x 34 output of a 3x3 pad-1 layer over 8 x 34
BAD_WINDOWS = [(0, 34), (8, 0), (9, 34), (8, 35), (-1, 34), (8, -2)]


@pytest.mark.parametrize('bf16out', [0, 1], ids=['fp32 out', 'bf16 out'])
@pytest.mark.parametrize('ohw', BAD_WINDOWS, ids=['%dx%d' % a for a in BAD_WINDOWS])
def test_fwd_view_refuses_windows_outside_the_output(lib, bf16out, ohw):
    from animateportrait_amd import ops
    spec = ops.ConvSpec([64], 64, 3, 1, 1, ops.PAD_ZERO)
    spec.precision = ops.PRECISION_BF16 if bf16out else ops.PRECISION_BF16X3
    assert spec.out_size(8, 34) == (8, 34)
    d = _view_desc(spec, 2, 8, 34)
    v = _view(64 * 8 * 34, 8 * 34, 34, 1, 0, 0, *ohw)
    fn = lib.ap_conv2d_fwd_view_bf16out if bf16out else lib.ap_conv2d_fwd_view
    assert fn(ctypes.byref(d), ctypes.byref(v), _DUMMY, None, _DUMMY, None) == AP_ERR_INVALID
    assert b'window' in lib.ap_last_error()


# plans that take no output window: (precision, segments, cout, k, stride, pad, transposed, output_padding, H, W)
NO_VIEW_PLANS = [
    ('fp32', (64,), 64, 3, 1, 1, 0, 0, 8, 32),         # the fp32 implicit-GEMM kernel
    ('bf16x3', (64,), 32, 3, 1, 1, 0, 0, 8, 32),       # 32 outputs: fp32 kernel in split mode too
    ('bf16x3', (64,), 64, 3, 2, 1, 1, 1, 8, 16),       # transposed, even output: the four phases in one tile (conv_ph4)
    ('bf16x3', (64,), 64, 3, 2, 0, 1, 1, 8, 16),       # transposed, even output, pad 0: fused sub-pixel phases
    ('bf16x3', (64,), 64, 3, 2, 1, 1, 0, 8, 16),       # transposed, odd output: four launches
]


@pytest.mark.parametrize('bf16out', [0, 1], ids=['fp32 out', 'bf16 out'])
@pytest.mark.parametrize('row', NO_VIEW_PLANS, ids=['%s k%d s%d p%d%s op%d' % (r[0], r[3], r[4], r[5], ' T' if r[6] else '', r[7])
                                                    for r in NO_VIEW_PLANS])
def test_fwd_view_refuses_plans_without_windows(lib, bf16out, row):
    from animateportrait_amd import ops
    prec, segs, cout, k, stride, pad, tr, op, h, w = row
    spec = ops.ConvSpec(segs, cout, k, stride, pad, ops.PAD_ZERO, bool(tr), op, ops.W_IOHW if tr else ops.W_OIHW)
    spec.precision = ops.PRECISION_BY_NAME[prec]
    if bf16out and spec.precision == ops.PRECISION_BF16X3:
        spec.precision = ops.PRECISION_BF16
    ho, wo = spec.out_size(h, w)
    d = _view_desc(spec, 1, h, w)
    v = _view(cout * ho * wo, ho * wo, wo, 1, 0, 0, ho, wo)       # the whole output: only the plan is refused
    fn = lib.ap_conv2d_fwd_view_bf16out if bf16out else lib.ap_conv2d_fwd_view
    assert fn(ctypes.byref(d), ctypes.byref(v), _DUMMY, None, _DUMMY, None) == AP_ERR_UNSUPPORTED
    assert (b'bf16out_ok' if bf16out else b'single-launch') in lib.ap_last_error()
    assert lib.ap_conv2d_bf16out_ok(ctypes.byref(d)) == 0
