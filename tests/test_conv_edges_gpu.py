"""GPU (-m gpu): every forward convolution route at the edges of its selection (csrc/conv_plan.hip: make_plan; csrc/conv_fwd.hip:
the launchers), against fp64.

tests/test_conv_plan_cpu.py pins what the planner ANSWERS; this module RUNS the kernels there.  Each case of CASES is one small
layer and states what it is meant to launch, in the words of ap_conv2d_fwd_route (ops.conv_fwd_route): one word group per launch,
with the choices made at launch time -- the head kernel's rows per workgroup, the tap GEMM and its band height, the statistics
fall-back of the two narrow-output kernels, the kernel of every sub-pixel phase, the space-to-depth tap sets and the persistent
workgroup count.  A planner or launcher change that moves a case off its kernel fails the first assertion instead of silently
testing something else; tests/test_conv_edges_cpu.py checks without a GPU that the cases together name every kernel word of
ap_conv2d_fwd_route_names, and that every stated route is the query's answer.

Per case (test_conv_edge):
  1 route       the stated string is the query's answer;
  2 value       against an fp64 CPU evaluation of the same layer: the sources' InstanceNorm + activation (from the fp32 statistics
                the kernel is handed), padding, bias, epilogue activation.  Gaussian operands with a non-zero mean, a distinct bias
                per channel.  Bars, the project's own, times max|ref| before the activation: 2e-6 for the exact-fp32 kernels, 5e-5
                for split bf16, and for plain bf16 2e-5 against the fp64 sum of the bf16-ROUNDED operands (plain sources there);
                a bf16-stored output must lie between the bf16 roundings of ref - bar and ref + bar (the store rounds monotonically);
  3 poison      the C entry point is called directly: y and the statistics buffer NaN-filled with a 4096-float NaN tail each, the
                packed image exactly ap_conv2d_packed_floats long and followed by 4096 NaN floats.  Afterwards the tails are
                bit-for-bit NaN, and y and every one of the N * Cout * tiles * 2 statistics slots are finite;
  4 statistics  finalised through the product path (ops.Feat.mean / rstd); the normalised output against F.instance_norm of the
                fp64 result: 1e-4 for fp32, 2e-3 for split bf16;
  5 walk        split-bf16 routes: APAMD_BF3_BLOCKS = 1 and one count that does not divide the tile count of any launch (every
                split-bf16 case has at least three tiles per launch); each
                result bit-equal to the default launch, output and statistics alike;
  6 bits        two calls with identical inputs give identical bits.

kind: 'rows' is a 7x7 stem run as the 1 x 7 row form over its row expansion, 's2d' a 4x4 / 3x3 stride-2 layer run as the 2x2
space-to-depth form; the case states the original layer, the reference is the original layer's.

The final-layer shapes of tests/test_final_layer_gpu.py, the backward kernels and the test_served_shapes_* edge kernels are not
repeated here."""
import collections
import ctypes

import pytest
import torch
import torch.nn.functional as F

from conftest import linf

FP32, X3, B16 = 0, 1, 2
ZERO, REFLECT = 0, 1
NONE, RELU, LRELU = 0, 1, 2
OIHW, IOHW = 0, 1
PLAIN, OCTET, OB16 = 0, 1, 2
TAIL_FLOATS = 4096

# vsrc: activation of a virtual first source act(IN(raw)), or None: plain;  stats: a statistics buffer is passed;  form: PLAIN | OCTET |
# OB16;  refused: the entry point's (and the query's) refusal code for this form instead of a route
Case = collections.namedtuple('Case', 'name prec segs cout k stride pad mode tr op layout flip shape vsrc stats form kind act refused route')


def c(route, prec, segs, cout, k, shape, stride=1, pad=None, mode=ZERO, tr=False, op=0, layout=None, flip=False, vsrc=None,
      stats=False, form=PLAIN, kind='plain', act=None, refused=None):
    segs = (segs,) if isinstance(segs, int) else tuple(segs)
    pad = (k - 1) // 2 if pad is None else pad
    layout = (IOHW if tr else OIHW) if layout is None else layout
    act = (NONE if stats else LRELU) if act is None else act
    name = '%s %s->%d k%d s%d p%d%s %s' % (('fp32', 'bf16x3', 'bf16')[prec], '+'.join(map(str, segs)), cout, k, stride, pad,
                                           'r' if mode == REFLECT else 'z', 'x'.join(map(str, shape)))
    name += ''.join([' T op%d' % op if tr else '', ' iohw' if layout == IOHW and not tr else '', ' oihw' if layout == OIHW and tr else '',
                     ' flip' if flip else '', ' vsrc%d' % vsrc if vsrc is not None else '', ' stats' if stats else '',
                     ('', ' octet', ' ob16')[form], ' ' + kind if kind != 'plain' else '', ' refused' if refused else ''])
    return Case(name, prec, segs, cout, k, stride, pad, mode, tr, op, layout, flip, tuple(shape), vsrc, stats, form, kind, act, refused, route)


T2 = dict(stride=2, tr=True)
CASES = [
    # ---- head (Cin >= 64, one output, 4x4 pad 1, W <= 31): every RB at the smallest N x H, N <= 3, that the cost rule selects it for
    # at 256 CUs -- the kernel bounds W, not H, so these are tall 4-wide maps; Hout is never a multiple of RB -- and RB = 4 on the
    # PatchGAN's 31-row output at N = 24; W = 31 | 32, W = 2, a virtual source, and statistics (the general kernel)
    c('head<2>', FP32, 64, 1, 4, (1, 6, 31), pad=1),
    c('igemm ConvCfg<8,1,4,1,1,4,2> taps=16', FP32, 64, 1, 4, (1, 6, 32), pad=1),
    c('head<2>', FP32, 64, 1, 4, (2, 9, 2), pad=1),
    c('head<3>', FP32, 64, 1, 4, (1, 515, 4), pad=1),
    c('head<4>', FP32, 64, 1, 4, (1, 770, 4), pad=1),
    c('head<4>', FP32, 64, 1, 4, (24, 32, 8), pad=1),
    c('head<5>', FP32, 64, 1, 4, (3, 342, 4), pad=1),
    c('head<6>', FP32, 64, 1, 4, (1, 1282, 4), pad=1),
    c('head<10>', FP32, 64, 1, 4, (3, 512, 4), pad=1),
    c('head<2>', X3, 128, 1, 4, (2, 12, 20), pad=1, vsrc=LRELU),
    c('igemm ConvCfg<8,1,4,1,1,4,2> taps=16', FP32, 64, 1, 4, (2, 12, 20), pad=1, stats=True),

    # ---- tsmall (transposed 4x4 stride 2 pad 1, 1..4 outputs, IOHW): every width, maps of 1 x 1 and around the 8 x 32 tile;
    # statistics, Cout = 5 and output_padding = 1 leave it
    c('tsmall<1>', FP32, 16, 1, 4, (2, 1, 1), pad=1, **T2),
    c('tsmall<2>', FP32, 16, 2, 4, (1, 8, 32), pad=1, **T2),
    c('tsmall<4>', FP32, 16, 3, 4, (1, 9, 33), pad=1, vsrc=LRELU, **T2),
    c('tsmall<4>', FP32, 16, 4, 4, (2, 7, 45), pad=1, **T2),
    c('igemm ConvCfg<8,1,0,1,1,4,2> taps=4; igemm ConvCfg<8,1,0,1,1,4,2> taps=4; igemm ConvCfg<8,1,0,1,1,4,2> taps=4; igemm ConvCfg<8,1,0,1,1,4,2> taps=4', FP32, 16, 2, 4, (1, 9, 33), pad=1, stats=True, **T2),
    c('igemm ConvCfg<8,1,0,1,1,4,2> taps=4; igemm ConvCfg<8,1,0,1,1,4,2> taps=4; igemm ConvCfg<8,1,0,1,1,4,2> taps=4; igemm ConvCfg<8,1,0,1,1,4,2> taps=4', FP32, 16, 5, 4, (1, 9, 33), pad=1, **T2),
    c('igemm ConvCfg<8,1,0,1,1,4,2> taps=4; igemm ConvCfg<8,1,0,1,1,4,2> taps=4; igemm ConvCfg<8,1,0,1,1,4,2> taps=4; igemm ConvCfg<8,1,0,1,1,4,2> taps=4', FP32, 16, 2, 4, (1, 9, 33), pad=1, op=1, **T2),

    # ---- small (3x3, one source of <= 16 channels, 8 | 16 outputs): stride 1 staged, stride 2 gathering
    c('small<1,8> staged', FP32, 1, 8, 3, (2, 1, 1)),
    c('small<1,16> staged', FP32, 5, 16, 3, (1, 2, 2), mode=REFLECT),
    c('small<1,8> staged', FP32, 16, 8, 3, (1, 8, 32), mode=REFLECT, stats=True),
    c('igemm ConvCfg<2,1,3,1,1,4,2> taps=9', FP32, 17, 16, 3, (1, 8, 32)),
    c('small<1,16> staged', FP32, 16, 16, 3, (2, 9, 33), vsrc=RELU, stats=True),
    c('small<2,16> gather', FP32, 1, 16, 3, (1, 9, 33), stride=2),
    c('small<2,8> gather', FP32, 5, 8, 3, (2, 17, 65), stride=2, stats=True),
    c('small<2,16> gather', FP32, 16, 16, 3, (1, 8, 32), stride=2, mode=REFLECT),
    c('small<2,8> gather', FP32, 16, 8, 3, (1, 1, 1), stride=2),
    c('small<2,16> gather', X3, 8, 16, 3, (1, 9, 33), stride=2, vsrc=LRELU, stats=True),

    # ---- direct (7x7 'same', 1..4 outputs): cop 1 | 4, one to three segments with a 1-channel one, the reflection limit on 4 x 4,
    # one tile and just over it
    c('direct<7,1>', FP32, 8, 1, 7, (1, 16, 64), mode=REFLECT),
    c('direct<7,4>', FP32, (6, 1), 2, 7, (2, 17, 65), stats=True),
    c('direct<7,4>', FP32, (4, 3, 1), 3, 7, (1, 4, 4), mode=REFLECT),
    c('direct<7,4>', FP32, 12, 4, 7, (1, 17, 65), mode=REFLECT, vsrc=RELU),
    c('direct<7,4>', X3, 8, 3, 7, (1, 16, 64)),
    c('direct<7,1>', X3, 8, 1, 7, (1, 17, 65), mode=REFLECT, stats=True),
    # ... the tap GEMM body: bf16x3, 64 channels, reflection, no statistics -- and each condition off
    c('tapgemm th=7', X3, 64, 1, 7, (1, 20, 40), mode=REFLECT),
    c('direct<7,1>', X3, 48, 1, 7, (1, 20, 40), mode=REFLECT),
    c('direct<7,1>', X3, 64, 1, 7, (1, 20, 40)),
    c('direct<7,1>', X3, 64, 1, 7, (1, 20, 40), mode=REFLECT, stats=True),
    c('direct<7,1>', X3, (32, 32), 1, 7, (1, 20, 40), mode=REFLECT),
    c('direct<7,1>', FP32, 64, 1, 7, (1, 20, 40), mode=REFLECT),

    # ---- igemm: the channel-chunk rule.  First shrink loop: 12 = 8 + 4 -> 4, 10 -> 4 -> 2; second (the LDS target): a 7x7 with 64
    # outputs cannot keep 8-channel chunks; a 1-channel segment forces 2
    c('igemm ConvCfg<4,1,3,1,1,4,2> taps=9', FP32, (16, 12), 32, 3, (1, 9, 33)),
    c('igemm ConvCfg<2,1,3,1,1,4,2> taps=9', FP32, 10, 32, 3, (1, 9, 33), mode=REFLECT),
    c('igemm ConvCfg<2,1,7,1,2,4,2> taps=49', FP32, (8, 8, 8), 64, 7, (1, 9, 33), mode=REFLECT, stats=True),
    c('igemm ConvCfg<2,1,7,2,2,2,2> taps=49', FP32, (8, 8, 8), 128, 7, (1, 9, 33)),
    # ... and 8 -> 4 by the same rule: two 8-channel chunks need two LDS stages, two 4-channel stages fit
    c('igemm ConvCfg<4,1,7,1,1,4,2> taps=49', FP32, (8, 8), 33, 7, (1, 9, 33), mode=REFLECT),
    c('igemm ConvCfg<4,2,4,1,2,4,2> taps=16', FP32, (8, 8), 48, 4, (1, 9, 33), stride=2, pad=1, stats=True),
    c('igemm ConvCfg<4,1,4,2,2,2,2> taps=16', FP32, (8, 8), 96, 4, (2, 7, 11), pad=1),
    c('igemm ConvCfg<2,1,3,1,1,4,2> taps=9', FP32, (24, 1), 33, 3, (1, 9, 33), vsrc=LRELU),
    # ... the cout tile steps 31 | 32 | 33, 47 | 48, 95 | 96 and two tiles
    c('igemm ConvCfg<8,1,3,1,1,4,2> taps=9', FP32, 24, 31, 3, (2, 7, 11), mode=REFLECT),
    c('igemm ConvCfg<8,1,3,1,1,4,2> taps=9', FP32, 24, 32, 3, (2, 7, 11), stats=True),
    c('igemm ConvCfg<8,1,3,1,1,4,2> taps=9', FP32, 24, 33, 3, (2, 7, 11)),
    c('igemm ConvCfg<8,1,3,1,1,4,2> taps=9', FP32, 24, 47, 3, (2, 7, 11), stats=True),
    c('igemm ConvCfg<8,1,3,1,2,4,2> taps=9', FP32, 24, 48, 3, (2, 7, 11)),
    c('igemm ConvCfg<8,1,3,1,2,4,2> taps=9', FP32, 24, 95, 3, (2, 7, 11)),
    c('igemm ConvCfg<4,1,3,2,2,2,2> taps=9', FP32, 24, 96, 3, (2, 7, 11), stats=True),
    c('igemm ConvCfg<4,1,3,2,2,2,2> taps=9', FP32, 24, 129, 3, (2, 7, 11), mode=REFLECT, stats=True),
    # ... the data-gradient form (IOHW, flipped), and a segment off the 16-channel grid in bf16x3 (stays on fp32)
    c('igemm ConvCfg<8,1,3,1,1,4,2> taps=9', FP32, 24, 8, 3, (1, 9, 33), pad=2, layout=IOHW, flip=True),
    c('igemm ConvCfg<8,1,3,1,2,4,2> taps=9', X3, (24, 8), 64, 3, (1, 9, 33), mode=REFLECT, stats=True),
    c('igemm ConvCfg<8,1,3,1,2,4,2> taps=9', B16, (24, 8), 64, 3, (1, 9, 33), mode=REFLECT, stats=True),
    # ... transposed: K 3 | 4, pad 0 | 1, output_padding 0 | 1, a 1 x 1 input
    c('igemm ConvCfg<8,1,0,1,1,4,2> taps=1; igemm ConvCfg<8,1,0,1,1,4,2> taps=2; igemm ConvCfg<8,1,0,1,1,4,2> taps=2; igemm ConvCfg<8,1,0,1,1,4,2> taps=4', FP32, 8, 8, 3, (1, 1, 1), pad=1, op=1, **T2),
    c('igemm ConvCfg<8,1,0,1,1,4,2> taps=4; igemm ConvCfg<8,1,0,1,1,4,2> taps=2; igemm ConvCfg<8,1,0,1,1,4,2> taps=2; igemm ConvCfg<8,1,0,1,1,4,2> taps=1', FP32, 8, 40, 3, (2, 5, 7), pad=0, op=0, stats=True, **T2),
    c('igemm ConvCfg<8,1,0,1,1,4,2> taps=1; igemm ConvCfg<8,1,0,1,1,4,2> taps=2; igemm ConvCfg<8,1,0,1,1,4,2> taps=2; igemm ConvCfg<8,1,0,1,1,4,2> taps=4', FP32, 8, 40, 3, (2, 5, 7), pad=1, op=0, **T2),
    c('igemm ConvCfg<4,1,0,1,1,4,2> taps=4; igemm ConvCfg<4,1,0,1,1,4,2> taps=4; igemm ConvCfg<4,1,0,1,1,4,2> taps=4; igemm ConvCfg<4,1,0,1,1,4,2> taps=4', FP32, (4, 4), 8, 4, (1, 1, 1), pad=0, op=1, **T2),
    c('igemm ConvCfg<4,1,0,1,2,4,2> taps=4; igemm ConvCfg<4,1,0,1,2,4,2> taps=4; igemm ConvCfg<4,1,0,1,2,4,2> taps=4; igemm ConvCfg<4,1,0,1,2,4,2> taps=4', FP32, 12, 64, 4, (1, 5, 7), pad=1, op=1, stats=True, **T2),
    c('igemm ConvCfg<8,1,0,1,1,4,2> taps=4; igemm ConvCfg<8,1,0,1,1,4,2> taps=4; igemm ConvCfg<8,1,0,1,1,4,2> taps=4; igemm ConvCfg<8,1,0,1,1,4,2> taps=4', FP32, 8, 8, 4, (1, 5, 7), pad=1, op=0, layout=OIHW, flip=True, **T2),
]

# ... every ConvCfg of the registry a descriptor reaches: K = 1, 3, 4, 7 at stride 1 and K = 3, 4 at stride 2 (odd inputs), by channel
# chunk (one segment of 1, 3 and 5 channels) and cout tile (C: 33, B: 48, A: 96 outputs); statistics, reflection and a virtual source
# take turns.  Four entries are UNREACHABLE (tests/test_conv_edges_cpu.py): the LDS target halves the chunk of their layers, which
# run here on the entry they land on: one 5- or 3-channel segment is two chunks of 4 or 2 channels and two LDS stages, so 2 it is.
IGEMM_TILES = {'C': ('1,1,4,2', 33), 'B': ('1,2,4,2', 48), 'A': ('2,2,2,2', 96)}
IGEMM_LANDS = {'ConvCfg<4,1,7,2,2,2,2>': 'ConvCfg<2,1,7,2,2,2,2>', 'ConvCfg<8,1,7,2,2,2,2>': 'ConvCfg<2,1,7,2,2,2,2>',
               'ConvCfg<8,1,7,1,2,4,2>': 'ConvCfg<2,1,7,1,2,4,2>', 'ConvCfg<8,2,4,2,2,2,2>': 'ConvCfg<2,2,4,2,2,2,2>'}
IGEMM_UNREACHABLE = set(IGEMM_LANDS)
for _k, _s in ((1, 1), (3, 1), (4, 1), (7, 1), (3, 2), (4, 2)):
    for _ci, _segs in ((2, (1,)), (4, (3,)), (8, (5,))):
        for _t in 'CBA':
            _cfg = 'ConvCfg<%d,%d,%d,%s>' % (_ci, _s, 0 if _k == 1 else _k, IGEMM_TILES[_t][0])
            _cfg = IGEMM_LANDS.get(_cfg, _cfg)
            _i = len(CASES)
            CASES.append(c('igemm %s taps=%d' % (_cfg, _k * _k), FP32, _segs, IGEMM_TILES[_t][1], _k, (1, 9, 35) if _i % 2 else (2, 7, 11),
                           stride=_s, pad=0 if _k == 1 else (_k - 1) // 2, mode=REFLECT if _k > 1 and _i % 2 else ZERO,
                           stats=_i % 3 == 0, vsrc=RELU if _i % 4 == 1 else None))

for _p in (X3, B16):
    _a = 'x3' if _p == X3 else 'b16'
    _v = dict(vsrc=LRELU) if _p == X3 else {}        # (plain bf16: plain sources, the reference rounds the operands)
    CASES += [
        # ---- split-bf16 matrix path, in both arithmetic modes.  3x3 stride 1: the tall tile needs more than 128 tiles of 16 rows
        # (3 x 3 x 3 x 5 = 135 | 2 x 3 x 2 x 5 = 60), and a map no taller than the short tile takes the short one whatever the count
        c('bf3 Bf3Cfg<1,3,1,2,4,4> taps=9 {a} wg=135'.format(a=_a), _p, 32, 320, 3, (3, 33, 65), mode=REFLECT, stats=True),
        c('bf3 Bf3Cfg<1,3,1,2,4,1> taps=9 {a} wg=180'.format(a=_a), _p, 32, 320, 3, (2, 33, 64), mode=REFLECT),
        c('bf3 Bf3Cfg<1,3,1,2,4,1> taps=9 {a} wg=135'.format(a=_a), _p, 32, 320, 3, (3, 4, 288)),
        # ... the odd chunk count (a zero chunk), three segments, the eligibility edges: Cout 47 | 48, Cout 15 | 16 at Cin 128, Cin 16 | 32
        c('bf3 Bf3Cfg<1,3,1,2,4,1> taps=9 {a} wg=6'.format(a=_a), _p, (16, 16, 16), 48, 3, (1, 9, 33), mode=REFLECT, stats=True, **_v),
        c('igemm ConvCfg<8,1,3,1,1,4,2> taps=9'.format(a=_a), _p, 32, 47, 3, (1, 9, 33)),
        c('bf3 Bf3Cfg<1,3,1,2,4,1> taps=9 {a} wg=6'.format(a=_a), _p, 32, 48, 3, (1, 9, 33)),
        c('igemm ConvCfg<8,1,3,1,1,4,2> taps=9'.format(a=_a), _p, 128, 15, 3, (1, 9, 33)),
        c('bf3 Bf3Cfg<1,3,1,2,4,1> taps=9 {a} wg=6'.format(a=_a), _p, 128, 16, 3, (1, 9, 33), stats=True),
        c('igemm ConvCfg<8,1,3,1,2,4,2> taps=9'.format(a=_a), _p, 16, 64, 3, (1, 9, 33)),
        c('bf3 Bf3Cfg<1,3,1,2,4,1> taps=9 {a} wg=6'.format(a=_a), _p, 32, 64, 3, (1, 9, 33), **_v),
        # ... 4x4 stride 1, 3x3 stride 2 on odd inputs, 1x1, the row form of a stem
        c('bf3 Bf3Cfg<1,4,1,1,4,4> taps=16 {a} wg=4'.format(a=_a), _p, 32, 48, 4, (2, 9, 33), pad=1, stats=True),
        c('bf3 Bf3Cfg<2,3,2,1,2,2> taps=9 {a} wg=6'.format(a=_a), _p, 32, 48, 3, (3, 9, 33), stride=2, stats=True, **_v),
        c('bf3 Bf3Cfg<1,0,1,2,4,4,1> taps=1 {a} wg=6'.format(a=_a), _p, 48, 48, 1, (3, 9, 33), pad=0, stats=True),
        c('bf3 Bf3Cfg<1,7,1,1,4,2,0,1> taps=7 {a} wg=4'.format(a=_a), _p, 3, 32, 7, (1, 9, 33), mode=REFLECT, kind='rows', stats=True),
        c('bf3 Bf3Cfg<1,7,1,1,4,2,0,1> taps=7 {a} wg=4'.format(a=_a), _p, 4, 64, 7, (1, 8, 40), kind='rows'),
        # ... 2x2 space-to-depth: a 4x4 layer; 3x3 layers with compile-time tap sets (Cin 32: two chunks per input phase), run-time
        # masks (Cin 48: three) and neither (Cin 40: 160 channels, no whole chunks per phase)
        c('bf3 Bf3Cfg<1,0,1,2,4,2,4> taps=4 {a} wg=3'.format(a=_a), _p, 32, 48, 4, (3, 10, 34), stride=2, pad=1, kind='s2d', stats=True),
        c('bf3 Bf3Cfg<1,0,1,2,4,2,4> taps=4 {a} s2d3=ct wg=3'.format(a=_a), _p, 32, 48, 3, (3, 10, 34), stride=2, kind='s2d', stats=True),
        c('bf3 Bf3Cfg<1,0,1,2,4,2,4> taps=4 {a} s2d3=mask wg=3'.format(a=_a), _p, 48, 48, 3, (3, 10, 34), stride=2, kind='s2d'),
        c('bf3 Bf3Cfg<1,0,1,2,4,2,4> taps=4 {a} wg=3'.format(a=_a), _p, 40, 48, 3, (3, 10, 34), stride=2, kind='s2d'),
        # ... transposed: all phases in one tile (ph4 = 3 | 4), fused phases at pad 0, four launches at an odd output (K = 3:
        # 1 | 2 | 2 | 4 taps on the full-height tile; K = 4: four 4-tap launches on the half-height one); a 1 x 1 input
        c('bf3 Ph4Cfg<3> taps=4 {a} phases=ph4 wg=6'.format(a=_a), _p, 32, 48, 3, (3, 5, 17), pad=1, op=1, stats=True, **T2),
        c('bf3 Ph4Cfg<4> taps=4 {a} phases=ph4 wg=6'.format(a=_a), _p, 32, 48, 4, (3, 5, 17), pad=1, op=0, stats=True, **T2),
        c('bf3 Bf3Cfg<1,0,1,2,4,2,4> taps=4 {a} phases=fused wg=4'.format(a=_a), _p, 32, 48, 3, (1, 5, 17), pad=0, op=1, stats=True, **T2),
        c('bf3 Bf3Cfg<1,0,1,2,4,2,4> taps=4 {a} phases=fused wg=4'.format(a=_a), _p, 32, 48, 4, (1, 5, 17), pad=0, op=0, **T2),
        c('bf3 Bf3Cfg<1,0,1,2,4,4,1> taps=1 {a} phases=4launch wg=3; bf3 Bf3Cfg<1,0,1,2,4,4,2> taps=2 {a} phases=4launch wg=3; bf3 Bf3Cfg<1,0,1,2,4,4,2> taps=2 {a} phases=4launch wg=3; bf3 Bf3Cfg<1,0,1,2,4,4,4> taps=4 {a} phases=4launch wg=3'.format(a=_a), _p, 32, 48, 3, (3, 5, 17), pad=1, op=0, stats=True, **T2),
        c('bf3 Bf3Cfg<1,0,1,2,4,4,1> taps=1 {a} wg=3'.format(a=_a), _p, 32, 48, 3, (3, 1, 1), pad=1, op=0, **T2),
        c('; '.join(['bf3 Bf3Cfg<1,0,1,2,4,2,4> taps=4 {a} phases=4launch wg=3'] * 4).format(a=_a), _p, 32, 48, 4, (3, 5, 17), pad=1, op=1, stats=True, **T2),
    ]
CASES += [
    # ... more tiles than persistent workgroups by default (270 tiles of 4 rows on 256 single-workgroup CUs)
    c('bf3 Bf3Cfg<1,3,1,2,4,1> taps=9 x3 wg=256', X3, 32, 320, 3, (3, 33, 64), mode=REFLECT, stats=True),
    # ... the output forms where the plan takes them (ap_conv2d_octet_ok, ap_conv2d_bf16out_ok), and their refusal where it does not
    c('bf3 Bf3Cfg<1,3,1,2,4,1> taps=9 x3 wg=6', X3, 32, 48, 3, (1, 9, 33), mode=REFLECT, form=OCTET, stats=True),
    c('bf3 Bf3Cfg<1,0,1,2,4,4,1> taps=1 x3 wg=6', X3, 48, 48, 1, (3, 9, 33), pad=0, form=OCTET),
    c('bf3 Bf3Cfg<1,7,1,1,4,2,0,1> taps=7 b16 wg=4', B16, 3, 32, 7, (1, 9, 33), mode=REFLECT, kind='rows', form=OCTET, stats=True),
    c(-2, B16, 32, 48, 3, (1, 9, 33), form=OCTET, refused=-2),
    c(-2, X3, 32, 44, 3, (1, 9, 33), form=OCTET, refused=-2),
    c('bf3 Bf3Cfg<1,3,1,2,4,1> taps=9 b16 ob16 wg=6', B16, 32, 48, 3, (1, 9, 33), mode=REFLECT, form=OB16, stats=True),
    c('bf3 Bf3Cfg<1,3,1,2,4,4> taps=9 b16 ob16 wg=135', B16, 32, 320, 3, (3, 33, 65), form=OB16),
    c(-2, X3, 32, 48, 3, (1, 9, 33), form=OB16, refused=-2),
    c(-2, B16, 32, 48, 4, (1, 9, 33), pad=1, form=OB16, refused=-2),
]


def spec_of(case):
    """(the ConvSpec the case launches, the original layer's ConvSpec)"""
    from animateportrait_amd import ops
    orig = ops.ConvSpec(case.segs, case.cout, case.k, case.stride, case.pad, case.mode, case.tr, case.op, case.layout, case.flip)
    orig.precision = case.prec
    if case.kind == 'rows':
        assert ops.stem_rows_eligible(orig), case.name
        return ops.stem_rows_spec(orig), orig
    if case.kind == 's2d':
        # (ops.s2d_eligible is the product's rule; the form itself asks for this much)
        n, h, w = case.shape
        assert (case.stride, case.pad, case.mode, case.tr, len(case.segs), h % 2, w % 2) == (2, 1, ZERO, False, 1, 0, 0) and case.k in (3, 4)
        return ops.s2d_spec(orig), orig
    return orig, orig


def launch_dims(case):
    """N, H, W of the launched descriptor (the space-to-depth copy is (H/2 + 1) x (W/2 + 1))"""
    n, h, w = case.shape
    return (n, h // 2 + 1, w // 2 + 1) if case.kind == 's2d' else (n, h, w)


def query(case):
    """ops.conv_fwd_route's answer for a case under the current environment, or the refusal code"""
    from animateportrait_amd import ops, _capi
    spec, _ = spec_of(case)
    d = spec.desc(*launch_dims(case))
    lib = _capi.lib()
    if case.prec != FP32 and lib.ap_conv2d_wants_presplit(ctypes.byref(d)) == 1:
        d.presplit = 1
    buf = ctypes.create_string_buffer(512)
    rc = lib.ap_conv2d_fwd_route(ctypes.byref(d), int(case.stats), case.form, buf, len(buf))
    return buf.value.decode() if rc == 0 else rc


def family(route):
    return route.split()[0].split('<', 1)[0]


def workgroups(route):
    return [int(w[3:]) for w in route.replace(';', ' ').split() if w.startswith('wg=')]


# ------------------------------------------------------------------------------------------------ the GPU side
@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


def _act64(t, act):
    return t if act == NONE else (F.relu(t) if act == RELU else F.leaky_relu(t, 0.2))


def _r16(t):
    return t.float().bfloat16().double()


def _nan(n, dev, dtype=torch.float32):
    return torch.full((n,), float('nan'), dtype=dtype, device=dev)


def _tail_is_nan(buf, n, what):
    tail = buf[n:].cpu()
    bits = torch.int16 if buf.dtype == torch.bfloat16 else torch.int32
    assert torch.equal(tail.view(bits), torch.full_like(tail, float('nan')).view(bits)), what + ': wrote past its buffer'


def _ref64(case, x, w, b):
    """the layer before its epilogue activation, in fp64"""
    if case.tr:
        w = w if case.layout == IOHW else w.permute(1, 0, 2, 3)
        w = w.flip(2, 3) if case.flip else w
        return F.conv_transpose2d(x, w, b, stride=2, padding=case.pad, output_padding=case.op)
    w = w if case.layout == OIHW else w.permute(1, 0, 2, 3)
    w = w.flip(2, 3) if case.flip else w
    xp = F.pad(x, (case.pad,) * 4, mode='reflect') if case.mode == REFLECT and case.pad else F.pad(x, (case.pad,) * 4)
    return F.conv2d(xp, w, b, stride=case.stride)


class Problem:
    """The tensors of one case on the device, its fp64 reference, and the direct call of the entry point."""

    def __init__(self, case, dev):
        from animateportrait_amd import ops, _capi
        from test_wgrad_edges_gpu import _virtual
        self.case, self.dev, lib = case, dev, _capi.lib()
        n, h, w = case.shape
        gen = torch.Generator().manual_seed(sum(map(ord, case.name)))
        xs64, feats = [], []
        for i, ch in enumerate(case.segs):
            raw = torch.randn(n, ch, h, w, generator=gen) * 1.5 + 0.3
            if case.vsrc is not None and i == 0:
                f, val = _virtual(raw, case.vsrc, dev)
            else:
                f, val = ops.Feat(raw.to(dev)), raw.double()
            xs64.append(val)
            feats.append(f)
        x64 = torch.cat(xs64, 1)
        cin = x64.shape[1]
        wshape = (cin, case.cout, case.k, case.k) if case.layout == IOHW else (case.cout, cin, case.k, case.k)
        wt = torch.randn(wshape, generator=gen) * 0.05 + 0.01
        bias = torch.randn(case.cout, generator=gen) + torch.arange(case.cout) * 0.125
        self.spec, orig = spec_of(case)
        wdev = wt.to(dev)
        if case.kind == 'rows':
            feats, wdev = [ops.presplit_rows(feats[0], case.k, case.pad, case.mode)], ops.stem_rows_weight(wdev).contiguous()
        elif case.kind == 's2d':
            feats, wdev = [ops.presplit_s2d(feats[0])], ops.s2d_weight(wdev)
        self.feats, self.bias = feats, bias.to(dev)
        ln, lh, lw = launch_dims(case)
        assert tuple(feats[0].data.shape[2:]) == (lh, lw)
        self.d = d = self.spec.desc(ln, lh, lw, None, case.act)
        self.bf3 = case.prec != FP32 and _capi.check(lib.ap_conv2d_wants_presplit(ctypes.byref(d)), 'wants_presplit') == 1
        if self.bf3:
            self.spec.presplit_desc(ln, lh, lw, feats, d=d)
        else:
            self.spec.fill_sources(d, feats)
        plain16 = case.prec == B16 and self.bf3
        if plain16:
            assert case.vsrc is None
            self.pre = _ref64(case, _r16(x64), _r16(wt.double()), bias.double())
        else:
            self.pre = _ref64(case, x64, wt.double(), bias.double())
        self.ref = _act64(self.pre, case.act)
        self.scale = float(self.pre.abs().max())
        assert self.scale > 0
        # (the tap GEMM multiplies split-bf16 parts of fp32 sources: the split-bf16 bar, as tests/test_final_layer_gpu.py holds it to)
        split = self.bf3 or (not case.refused and family(case.route) == 'tapgemm')
        self.tol = (2e-5 if plain16 else 5e-5) if split else 2e-6
        self.norm_tol = 2e-3 if split else 1e-4
        ho, wo = ctypes.c_int32(), ctypes.c_int32()
        _capi.check(lib.ap_conv2d_out_size(ctypes.byref(d), ctypes.byref(ho), ctypes.byref(wo)), 'out_size')
        self.oshape = (n, case.cout, ho.value, wo.value)
        assert tuple(self.ref.shape) == self.oshape, (tuple(self.ref.shape), self.oshape)
        # the packed image: exactly packed_floats long, NaN behind it
        self.npacked = _capi.check(lib.ap_conv2d_packed_floats(ctypes.byref(d)), 'packed_floats')
        self.packed = _nan(self.npacked + TAIL_FLOATS, dev)
        _capi.check(lib.ap_conv2d_pack_weights(ctypes.byref(d), ops._ptr(wdev), ops._ptr(self.packed), ops._stream()), 'pack_weights')
        torch.cuda.synchronize()
        _tail_is_nan(self.packed, self.npacked, 'the weight packer')
        self.tiles = _capi.check(lib.ap_conv2d_stat_tiles(ctypes.byref(d)), 'stat_tiles') if case.stats else 0

    def call(self, what):
        """One call of the entry point into NaN buffers with NaN tails; returns (y as NCHW fp32 on the CPU, raw y buffer, partials)"""
        from animateportrait_amd import ops, _capi
        case, lib, dev = self.case, _capi.lib(), self.dev
        n, cout, ho, wo = self.oshape
        ny = n * cout * ho * wo
        y = _nan(ny + TAIL_FLOATS, dev, torch.bfloat16 if case.form == OB16 else torch.float32)
        nst = n * cout * self.tiles * 2
        st = _nan(nst + TAIL_FLOATS, dev) if case.stats else None
        fwd = (lib.ap_conv2d_fwd, lib.ap_conv2d_fwd_octet, lib.ap_conv2d_fwd_bf16out)[case.form]
        rc = fwd(ctypes.byref(self.d), ops._ptr(self.packed), ops._ptr(self.bias), ops._ptr(y), ops._ptr(st), ops._stream())
        _capi.check(rc, what)
        torch.cuda.synchronize()
        _tail_is_nan(y, ny, what + ': y')
        _tail_is_nan(self.packed, self.npacked, what + ': packed image')
        assert bool(torch.isfinite(y[:ny].float()).all()), what + ': y holds a value that is not finite (unwritten, or read past an operand)'
        if st is not None:
            _tail_is_nan(st, nst, what + ': statistics')
            assert bool(torch.isfinite(st[:nst]).all()), what + ': a statistics tile slot no workgroup wrote'
        out = y[:ny].float()
        out = out.view(n, cout // 8, ho * wo, 8).permute(0, 1, 3, 2).reshape(self.oshape) if case.form == OCTET else out.view(self.oshape)
        return out, y, st

    def check(self, out, what):
        out = out.cpu().double()
        if self.case.form == OB16:
            # the store rounds to nearest, which is monotonic: a value within the bar of ref lands between the rounded ends of the bar
            lo, hi = _r16(self.ref - self.tol * self.scale), _r16(self.ref + self.tol * self.scale)
            err = torch.maximum(lo - out, out - hi).clamp(min=0)
            e = float(err.max()) / self.scale
            print('%-72s %-22s outside the rounded bar by %.3g' % (self.case.name, what, e))
            assert e == 0, (what, e)
            return
        e = float((out - self.ref).abs().max()) / self.scale
        print('%-72s %-22s err %.3g of bar %.0e' % (self.case.name, what, e, self.tol))
        assert e < self.tol, (what, e, self.tol)

    def check_stats(self, y, st, what):
        """finalise through the product path and compare the normalised output"""
        from animateportrait_amd import ops
        n, cout, ho, wo = self.oshape
        ny, nst = n * cout * ho * wo, n * cout * self.tiles * 2
        f = ops.Feat(ops._stand_in(self.oshape, self.dev) if self.case.form == OCTET else y[:ny].view(self.oshape),
                     pending=(st[:nst].view(n * cout, self.tiles, 2), self.tiles))
        want = F.instance_norm(self.pre)
        if self.case.form == OB16:
            # a bf16 raw output is finalised inside its first consumer, the norm / split pass; the store's rounding, 2^-8 |y|, is
            # scaled by the plane's rstd like the values
            got = ops._norm_apply_split(f, None, want_y=True, want_xs=False)[0].cpu().double()
            rstd64 = (self.pre.var((2, 3), unbiased=False, keepdim=True) + 1e-5).rsqrt()
            err = ((got - want).abs() - self.pre.abs() * rstd64 * 2.0 ** -8).clamp(min=0)
        else:
            if self.case.form == OCTET:
                f.oct = y[:ny].view(n, cout // 8, ho * wo, 8)
            mean, rstd = f.mean.view(n, cout, 1, 1).cpu().double(), f.rstd.view(n, cout, 1, 1).cpu().double()
            out = y[:ny].float()
            out = out.view(n, cout // 8, ho * wo, 8).permute(0, 1, 3, 2).reshape(self.oshape) if self.case.form == OCTET else out.view(self.oshape)
            err = ((out.cpu().double() - mean) * rstd - want).abs()
        e = float(err.max())
        print('%-72s %-22s normalised err %.3g of bar %.0e' % (self.case.name, what, e, self.norm_tol))
        assert e < self.norm_tol, (what, e, self.norm_tol)


def a_ragged_count(tiles):
    """the smallest workgroup count below the tile count that does not divide it (None: there is none)"""
    for blocks in range(2, tiles):
        if tiles % blocks:
            return blocks
    return None


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES, ids=[k.name for k in CASES])
def test_conv_edge(dev, monkeypatch, case):
    from animateportrait_amd import _capi, ops
    for v in ops.plan_switch_names():
        monkeypatch.delenv(v, raising=False)
    # 1 route
    assert query(case) == (case.refused if case.refused else case.route)
    prob = Problem(case, dev)
    if case.refused:
        # the entry point refuses what the query refuses, with the same code, before anything is written
        from animateportrait_amd import ops
        lib = _capi.lib()
        n, cout, ho, wo = prob.oshape
        y = _nan(n * cout * ho * wo, dev, torch.bfloat16 if case.form == OB16 else torch.float32)
        fwd = (lib.ap_conv2d_fwd, lib.ap_conv2d_fwd_octet, lib.ap_conv2d_fwd_bf16out)[case.form]
        assert fwd(ctypes.byref(prob.d), ops._ptr(prob.packed), ops._ptr(prob.bias), ops._ptr(y), None, ops._stream()) == case.refused
        torch.cuda.synchronize()
        assert bool(torch.isnan(y.float()).all())
        return
    # 2 value, 3 poison, 4 statistics, 6 bits
    out, y, st = prob.call('default launch')
    prob.check(out, 'default launch')
    if case.stats:
        prob.check_stats(y, st, 'default launch')
    _, y2, st2 = prob.call('second call')
    assert torch.equal(_bits(y), _bits(y2)), 'two calls with identical inputs differ'
    assert st is None or torch.equal(_bits(st), _bits(st2)), 'two calls with identical inputs differ in their statistics'
    # 5 the persistent walk
    if family(case.route) != 'bf3':
        assert not prob.bf3
        return
    assert prob.bf3
    monkeypatch.setenv('APAMD_BF3_BLOCKS', '1000000')
    tiles = workgroups(query(case))                      # (the cap: one workgroup per tile)
    ragged = a_ragged_count(tiles[0])
    assert min(tiles) >= 3 and ragged is not None and all(t % ragged for t in tiles), 'a split-bf16 case needs a ragged walk: %s' % tiles
    for blocks in (1, ragged):
        monkeypatch.setenv('APAMD_BF3_BLOCKS', str(blocks))
        assert workgroups(query(case)) == [min(blocks, t) for t in tiles]
        what = '%d workgroups over %d tiles' % (blocks, tiles[0])
        _, yw, stw = prob.call(what)
        assert torch.equal(_bits(y), _bits(yw)), what + ': differs from the default launch'
        assert st is None or torch.equal(_bits(st), _bits(stw)), what + ': statistics differ from the default launch'
