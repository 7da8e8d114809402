"""GPU (-m gpu): every weight-gradient family at the edges of its planner (csrc/wgrad_plan.hip: make_wgrad_plan), against fp64.

tests/test_wgrad_plan_cpu.py pins what the planner ANSWERS on both sides of every branch; this module RUNS the kernels there.
Each case of CASES is one small layer and states the route it is meant to exercise, in the words of ap_conv2d_wgrad_route
(ops.wgrad_kernel_route): kernel table entry, operand forms, P and nstages.  A planner change that moves a case off its kernel
fails the first assertion instead of silently testing something else; tests/test_wgrad_edges_cpu.py checks without a GPU that the
cases together name every kernel table entry and operand form, and that every stated route is the planner's answer.

Per case (test_wgrad_edge):
  1 route     the stated string is the query's answer;
  2 value     dw against the autograd gradient of an fp64 F.conv2d on the CPU with respect to a zero weight.  Gaussian operands with
              a non-zero mean.  Bars, the ones the project already holds these families to: 5e-6 max|ref| for the exact-fp32 kernels
              (igemm, narrow, final), 5e-5 for split bf16, and for plain bf16 3e-5 max|ref16| against the fp64 sum of the bf16-ROUNDED
              operands (plain sources there: act(IN(.)) evaluated on the device may round to the neighbouring bf16);
  3 poison    the C entry point is called directly with a workspace of workspace_floats + 4096 floats, all NaN, and a NaN dw: the
              tail must come back bit-for-bit NaN and dw must hold no NaN -- a GEMM that reads an operand slot the preparation pass
              did not write shows up here and not in a fresh (zero) allocation;
  4 stages    the same under APAMD_WGRAD_BLOCKS = 1, a value whose P does not divide nstages (where one exists: P and nstages are
              read off the route string), and 100000 (the cap: nstages / 2 for the bf16 GEMM, nstages for igemm); each against fp64.
              The narrow family splits image rows, not stages, and does not read the knob: its route must not move;
  5 bits      two calls with identical inputs give identical bits (fixed reduction order, no atomics).

The few-output and final routes of ops.wgrad have no plan of this kind: their cases state ops.wgrad_route's answer (and, for
few_outputs, the route of the role-swapped inner call), run ops.wgrad for the value, and poison the workspace of the entry point
underneath.  (few_outputs needs 2 pad = k - 1, which no 4x4 layer meets: the K = 4 case of the issue's list states what runs instead.)

The k7 / d0 bf16 edge kernels and the PatchGAN head are covered by test_served_shapes_gpu.py and are not repeated here."""
import collections
import ctypes
import re

import pytest
import torch
import torch.nn.functional as F

from conftest import linf

FP32, X3, B16 = 0, 1, 2
ZERO, REFLECT = 0, 1
NONE, RELU, LRELU = 0, 1, 2
TAIL_FLOATS = 4096

# via: 'wgrad' ap_conv2d_wgrad | 'pre' ap_conv2d_wgrad_pre (g_t from instnorm_bwd_split) | 'xs' ap_conv2d_wgrad_xs (g as a split copy)
#      | 'final' | 'few' (routes of ops.wgrad);  xs: which forward copies the source carries: '' | 'plain' | 's2d'
#      g: activation of a virtual gradient act(IN(raw)), or None: plain;  vsrc: the first source is act(IN(.)) with ReLU
Case = collections.namedtuple('Case', 'name prec segs m k stride pad mode shape g vsrc env via xs route')


def c(route, prec, segs, m, k, shape, stride=1, pad=None, mode=ZERO, g=None, vsrc=False, env=None, via='wgrad', xs=''):
    segs = (segs,) if isinstance(segs, int) else tuple(segs)
    pad = (k - 1) // 2 if pad is None else pad
    name = '%s %s->%d k%d s%d p%d%s %s' % (('fp32', 'bf16x3', 'bf16')[prec], '+'.join(map(str, segs)), m, k, stride, pad,
                                           'r' if mode == REFLECT else 'z', 'x'.join(map(str, shape)))
    name += ''.join([' g=act%d' % g if g is not None else '', ' vsrc' if vsrc else '', ' ' + via if via != 'wgrad' else '',
                     ' xs=' + xs if xs else ''] + [' %s=%s' % (k_[6:], v) for k_, v in sorted((env or {}).items())])
    return Case(name, prec, segs, m, k, stride, pad, mode, tuple(shape), g, vsrc, dict(env or {}), via, xs, route)


A, B = (2, 32, 32), (1, 33, 47)
ROWS = {'APAMD_ROWS_WGRAD': '1'}
CASES = [
    # ---- bf16 GEMM, stride 1.  M 47 | 48 (the matrix pipe's floor) and 127 | 128 | 256 (the 8-wave workgroup), Cin = 64, reflect
    c('igemm<1,3,128,256,2> g=direct a=pad P=32 nstages=32', X3, 64, 47, 3, A, mode=REFLECT),
    c('bf16gemm<3,split> g=vec a=pad_rows P=16 nstages=32', X3, 64, 48, 3, A, mode=REFLECT),
    c('igemm<1,3,128,256,2> g=pad a=pad P=34 nstages=34', X3, 64, 47, 3, B, mode=REFLECT),
    c('bf16gemm<3,split> g=general a=general P=17 nstages=34', X3, 64, 48, 3, B, mode=REFLECT),
    c('igemm<1,3,128,256,2> g=direct a=pad P=32 nstages=32', B16, 64, 47, 3, A, mode=REFLECT),
    c('bf16gemm<3,heads> g=vec a=pad_rows P=16 nstages=32', B16, 64, 48, 3, A, mode=REFLECT),
    c('igemm<1,3,128,256,2> g=pad a=pad P=34 nstages=34', B16, 64, 47, 3, B, mode=REFLECT),
    c('bf16gemm<3,heads> g=general a=general P=17 nstages=34', B16, 64, 48, 3, B, mode=REFLECT),
    c('bf16gemm<3,split> g=vec a=pad_rows P=16 nstages=32', X3, 64, 127, 3, A, mode=REFLECT),
    c('bf16gemm<3,wide> g=vec a=pad_rows P=16 nstages=32', X3, 64, 128, 3, A, mode=REFLECT),
    c('bf16gemm<3,split> g=general a=general P=17 nstages=34', X3, 64, 127, 3, B, mode=REFLECT),
    c('bf16gemm<3,wide> g=general a=general P=17 nstages=34', X3, 64, 128, 3, B, mode=REFLECT),
    c('bf16gemm<3,heads> g=vec a=pad_rows P=16 nstages=32', B16, 64, 127, 3, A, mode=REFLECT),
    c('bf16gemm<3,heads> g=vec a=pad_rows P=16 nstages=32', B16, 64, 128, 3, A, mode=REFLECT),
    c('bf16gemm<3,heads> g=general a=general P=17 nstages=34', B16, 64, 127, 3, B, mode=REFLECT),
    c('bf16gemm<3,heads> g=general a=general P=17 nstages=34', B16, 64, 128, 3, B, mode=REFLECT),
    c('bf16gemm<3,wide> g=vec a=pad_rows P=16 nstages=32', X3, 64, 256, 3, A, mode=REFLECT),
    c('bf16gemm<3,wide> g=general a=general P=17 nstages=34', X3, 64, 256, 3, B, mode=REFLECT),
    # ... Cin 31 | 32
    c('igemm<1,3,128,256,2> g=direct a=pad P=32 nstages=32', X3, 31, 64, 3, A, mode=REFLECT),
    c('bf16gemm<3,split> g=vec a=pad_rows P=16 nstages=32', X3, 32, 64, 3, A, mode=REFLECT),
    c('igemm<1,3,128,256,2> g=pad a=pad P=34 nstages=34', B16, 31, 64, 3, B, mode=REFLECT),
    c('bf16gemm<3,heads> g=general a=general P=17 nstages=34', B16, 32, 64, 3, B, mode=REFLECT),
    # ... segment lists: two channel tiles with a segment boundary inside the first, five tiles, and a list that stays on fp32
    c('bf16gemm<3,split> g=vec a=pad_rows P=16 nstages=32', X3, (48, 16, 32), 64, 3, A),
    c('bf16gemm<3,heads> g=general a=general P=17 nstages=34', B16, (48, 16, 32), 64, 3, B),
    c('bf16gemm<3,split> g=general a=general P=17 nstages=34', X3, (256, 16), 64, 3, B, mode=REFLECT),
    c('igemm<1,3,128,256,2> g=direct a=pad P=32 nstages=32', X3, (16, 8, 7), 64, 3, A),
    # ... 4x4: never the 8-wave workgroup; the 31 x 31 output of the PatchGAN's tail
    c('bf16gemm<4,split> g=general a=pad_rows P=16 nstages=32', X3, 64, 128, 4, A),
    c('bf16gemm<4,heads> g=general a=pad_rows P=16 nstages=32', B16, 64, 128, 4, A),
    c('bf16gemm<4,split> g=general a=general P=15 nstages=30', X3, 32, 48, 4, (2, 31, 31)),
    # ... operand forms: the padded-row kernel at every row width with 1 - 3 segments and odd row counts; the general one at W = 40, 45
    c('bf16gemm<3,split> g=vec a=pad_rows P=12 nstages=24', X3, (32,), 48, 3, (1, 5, 256), mode=REFLECT),
    c('bf16gemm<3,heads> g=vec a=pad_rows P=10 nstages=20', B16, (32, 16), 64, 3, (1, 10, 128), mode=REFLECT),
    c('bf16gemm<3,split> g=vec a=pad_rows P=20 nstages=40', X3, (40, 24, 8), 80, 3, (2, 19, 64)),
    c('bf16gemm<3,split> g=general a=general P=6 nstages=12', X3, 40, 48, 3, (1, 12, 40)),
    c('bf16gemm<3,heads> g=general a=general P=6 nstages=12', B16, 32, 64, 3, (1, 11, 45), mode=REFLECT),
    # ... one-stage and few-stage maps
    c('bf16gemm<3,split> g=vec a=pad_rows P=1 nstages=1', X3, 64, 64, 3, (1, 2, 32)),
    c('bf16gemm<3,split> g=general a=general P=1 nstages=2', X3, 64, 64, 3, (1, 4, 8)),
    c('bf16gemm<3,wide> g=vec a=pad_rows P=2 nstages=4', X3, 64, 128, 3, (1, 4, 64)),
    c('bf16gemm<3,heads> g=vec a=pad_rows P=1 nstages=1', B16, 64, 64, 3, (1, 2, 32)),
    # ... a virtual gradient and a virtual first source
    c('bf16gemm<3,split> g=vec a=pad_rows P=16 nstages=32', X3, 64, 64, 3, A, g=RELU, vsrc=True),
    c('bf16gemm<3,split> g=general a=general P=17 nstages=34', X3, (32, 16), 48, 3, B, mode=REFLECT, g=LRELU, vsrc=True),

    # ---- bf16 GEMM, stride 2 as space-to-depth (zero pad 1): Cb = 4 Cin = 32 (half a channel tile), 96 (a ragged second tile), 256, 512
    c('bf16gemm<2,split>+s2d g=general a=general P=9 nstages=18', X3, 8, 64, 3, (2, 34, 46), stride=2),
    c('bf16gemm<2,heads>+s2d g=general a=general P=9 nstages=18', B16, 8, 64, 4, (2, 34, 46), stride=2),
    c('bf16gemm<2,split>+s2d g=general a=general P=9 nstages=18', X3, 24, 64, 4, (2, 34, 46), stride=2),
    c('bf16gemm<2,heads>+s2d g=general a=general P=9 nstages=18', B16, 24, 64, 3, (2, 34, 46), stride=2),
    c('bf16gemm<2,split>+s2d g=general a=general P=9 nstages=18', X3, 64, 64, 3, (2, 34, 46), stride=2, vsrc=True),
    c('bf16gemm<2,wide>+s2d g=vec a=s2d_rows P=8 nstages=16', X3, 128, 256, 3, (2, 32, 64), stride=2),
    c('bf16gemm<2,wide>+s2d g=vec a=s2d_rows P=8 nstages=16', X3, 128, 256, 4, (2, 32, 64), stride=2),
    # ... whole source rows: the space-to-depth row kernel
    c('bf16gemm<2,split>+s2d g=vec a=s2d_rows P=1 nstages=2', X3, 32, 64, 3, (1, 8, 64), stride=2),
    c('bf16gemm<2,heads>+s2d g=vec a=s2d_rows P=1 nstages=2', B16, 64, 64, 4, (1, 4, 128), stride=2),
    c('bf16gemm<2,split>+s2d g=vec a=s2d_rows P=2 nstages=4', X3, 32, 48, 4, (1, 2, 256), stride=2),
    # ... M 47 | 48, Cin 7, and the layers the view does not exist for: odd H, reflection padding, the switch
    c('igemm<2,3,64,64,1> g=pad a=pad P=16 nstages=16', X3, 64, 47, 3, (1, 32, 48), stride=2),
    c('bf16gemm<2,split>+s2d g=general a=general P=4 nstages=8', X3, 64, 48, 3, (1, 32, 48), stride=2),
    c('igemm<2,3,64,64,1> g=pad a=pad P=16 nstages=16', X3, 7, 64, 3, (1, 32, 48), stride=2),
    c('igemm<2,3,64,64,1> g=direct a=pad P=17 nstages=17', X3, 64, 64, 3, (1, 33, 64), stride=2),
    c('igemm<2,3,64,64,1> g=direct a=pad P=32 nstages=32', X3, 64, 64, 3, (2, 32, 64), stride=2, mode=REFLECT),
    c('igemm<2,4,128,256,1> g=direct a=pad P=32 nstages=32', X3, 64, 64, 4, (2, 32, 64), stride=2, env={'APAMD_NO_S2D_WGRAD': '1'}),

    # ---- the forward pass's split copies (segments that are multiples of 8)
    c('bf16gemm<3,split> g=vec a=xs_transpose P=16 nstages=32 xs<3,2,2>', X3, (32, 16, 16), 96, 3, A, xs='plain', vsrc=True),
    c('bf16gemm<3,heads> g=general a=xs_transpose P=17 nstages=34 xs<3,1,2>', B16, (40, 24), 48, 3, B, mode=REFLECT, xs='plain'),
    c('bf16gemm<2,split>+s2d g=general a=xs_transpose P=9 nstages=18 xs<2,2,2>', X3, 24, 64, 3, (2, 34, 46), stride=2, xs='s2d', vsrc=True),
    c('bf16gemm<2,split>+s2d g=general a=xs_transpose P=9 nstages=18 xs<2,2,2>', X3, 24, 64, 4, (2, 34, 46), stride=2, xs='plain'),
    # ... both operands as split copies: the six kernels of wgrad_xs.h
    c('bf16gemm<2,split>+s2d g=none a=xs_transpose P=9 nstages=18 xs<2,2,2>', X3, 24, 72, 3, (2, 34, 46), stride=2, via='xs', xs='s2d'),
    c('bf16gemm<2,split>+s2d g=none a=xs_transpose P=9 nstages=18 xs<2,2,2>', X3, 40, 64, 4, (2, 34, 46), stride=2, via='xs', xs='plain', vsrc=True),
    c('bf16gemm<2,wide>+s2d g=none a=xs_transpose P=4 nstages=8 xs<2,2,4>', X3, 32, 128, 4, (1, 32, 64), stride=2, via='xs', xs='s2d'),
    c('bf16gemm<2,wide>+s2d g=none a=xs_transpose P=4 nstages=8 xs<2,2,4>', X3, 32, 128, 3, (1, 32, 64), stride=2, via='xs', xs='plain'),
    c('bf16gemm<3,heads> g=none a=xs_transpose P=17 nstages=34 xs<3,1,2>', B16, (40, 24), 72, 3, B, mode=REFLECT, via='xs', xs='plain'),
    c('bf16gemm<3,split> g=none a=xs_transpose P=17 nstages=34 xs<3,2,2>', X3, (32, 16, 16), 72, 3, B, via='xs', xs='plain', vsrc=True),
    c('bf16gemm<3,wide> g=none a=xs_transpose P=17 nstages=34 xs<3,2,4>', X3, (40, 24), 128, 3, B, mode=REFLECT, via='xs', xs='plain'),
    c('bf16gemm<4,split> g=none a=xs_transpose P=15 nstages=30 xs<4,2,2>', X3, 40, 56, 4, (2, 31, 31), via='xs', xs='plain'),
    # ... the gradient operand written by instnorm_bwd_split, M = 72: padded channel slots
    c('bf16gemm<3,split> g=none a=general P=24 nstages=48', X3, 64, 72, 3, (2, 24, 40), via='pre'),
    c('bf16gemm<3,heads> g=none a=pad_rows P=16 nstages=32', B16, 64, 72, 3, A, mode=REFLECT, via='pre'),

    # ---- the row form of the 7x7 stems (opt-in, plain bf16): M 24 | 23, Cin 9 | 10
    c('bf16gemm<7,heads>+rows g=vec a=general P=16 nstages=32', B16, 3, 24, 7, A, mode=REFLECT, env=ROWS),
    c('igemm<1,7,64,192,2> g=direct a=pad P=32 nstages=32', B16, 3, 23, 7, A, mode=REFLECT, env=ROWS),
    c('bf16gemm<7,heads>+rows g=general a=general P=25 nstages=51', B16, 3, 24, 7, (1, 34, 70), mode=REFLECT, env=ROWS),
    c('bf16gemm<7,heads>+rows g=general a=general P=25 nstages=51', B16, 9, 64, 7, (1, 34, 70), env=ROWS),
    c('igemm<1,7,64,192,2> g=pad a=pad P=51 nstages=51', B16, 10, 64, 7, (1, 34, 70), env=ROWS),
    c('bf16gemm<7,heads>+rows g=vec a=general P=16 nstages=32', B16, 9, 64, 7, A, mode=REFLECT, env=ROWS),

    # ---- igemm: one case per tile shape of kWgradKernels at least; g read in place (whole tiles, plain) or padded
    c('igemm<1,3,128,256,2> g=direct a=pad P=32 nstages=32', FP32, 64, 64, 3, A, mode=REFLECT),
    c('igemm<1,3,128,256,2> g=pad a=pad P=34 nstages=34', FP32, (48, 16), 64, 3, B, vsrc=True),
    c('igemm<1,3,128,256,2> g=pad a=pad P=32 nstages=32', FP32, 64, 64, 3, A, g=RELU),
    c('igemm<1,4,128,256,2> g=pad a=pad P=32 nstages=32', FP32, 64, 64, 4, A),
    c('igemm<1,7,64,192,2> g=direct a=pad P=8 nstages=8', FP32, 64, 64, 7, (1, 16, 32), mode=REFLECT),
    c('igemm<1,7,128,256,2> g=direct a=pad P=8 nstages=8', FP32, 32, 96, 7, (1, 16, 32), mode=REFLECT),
    c('igemm<1,7,64,192,2> g=direct a=pad P=32 nstages=32', FP32, 3, 32, 7, A, mode=REFLECT),
    c('igemm<1,7,64,192,2> g=pad a=pad P=34 nstages=34', FP32, 3, 64, 7, B, mode=REFLECT),
    c('igemm<2,3,64,64,1> g=direct a=pad P=64 nstages=64', FP32, 8, 16, 3, (2, 64, 64), stride=2),
    c('igemm<2,3,64,64,1> g=pad a=pad P=17 nstages=17', FP32, 16, 16, 3, B, stride=2),
    # (a 64-output stride-2 layer: the table's 64 x 256 entry was written for it, but pick_igemm_tile meets the 64 x 64 entry first,
    # whose padded grid is never larger, and a later entry must undercut the pick by 30 %: igemm<2,3,64,256,1> is never chosen --
    # tests/test_wgrad_edges_cpu.py sweeps the rule for that)
    c('igemm<2,3,64,64,1> g=direct a=pad P=32 nstages=32', FP32, 64, 64, 3, (2, 32, 64), stride=2),
    c('igemm<2,3,128,256,1> g=pad a=pad P=17 nstages=17', FP32, 64, 128, 3, B, stride=2, mode=REFLECT),
    c('igemm<2,4,128,256,1> g=pad a=pad P=32 nstages=32', FP32, 64, 128, 4, A, stride=2),
    c('igemm<2,4,128,256,1> g=pad a=pad P=30 nstages=30', FP32, 16, 64, 4, A, stride=2, pad=0),

    # ---- narrow: the five streaming kernels; the LDS-staged form at its conditions and just off them
    c('narrow<3,1,1,0> g=direct a=direct P=32 nstages=0', FP32, 1, 8, 3, (2, 64, 64)),
    c('narrow<3,1,1,0> g=direct a=direct P=9 nstages=0', FP32, 1, 20, 3, B, mode=REFLECT),
    c('narrow<4,2,1,1> g=direct a=direct P=8 nstages=0', FP32, 1, 64, 4, (2, 64, 64), stride=2),
    c('narrow<4,2,2,1> g=direct a=direct P=8 nstages=0', FP32, 2, 64, 4, (2, 64, 64), stride=2),
    c('narrow<4,2,2,1> g=direct a=direct P=8 nstages=0', FP32, 2, 10, 4, (2, 64, 64), stride=2),
    c('narrow<4,2,1,0> g=direct a=direct P=8 nstages=0', FP32, 1, 64, 4, (2, 64, 48), stride=2),
    c('narrow<4,2,2,0> g=direct a=direct P=5 nstages=0', FP32, 2, 64, 4, (2, 40, 64), stride=2),
    c('narrow<4,2,1,0> g=direct a=direct P=8 nstages=0', FP32, 1, 64, 4, (2, 64, 64), stride=2, mode=REFLECT),
    c('narrow<4,2,2,0> g=direct a=direct P=2 nstages=0', FP32, 2, 3, 4, B, stride=2),
    c('igemm<2,4,128,256,1> g=pad a=pad P=64 nstages=64', FP32, 1, 64, 4, (2, 64, 64), stride=2, g=LRELU),
    c('igemm<1,3,128,256,2> g=pad a=pad P=128 nstages=128', FP32, 1, 8, 3, (2, 64, 64), g=RELU),

    # ---- routes of ops.wgrad above the planner
    c('final', FP32, 16, 1, 7, (2, 20, 52), mode=REFLECT, via='final'),
    c('final', FP32, 24, 1, 7, (1, 33, 47), via='final', vsrc=True),
    c('final', X3, 16, 1, 7, (1, 33, 50), mode=REFLECT, via='final', vsrc=True),
    c('final', FP32, 16, 1, 7, (2, 16, 64), via='final'),
    c('few_outputs: narrow<3,1,1,0> g=direct a=direct P=8 nstages=0', FP32, 16, 2, 3, (1, 30, 34), mode=REFLECT, via='few'),
    c('few_outputs: narrow<3,1,1,0> g=direct a=direct P=17 nstages=0', X3, (16, 8), 3, 3, A, via='few', vsrc=True),
    c('few_outputs: igemm<1,7,64,192,2> g=pad a=pad P=36 nstages=36', FP32, 16, 2, 7, (1, 30, 34), mode=REFLECT, via='few'),
    c('few_outputs: igemm<1,7,64,192,2> g=pad a=pad P=76 nstages=76', FP32, 20, 3, 7, A, via='few'),
    c('igemm<1,4,128,256,2> g=pad a=pad P=32 nstages=32', FP32, 16, 2, 4, A),           # (no few_outputs route for a 4x4 layer)
]


def expected_form(case, f):
    """ops.Form of the case's gradient (f = 'g') or of source segment f, as the GPU test builds the tensors"""
    from animateportrait_amd import ops
    n, h, w = case.shape
    if f == 'g':
        gh, gw = (h + 2 * case.pad - case.k) // case.stride + 1, (w + 2 * case.pad - case.k) // case.stride + 1
        return ops.Form((n, case.m, gh, gw), torch.float32, case.g is not None, case.g or NONE, False, False, False, False)
    virtual = case.vsrc and f == 0
    return ops.Form((n, case.segs[f], h, w), torch.float32, virtual, RELU if virtual else NONE, case.xs == 'plain', case.xs == 's2d',
                    False, False)


def inner_of_few(case):
    """the role-swapped layer ops._wgrad_few_outputs hands back to ops.wgrad, once per output channel: M = Cin rows of the padded
    input against the one-channel gradient, zero padding k - 1"""
    n, h, w = case.shape
    return c(case.route.split(': ', 1)[1], case.prec, 1, sum(case.segs), case.k, (n, h, w), pad=case.k - 1)


def query(case):
    """the route string of a case under the current environment (ops.wgrad_kernel_route; the routes of ops.wgrad by ops.wgrad_route)"""
    from animateportrait_amd import ops
    g, forms = expected_form(case, 'g'), [expected_form(case, i) for i in range(len(case.segs))]
    cin = sum(case.segs)
    if case.via in ('final', 'few'):
        top = ops.wgrad_route(case.k, case.stride, case.pad, case.mode, g, forms, (case.m, cin, case.k, case.k), case.prec, False)
        if case.via == 'final':
            return top
        return top + ': ' + query(inner_of_few(case))
    return ops.wgrad_kernel_route(case.k, case.stride, case.pad, case.mode, g, forms, case.prec, own_g=case.via == 'wgrad')


def family(route):
    return route.split(': ')[-1].split('<', 1)[0]


def p_and_nstages(route):
    m = re.search(r' P=(\d+) nstages=(\d+)', route)
    return int(m.group(1)), int(m.group(2))


# ------------------------------------------------------------------------------------------------ the GPU side
@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


def _act64(t, act):
    return t if act == NONE else (F.relu(t) if act == RELU else F.leaky_relu(t, 0.2))


def _virtual(raw, act, dev):
    """(Feat of act(IN(raw)), its value in fp64 from the same fp32 statistics)"""
    from animateportrait_amd import ops
    n, ch = raw.shape[:2]
    mean = raw.double().mean((2, 3)).float()
    rstd = (raw.double().var((2, 3), unbiased=False) + 1e-5).rsqrt().float()
    val = _act64((raw.double() - mean.double().view(n, ch, 1, 1)) * rstd.double().view(n, ch, 1, 1), act)
    return ops.Feat(raw.to(dev), mean.reshape(-1).to(dev), rstd.reshape(-1).to(dev), act), val


def _r16(t):
    return t.float().bfloat16().double()


def _dw_ref(case, x, up, cin=None, m=None, pad=None, mode=None):
    """autograd of an fp64 convolution with respect to a zero weight"""
    pad = case.pad if pad is None else pad
    w = torch.zeros(m or case.m, cin or x.shape[1], case.k, case.k, dtype=torch.float64, requires_grad=True)
    xp = F.pad(x, (pad,) * 4, mode='reflect') if (case.mode if mode is None else mode) == REFLECT else F.pad(x, (pad,) * 4)
    (F.conv2d(xp, w, stride=case.stride) * up).sum().backward()
    return w.grad


class Problem:
    """The tensors of one case on the device, its fp64 reference, and the direct call of the entry point underneath."""

    def __init__(self, case, dev):
        from animateportrait_amd import ops
        self.case, self.dev = case, dev
        n, h, w = case.shape
        gen = torch.Generator().manual_seed(sum(map(ord, case.name)))
        xs64, self.feats = [], []
        for i, ch in enumerate(case.segs):
            raw = torch.randn(n, ch, h, w, generator=gen) * 1.5 + 0.3
            if case.vsrc and i == 0:
                f, val = _virtual(raw, RELU, dev)
            else:
                f, val = ops.Feat(raw.to(dev)), raw.double()
            xs64.append(val)
            self.feats.append(f)
        x64 = torch.cat(xs64, 1)
        gshape = expected_form(case, 'g').shape
        raw_g = torch.randn(gshape, generator=gen) + 0.25
        self.g_t = self.g_xs = None
        if case.via == 'pre':
            # the gradient of a layer y -> IN -> ReLU as ap_instnorm_bwd_split leaves it: dy in fp32 (the reference's operand) and the
            # M-role operand in the kernel's own layout, with the slots beyond H x W x M zero as its contract asks
            y, _ = _virtual(torch.randn(gshape, generator=gen) * 1.7 + 0.4, RELU, dev)
            dims = ops.wgrad_gt_dims(case.k, case.stride, case.pad, case.mode, gshape, self.feats, case.prec)
            assert dims is not None and dims[2] > case.m and ops.instnorm_bwd_split_ok(y.data, 0)
            self.gf, self.g_t, _ = ops.instnorm_bwd_split((raw_g.to(dev), 0, None), y, dims, want_xs=False, want_dy=True)
            g64 = self.gf.data.cpu().double()
        elif case.g is not None:
            self.gf, g64 = _virtual(raw_g * 1.3, case.g, dev)
        else:
            self.gf, g64 = ops.Feat(raw_g.to(dev)), raw_g.double()
        if case.xs == 'plain':
            for f in self.feats:
                ops.presplit(f, ops.PRECISION_BF16X3)
        elif case.xs == 's2d':
            self.feats[0].s2d = ops.presplit_s2d(self.feats[0])
        if case.via == 'xs':
            self.g_xs = ops.presplit(self.gf, ops.PRECISION_BF16X3)
        # the tensors are what the case table says they are (the CPU reach test asks the planner about these forms)
        assert ops.form_of(self.gf)[:4] == expected_form(case, 'g')[:4]
        assert [ops.form_of(f)[:6] for f in self.feats] == [expected_form(case, i)[:6] for i in range(len(case.segs))]
        cin = x64.shape[1]
        self.out_shape = (case.m, cin, case.k, case.k)
        if case.via == 'few':
            # the inner call, output channel 0: dwt[ci][0][ky'][kx'] = the layer's dw[0][ci] with both tap axes mirrored
            inner = inner_of_few(case)
            self.a_pad = ops.pad_materialize(self.feats, case.pad, case.mode)
            self.g0 = self.gf.data[:, :1].contiguous()
            self.ref = _dw_ref(case, x64, g64)
            self.inner_ref = self.ref[:1].flip(2, 3).permute(1, 0, 2, 3).contiguous()
            self.inner = inner
        elif case.prec == B16 and family(case.route) == 'bf16gemm':
            assert not case.vsrc and case.g is None
            self.ref = _dw_ref(case, _r16(x64), _r16(g64))
        else:
            self.ref = _dw_ref(case, x64, g64)
        fam = family(case.route)
        self.tol = (3e-5 if case.prec == B16 else 5e-5) if fam == 'bf16gemm' else 5e-6
        self.scale = float(self.ref.abs().max())
        assert self.scale > 0

    def direct(self, what):
        """One call of the C entry point into a NaN workspace with a NaN tail and a NaN dw; returns dw after checking the tail."""
        from animateportrait_amd import ops, _capi
        from test_served_shapes_gpu import assert_tail_untouched
        case, lib, dev = self.case, _capi.lib(), self.dev
        if case.via == 'final':
            n, h, w = case.shape
            cin = sum(case.segs)
            nfloats = lib.ap_conv_final_wgrad_workspace_floats(n, cin, h, w)
            shape = self.out_shape
        else:
            lay = self.inner if case.via == 'few' else case
            g = ops.Feat(self.a_pad) if case.via == 'few' else self.gf
            srcs = [ops.Feat(self.g0)] if case.via == 'few' else self.feats
            d = ops._wgrad_desc(lay.k, lay.stride, lay.pad, lay.mode, tuple(g.data.shape), g if case.via in ('wgrad', 'few') else None, srcs, lay.prec)
            nfloats = lib.ap_conv2d_wgrad_workspace_floats(ctypes.byref(d))
            shape = (lay.m, sum(lay.segs), lay.k, lay.k)
        assert nfloats > 0, (what, nfloats, lib.ap_last_error())
        ws = torch.full((nfloats + TAIL_FLOATS,), float('nan'), dtype=torch.float32, device=dev)
        dw = torch.full(shape, float('nan'), dtype=torch.float32, device=dev)
        stream = ops._stream()
        if case.via == 'final':
            s = ops._src_of(self.feats[0])
            rc = lib.ap_conv_final_wgrad(ctypes.byref(s), ops._ptr(self.gf.data), n, h, w, case.k, case.pad, case.mode, ops._ptr(ws), ops._ptr(dw),
                                         stream)
        elif case.via == 'xs':
            assert lib.ap_conv2d_wgrad_xs_ok(ctypes.byref(d)) == 1, what
            rc = lib.ap_conv2d_wgrad_xs(ctypes.byref(d), ops._ptr(self.g_xs), ops._ptr(ws), ops._ptr(dw), stream)
        elif case.via == 'pre':
            rc = lib.ap_conv2d_wgrad_pre(ctypes.byref(d), ops._ptr(self.g_t), ops._ptr(ws), ops._ptr(dw), stream)
        else:
            rc = lib.ap_conv2d_wgrad(ctypes.byref(d), ops._ptr(ws), ops._ptr(dw), stream)
        _capi.check(rc, what)
        assert_tail_untouched(ws, nfloats, what)
        return dw

    def check(self, dw, what):
        ref = self.inner_ref if self.case.via == 'few' else self.ref
        assert not bool(torch.isnan(dw).any()), what + ': NaN in dw (an operand slot was read that no pass wrote)'
        err = linf(dw, ref) / float(ref.abs().max())
        print('%-60s %-28s err %.3g of bar %.0e' % (self.case.name, what, err, self.tol))
        assert err < self.tol, (what, err, self.tol)


def blocks_with_a_ragged_split(case, setenv):
    """the smallest APAMD_WGRAD_BLOCKS whose P does not divide the stage count (None: every reachable P divides it)"""
    for blocks in range(1, 4097):
        setenv('APAMD_WGRAD_BLOCKS', str(blocks))
        p, nstages = p_and_nstages(query(case))
        if nstages % p:
            return blocks
    return None


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES, ids=[k.name for k in CASES])
def test_wgrad_edge(dev, monkeypatch, case):
    from animateportrait_amd import ops
    for v in ops.plan_switch_names():
        monkeypatch.delenv(v, raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    # 1 route
    assert query(case) == case.route
    prob = Problem(case, dev)
    # 2 value through ops.wgrad for its own routes (the planner's cases go through the entry point below: the same call)
    if case.via in ('final', 'few'):
        dw = ops.wgrad(case.k, case.stride, case.pad, case.mode, prob.gf, prob.feats, prob.out_shape, precision=case.prec)
        err = linf(dw, prob.ref) / prob.scale
        print('%-60s %-28s err %.3g of bar %.0e' % (case.name, 'ops.wgrad', err, prob.tol))
        assert err < prob.tol, ('ops.wgrad', err)
    # 2, 3 value and poison, 5 bits
    first = prob.direct('default split')
    prob.check(first, 'default split')
    again = prob.direct('second call')
    assert torch.equal(first.view(torch.int32), again.view(torch.int32)), 'two calls with identical inputs differ'
    # 4 stage split
    if case.via == 'final':
        return                  # (wgrad_final_kernel splits pixel tiles by its own rule; it has no knob)
    lay = prob.inner if case.via == 'few' else case
    fam, (p0, nstages) = family(case.route), p_and_nstages(case.route)
    ragged = blocks_with_a_ragged_split(lay, monkeypatch.setenv) if fam != 'narrow' else None
    for blocks, which in (('1', 'one'), (ragged, 'ragged'), ('100000', 'cap')):
        if blocks is None:
            continue
        monkeypatch.setenv('APAMD_WGRAD_BLOCKS', str(blocks))
        p, ns = p_and_nstages(query(lay))
        assert ns == nstages
        if fam == 'narrow':
            assert p == p0, 'the narrow family does not read the knob'
            continue
        if which == 'one':
            assert p == 1
        elif which == 'ragged':
            assert nstages % p != 0
        else:
            assert p == (max(nstages // 2, 1) if fam == 'bf16gemm' else nstages)
        what = 'P=%d of %d stages' % (p, nstages)
        prob.check(prob.direct(what), what)
