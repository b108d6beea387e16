"""Which bytes do the kernels touch?  Every case runs one C-ABI call through tests/footprint.py: each tensor embedded in
guards, strided tensors with their real ``ld`` (gap columns are surroundings), workspace / statistics partials / amax slots at
exactly the size the library reports.  Written surroundings must stay bit-identical; the outputs must be bit-identical under
zero / NaN / 3e38 surroundings of everything that is read, finite, and equal to the plain call.  The values of the same launches are
judged by tests/test_gpu_case_values.py against the float64 restatement of the two ABIs in tests/abi_ref.py, those of the flat entry
points by tests/test_gpu_flat_values.py against the restatements in tests/flat_ref.py.

The case tables are plain data, importable without a GPU.  A convolution case names its kernel at two levels: the FAMILY string
``keep_conv2d_plan`` reports (the form's name, which the engine's precision policies key on) and the LAUNCHED instantiation
``keep_conv2d_launch_plan`` reports (what the launch takes for the real N, the flags, the chunk count and the activations, follow-up
kernels joined with " + ").  tests/test_host_logic.py asks both (host C) for every convolution case and ``keep_attention_plan`` for every
attention case, and checks that the tables reach every convolution kernel family, every template instantiation keep_conv2d and
keep_attention can launch, and name every launcher of include/keep_hip.h.
"""
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch

import footprint as FP
from abi_ref import AUX_W, LN_EPS, attn_scale
from conftest import op_input
from comfyui_keep_amd.engine import hiplib as L
from comfyui_keep_amd.engine import ops

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
# Largest block of memory one step of a convolution / attention kernel can touch past a tensor edge: a 128-row tile of the
# widest row used here (in_ld <= 2048 floats) = 1 MiB would be the gather tile of a GEMM whose rows run over; the 3x3 halo
# tile is (8 + 2) x (32 + 2) pixels.  Every case below has rows of at most 1040 floats, so 128 rows x 1040 x 4 = 520 KiB.
CONV_TILE_BYTES = 128 * 1040 * 4


def rnd(name, shape, scale=1.0, dtype=F32):
    return op_input('fp:' + name, shape, scale).to(dtype)


# ------------------------------------------------------------------------------------------------ keep_conv2d
# name -> (expected family string of keep_conv2d_plan, expected launched string of keep_conv2d_launch_plan, arguments).  Geometry keys: N H W Cin Cout k stride pad (or pad_t/pad_l) Ho Wo
# (default: same-size for stride 1, the symmetric-padding size otherwise) in_ld in_off out_ld out_off res_ld aux pro pro_act act split_k
# stats amax amax_stale (the amax slots hold stale values and the call says so: x3_out_amax_zeroed = 0) in_amax in2_cin1 reflect upsample
# in_bf16 out_bf16 bk256 ln flags launch (False: plan-only); data keys: pro_amp (prologue rows are 1 +- pro_amp / +- pro_amp, default 0.2),
# bias_amp (default 1), x_amp (input, default 2), w_amp (weights, default 0.05) and w_peak (every w_peak-th input channel's weights at w_amp, the others at w_amp /
# w_peak, or at w_amp * w_floor where that is given; default 1: all alike): set where a tolerance class would otherwise let a kernel that ignores an input,
# or takes a neighbouring activation, pass (tests/test_host_logic.py: every such change moves the reference by >= 100 x the tolerance).
def _c(expect, launched, mma, **kw):
    return expect, launched, dict(mma=mma, **kw)


F_, B_, X_, X1_ = L.MMA_F32, L.MMA_BF16, L.MMA_X3, L.MMA_X1
CONV_CASES = {
    # ---- <= 4 output channels, every policy (exact-fp32 VALU kernel): N = 3, strided input slice, prologue
    'cout4_f32': _c('conv3x3_cout4_kernel',
                    'conv3x3_cout4_kernel', F_, N=3, H=8, W=32, Cin=16, Cout=3, in_ld=24, in_off=4, out_ld=5, out_off=1, pro=True,
                    pro_act=L.PRO_SWISH),
    'cout4_x3': _c('conv3x3_cout4_kernel',
                   'conv3x3_cout4_kernel', X_, N=1, H=16, W=32, Cin=32, Cout=2, act=L.ACT_SIGMOID),
    # ---- RGB first convolutions (rows of 3 floats inside rows of 4: the 4th float is a gap)
    'c3_bf16': _c('conv3x3_c3_kernel',
                  'conv3x3_c3_kernel', B_, N=3, H=8, W=32, Cin=3, Cout=32, in_ld=4, stats=True),
    'c3_x3': _c('conv3x3_c3_x3_kernel',
                'conv3x3_c3_x3_kernel', X_, N=1, H=16, W=32, Cin=3, Cout=48, out_ld=64, out_off=8, in_amax=True, amax=True),
    'c3_x3_dense': _c('conv3x3_c3_x3_kernel',
                      'conv3x3_c3_x3_kernel', X_, N=3, H=8, W=32, Cin=2, Cout=32, in_amax=True, amax=True, stats=True),
    # ---- x3 halo kernels
    'up2_phases': _c('conv3x3_halo_x3_kernel<32, x2 phases>',
                     'conv3x3_halo_x3_kernel<32, 0, true, true, true, true, false>', X_, N=1, H=8, W=32, Cin=16, Cout=64, upsample=2, in_ld=20, in_off=4,
                     res_ld=72, in_amax=True, amax=True),
    'up2_phases_n3': _c('conv3x3_halo_x3_kernel<32, x2 phases>',
                        'conv3x3_up2_x3s_kernel', X_, N=3, H=8, W=32, Cin=48, Cout=64, upsample=2, out_ld=80, out_off=12,
                        in_amax=True),
    'x3s_plain': _c('conv3x3_halo_x3s_kernel',
                    'conv3x3_halo_x3s_kernel<0, false, false>', X_, N=3, H=8, W=32, Cin=32, Cout=32, in_ld=40, in_off=8, out_ld=48, out_off=8, res_ld=36,
                    in_amax=True, amax=True),
    'x3s_pro': _c('conv3x3_halo_x3s_kernel',
                  'conv3x3_halo_x3s_kernel<1, true, false>', X_, N=1, H=16, W=32, Cin=48, Cout=96, pro=True, pro_act=L.PRO_SWISH, stats=True, amax=True),
    'x3s_reflect': _c('conv3x3_halo_x3s_kernel',
                      'conv3x3_halo_x3s_act_kernel<0, false, false, 2>', X_, N=1, H=8, W=32, Cin=32, Cout=32, reflect=True, act=L.ACT_LRELU02, in_amax=True),
    'x3s_up': _c('conv3x3_halo_x3s_kernel',
                 'conv3x3_halo_x3s_kernel<0, false, false>', X_, N=1, H=8, W=16, Cin=32, Cout=32, upsample=1, in_amax=True),
    'halo_x3_16': _c('conv3x3_halo_x3_kernel<16>',
                     'conv3x3_halo_x3_kernel<16, 2, true, true, true, false, false>', X_, N=3, H=16, W=16, Cin=48, Cout=96, pro=True, pro_act=L.PRO_RELU, stats=True,
                     amax=True, in_ld=52, in_off=4),
    'halo_x3_16_aux': _c('conv3x3_halo_x3_kernel<16>',
                         'conv3x3_halo_x3_kernel<16, 0, false, true, true, false, false>', X_, N=1, H=16, W=16, Cin=16, Cout=32, res_ld=40, aux=True, in_amax=True),
    'halo_x3_32_split': _c('conv3x3_halo_x3_kernel<32>',
                           'conv3x3_halo_x3_kernel<32, 0, false, true, true, false, false> + conv_splitk_reduce4_kernel', X_, N=1, H=8, W=32, Cin=48, Cout=32, split_k=3, in_amax=True, res_ld=32),
    'halo_x3_16_autosplit': _c('conv3x3_halo_x3_kernel<16>',
                               'conv3x3_halo_x3_kernel<16, 1, false, true, true, false, false> + conv_splitk_reduce4_kernel', X_, N=1, H=16, W=16, Cin=128, Cout=32, pro=True, pro_act=L.PRO_SWISH),
    # ---- the 64-pixel-block x3 kernels of keep_conv_x3p.hip.  keep_conv2d_plan prints them under the halo names (it names the family whose
    # values they reproduce); the dispatch takes them for few-item launches with Cout % 64 == 0 (keep_conv_x3p_ok / _full_ok / x3q_ok):
    # conv3x3_x3p_kernel<.., 4> as split-K producer, conv3x3_x3p_kernel with the full epilogue (16-wide map, aux), conv3x3_x3q_kernel
    'x3p_partials': _c('conv3x3_halo_x3_kernel<16>',
                       'conv3x3_x3p_kernel<0, true, 4> + conv_splitk_reduce4_kernel', X_, N=3, H=16, W=16, Cin=128, Cout=64, split_k=2, pro=True, in_ld=132, in_off=4, res_ld=72),
    'x3p_full_aux': _c('conv3x3_halo_x3_kernel<16>',
                       'conv3x3_x3p_kernel<0, false, 4>', X_, N=1, H=16, W=16, Cin=64, Cout=64, split_k=1, res_ld=68, aux=True, act=L.ACT_LRELU02,
                       in_amax=True, amax=True, out_ld=72, out_off=4),
    'x3q_small': _c('conv3x3_halo_x3s_kernel',
                    'conv3x3_x3q_kernel<0, false, 0> + conv_stats_replica_kernel', X_, N=3, H=8, W=32, Cin=32, Cout=64, split_k=1, in_ld=40, in_off=8, res_ld=68, act=L.ACT_LRELU02,
                    stats=True, in_amax=True, amax=True),
    # ---- x3 GEMM / gather kernels
    'gemm_x3l_4': _c('gemm_x3l_kernel<4>',
                     'gemm_x3l_kernel<4, 1, true>', X_, N=3, H=64, W=1, Cin=256, Cout=32, k=1, in_ld=260, in_off=4, out_ld=40, out_off=4,
                     res_ld=36, in_amax=True, amax=True, act=L.ACT_GELU),
    'gemm_x3l_8': _c('gemm_x3l_kernel<8>',
                     'gemm_x3l_kernel<8, 1, true>', X_, N=1, H=192, W=1, Cin=1024, Cout=96, k=1, in_amax=True, amax=True),
    'x3_ln': _c('conv_x3_kernel<4, 1, 1, 4, true, true> + LayerNorm',
                'conv_x3_kernel<4, 1, 1, 4, true, true, false, true, false, false>', X_, N=3, H=128, W=1, Cin=48, Cout=128, k=1, ln=True, res_ld=132,
                in_ld=56, in_off=4, in_amax=True, amax=True),
    'x3_gemm_small': _c('conv_x3_kernel<2, 2, 1, 1, true, true>',
                        'conv_x3_kernel<2, 2, 1, 1, true, true, false, true, false, false>', X_, N=1, H=300, W=1, Cin=80, Cout=48, k=1, in_ld=96, in_off=8, out_ld=56,
                        out_off=4, res_ld=52, in_amax=True),
    'x3_gemm_in2': _c('conv_x3_kernel<2, 2, 1, 1, true, true>',
                      'conv_x3_kernel<2, 2, 1, 1, true, true, false, true, false, false>', X_, N=1, H=200, W=1, Cin=80, Cout=48, k=1, in2_cin1=32, in_ld=36),
    'x3_gemm_big': _c('conv_x3_kernel<2, 2, 2, 2, true, true>',
                      'conv_x3_kernel<2, 2, 1, 1, true, true, false, true, false, false>', X_, N=1, H=777, W=1, Cin=48, Cout=96, k=1, in_amax=True, act=L.ACT_GELU),
    'x3_gemm_pro_amax': _c('conv_x3_kernel<2, 2, 1, 1, false, true>',
                           'conv_x3_kernel<2, 2, 1, 1, false, true, false, true, false, false>', X_, N=3, H=8, W=8, Cin=48, Cout=48, k=1, pro=True, stats=True, amax=True),
    'x3_gemm_split': _c('conv_x3_kernel<2, 2, 1, 1, true, true>',
                        'conv_x3_kernel<2, 2, 1, 1, true, true, false, true, false, false> + conv_splitk_reduce4_kernel', X_, N=1, H=300, W=1, Cin=512, Cout=48, k=1, in_amax=True, flags=L.CONV_NO_GEMM_LAT),
    'x3_gather_down': _c('conv_x3_kernel<2, 2, 1, 1, true, false>',
                         'conv_x3_kernel<2, 2, 1, 1, true, false, false, true, false, false> + conv_splitk_reduce4_kernel', X_, N=3, H=10, W=14, Cin=16, Cout=48, stride=2, pad_t=0, pad_l=0,
                         Ho=5, Wo=7, in_amax=True),
    'x3_gather_7x7': _c('conv_x3_kernel<2, 2, 1, 1, false, false>',
                        'conv_x3_kernel<2, 2, 1, 1, false, false, false, true, false, false> + conv_splitk_reduce4_kernel', X_, N=1, H=5, W=7, Cin=144, Cout=48, k=7, pad=3, pro=True,
                        pro_act=L.PRO_RELU, split_k=5),
    'x3_gather_reflect': _c('conv_x3_kernel<2, 2, 2, 2, true, false>',
                            'conv_x3_kernel<2, 2, 1, 1, true, false, false, true, false, false> + conv_splitk_reduce4_kernel', X_, N=1, H=18, W=18, Cin=16, Cout=96, reflect=True, in_amax=True),
    # ---- exact-f32 halo kernel
    'halo_f32_32': _c('conv3x3_halo_f32_kernel<32>',
                      'conv3x3_halo_f32_kernel<32, 1>', F_, N=3, H=8, W=32, Cin=16, Cout=32, in_ld=24, in_off=4, out_ld=48, out_off=8,
                      res_ld=40, pro=True, pro_act=L.PRO_SWISH),
    'halo_f32_16': _c('conv3x3_halo_f32_kernel<16>',
                      'conv3x3_halo_f32_kernel<16, 0>', F_, N=1, H=16, W=16, Cin=48, Cout=96, stats=True, act=L.ACT_LRELU02),
    'halo_f32_16_split': _c('conv3x3_halo_f32_kernel<16>',
                            'conv3x3_halo_f32_kernel<16, 0> + conv_splitk_reduce4_kernel', F_, N=1, H=16, W=16, Cin=48, Cout=96, split_k=3, res_ld=100, aux=True),
    'halo_f32_up_auto': _c('conv3x3_halo_f32_kernel<16>',
                           'conv3x3_halo_f32_kernel<16, 0> + conv_splitk_reduce4_kernel', F_, N=1, H=8, W=8, Cin=128, Cout=32, upsample=1),
    # ---- bf16 halo kernels
    'halo3_f32in_32': _c('conv3x3_halo3_kernel<false, 32>',
                         'conv3x3_halo3_kernel<false, 32, true>', B_, N=1, H=8, W=32, Cin=32, Cout=32, in_ld=40, in_off=8, out_ld=48, out_off=8,
                         res_ld=36),
    'halo3_bf16in_16': _c('conv3x3_halo3_kernel<true, 16>',
                          'conv3x3_halo3_kernel<true, 16, true>', B_, N=3, H=16, W=16, Cin=32, Cout=64, in_bf16=True, out_bf16=True, bias_amp=2.0),
    'halo3_bf16in_split': _c('conv3x3_halo3_kernel<true, 32>',
                             'conv3x3_halo3_kernel<true, 32, false> + conv_splitk_reduce4_kernel', B_, N=1, H=8, W=32, Cin=96, Cout=96, in_bf16=True, split_k=3, act=L.ACT_GELU),
    'halo_bf16_pro_fused': _c('conv3x3_halo3_kernel<false, 16>',
                              'conv3x3_halo_kernel<false, 16>', B_, N=1, H=16, W=16, Cin=32, Cout=64, pro=True, pro_act=L.PRO_SWISH, stats=True, pro_amp=0.8, x_amp=0.7, w_amp=0.1),
    'halo_bf16_needs_prenorm': _c('(keep_norm_act_bf16 first)',
                                  '', B_, N=1, H=16, W=16, Cin=32, Cout=64, in_bf16=True, pro=True, launch=False),
    # ---- bf16 gather kernels
    'bf16_t0': _c('conv_bf16_kernel<4, 1, 1, 1, 64, 1, false>',
                  'conv_bf16_kernel<4, 1, 1, 1, 64, 1, false> + conv_splitk_reduce4_kernel', B_, N=3, H=5, W=7, Cin=24, Cout=20, stride=2, in_ld=28, in_off=4),
    'bf16_t1_plain': _c('conv_bf16_kernel<2, 2, 1, 1, 64, 1, true>',
                        'conv_bf16_kernel<2, 2, 1, 1, 64, 1, true>', B_, N=1, H=300, W=1, Cin=80, Cout=48, k=1, in_ld=96, in_off=8, out_ld=56,
                        out_off=4, res_ld=52, out_bf16=False),
    'bf16_t1_pro': _c('conv_bf16_kernel<2, 2, 1, 1, 64, 1, false>',
                      'conv_bf16_kernel<2, 2, 1, 1, 64, 1, false> + conv_splitk_reduce4_kernel', B_, N=1, H=5, W=7, Cin=130, Cout=48, k=7, pad=3, pro=True, pro_act=L.PRO_RELU, pro_amp=0.8,
                      bias_amp=1.5, x_amp=0.5),
    'bf16_t1_bf16out': _c('conv_bf16_kernel<2, 2, 1, 1, 64, 1, true>',
                          'conv_bf16_kernel<2, 2, 1, 1, 64, 1, true>', B_, N=1, H=250, W=1, Cin=48, Cout=64, k=1, out_bf16=True),
    'bf16_t1_bk256': _c('conv_bf16_kernel<2, 2, 1, 1, 256, 1, false>',
                        'conv_bf16_kernel<2, 2, 1, 1, 256, 1, false>', B_, N=1, H=100, W=1, Cin=512, Cout=64, k=1, bk256=True),
    'bf16_t2': _c('conv_bf16_kernel<2, 2, 2, 2, 64, 1, true>',
                  'conv_bf16_kernel<2, 2, 2, 2, 64, 1, true>', B_, N=1, H=4133, W=1, Cin=16, Cout=96, k=1, stats=False),
    'bf16_t2_up': _c('conv_bf16_kernel<2, 2, 2, 2, 64, 1, false>',
                     'conv_bf16_kernel<2, 2, 2, 2, 64, 1, false> + conv_splitk_reduce4_kernel', B_, N=1, H=33, W=35, Cin=16, Cout=96, upsample=1),
    'bf16_flatk': _c('conv_bf16_kernel<2, 2, 1, 1, 64, 1, false>',
                     'conv_bf16_kernel<2, 2, 1, 1, 64, 1, false>', B_, N=1, H=5, W=7, Cin=3, Cout=48),
    # ---- exact-f32 gather kernels
    'f32_t0_7x7': _c('conv_f32_kernel<4, 1, 1, 1>',
                     'conv_f32_kernel<4, 1, 1, 1, false> + conv_splitk_reduce4_kernel', F_, N=1, H=5, W=7, Cin=130, Cout=32, k=7, pad=3, in_ld=132),
    'f32_t0_down': _c('conv_f32_kernel<4, 1, 1, 1>',
                      'conv_f32_kernel<4, 1, 1, 1, false> + conv_splitk_reduce_kernel', F_, N=3, H=10, W=14, Cin=24, Cout=20, stride=2, pad_t=0, pad_l=0, Ho=5, Wo=7,
                      pro=True, pro_act=L.PRO_SWISH, out_ld=23, out_off=2),
    'f32_t1': _c('conv_f32_kernel<2, 2, 1, 1>',
                 'conv_f32_kernel<2, 2, 1, 1, true>', F_, N=1, H=300, W=1, Cin=80, Cout=48, k=1, in_ld=96, in_off=8, out_ld=56, out_off=4,
                 res_ld=52, act=L.ACT_GELU),
    'f32_t1_split': _c('conv_f32_kernel<2, 2, 1, 1>',
                       'conv_f32_kernel<2, 2, 1, 1, true> + conv_splitk_reduce_kernel', F_, N=1, H=5, W=7, Cin=48, Cout=48, split_k=4, res_ld=50, aux=True),
    'f32_t1_autosplit': _c('conv_f32_kernel<2, 2, 1, 1>',
                           'conv_f32_kernel<2, 2, 1, 1, true> + conv_splitk_reduce4_kernel', F_, N=1, H=8, W=8, Cin=512, Cout=64, k=1),
    'f32_t1_stats': _c('conv_f32_kernel<2, 2, 1, 1>',
                       'conv_f32_kernel<2, 2, 1, 1, false>', F_, N=3, H=8, W=8, Cin=24, Cout=48, k=1, stats=True),
    'f32_t1_reflect_up': _c('conv_f32_kernel<2, 2, 1, 1>',
                            'conv_f32_kernel<2, 2, 1, 1, false> + conv_splitk_reduce4_kernel', F_, N=1, H=5, W=7, Cin=10, Cout=40, reflect=True, upsample=1),
    'f32_t1_flatk': _c('conv_f32_kernel<2, 2, 1, 1>',
                       'conv_f32_kernel<2, 2, 1, 1, false>', F_, N=3, H=9, W=11, Cin=3, Cout=36, stride=2),
    'f32_t2': _c('conv_f32_kernel<2, 2, 2, 2>',
                 'conv_f32_kernel<2, 2, 2, 2, true>', F_, N=1, H=777, W=1, Cin=48, Cout=96, k=1, res_ld=96),
    'f32_t2_x3_fallback': _c('conv_f32_kernel<2, 2, 2, 2>',
                             'conv_f32_kernel<2, 2, 2, 2, false>', X_, N=1, H=777, W=1, Cin=40, Cout=130, k=1, in_amax=False),
}

# ------------------------------------------------------------------------------------------------ the table, grown to the universe
# Every instantiation keep_conv2d can launch (tests/test_host_logic.py: test_conv_table_reaches_every_instantiation) has a case: the
# families below are dealt out arm by arm, each case at the smallest shape that still takes its arm -- one or two 256-pixel tiles, N <= 3,
# the smallest Cin that gives the chunk count -- with the launched string spelled from the case's own parameters.
_ACT_NAMES = {L.ACT_NONE: 'none', L.ACT_RELU: 'relu', L.ACT_LRELU02: 'lrelu02', L.ACT_GELU: 'gelu', L.ACT_SIGMOID: 'sigmoid',
              L.ACT_LRELU01: 'lrelu01', L.ACT_SILU: 'silu'}
_NSP, _EXACT, _NOSTREAM = L.CONV_NO_SMALL_PARTIALS, L.CONV_X3_EXACT_ACT, L.CONV_NO_STREAM


def _b(v):
    return 'true' if v else 'false'


def _awkward(i, Cin, Cout, fused=True):
    """The table's awkwardness, dealt round-robin over a family: a strided input slice, a strided output, res_ld != Cout, N = 3 with
    per-image maxima, statistics (``fused`` = False: a form that cannot emit amax / statistics takes N = 3 / N = 2 plain)."""
    return [dict(in_ld=Cin + 8, in_off=8), dict(out_ld=Cout + 16, out_off=8), dict(res_ld=Cout + 4),
            dict(N=3, in_amax=True, amax=True) if fused else dict(N=3, in_amax=True),
            dict(stats=True, amax=True) if fused else dict(N=2)][i % 5]


# The single-fp16 bound is per output, (2^-10 + 2e-6) sum |x| |w|: with 288 like terms a neighbouring activation moves an output by less than
# 100 x that.  The x1 cases therefore sum few dominant terms (one input channel in 32 at full weight) behind a wide prologue, and the
# sigmoid cases -- whose slope of at most 1/4 the bound does not know -- keep the other channels at 1/1024 and the outputs near zero.
_X1_DATA = dict(w_peak=32, pro_amp=1.0, w_amp=0.02)
_X1_SIGMOID = dict(w_peak=16, w_floor=1.0 / 1024, pro_amp=0.8, w_amp=0.05, bias_amp=0.15, x_amp=1.2)


def _grow(cases):
    i = 0
    # ---- the streaming kernel: <PRO, AFF, X1> x the epilogue activation, x3 and single fp16 (x3 launches of so few items stay on it under
    # CONV_NO_SMALL_PARTIALS; the x1 form has no 64-pixel twin)
    pro_forms = {'raw': (L.PRO_NONE, False), 'aff': (L.PRO_NONE, True), 'affswish': (L.PRO_SWISH, True), 'affrelu': (L.PRO_RELU, True)}
    for x1 in (False, True):
        for pname, (pact, aff) in pro_forms.items():
            for act, aname in _ACT_NAMES.items():
                targs = f'{pact}, {_b(aff)}, {_b(x1)}'
                launched = f'conv3x3_halo_x3s_kernel<{targs}>' if act == L.ACT_NONE else f'conv3x3_halo_x3s_act_kernel<{targs}, {act}>'
                expect = f'conv3x3_halo_x3s_kernel<{pact}, {_b(aff)}, true>' if x1 else 'conv3x3_halo_x3s_kernel'
                kw = dict(N=1, H=8, W=32, Cin=32, Cout=64, pro=aff, pro_act=pact, act=act, split_k=1, flags=0 if x1 else _NSP)
                if x1:
                    kw.update(_X1_SIGMOID if act == L.ACT_SIGMOID else _X1_DATA)
                cases[f"{'x1s' if x1 else 'x3s'}_{pname}_{aname}"] = _c(expect, launched, X1_ if x1 else X_, **dict(kw, **_awkward(i, 32, 64)))
                i += 1
    # ---- the stage-barrier halo kernel: <TW, PRO, SIMPLE_EPI, FASTACT, WDMA, UP2 = false, X1 = false>.  16-wide maps always run it; 32-wide
    # maps under CONV_NO_STREAM, or with the exact swish (the streaming kernel has the fast form only).  Cout = 96: no 64-pixel blocks.
    for tw, (H, W) in ((16, (16, 16)), (32, (8, 32))):
        for pname, (pact, aff, exact) in {'raw': (L.PRO_NONE, False, False), 'relu': (L.PRO_RELU, True, False), 'swish': (L.PRO_SWISH, False, False),
                                          'swish_exact': (L.PRO_SWISH, True, True)}.items():
            for simple in (True, False):
                launched = f'conv3x3_halo_x3_kernel<{tw}, {pact}, {_b(simple)}, {_b(not exact)}, {_b(not exact)}, false, false>'
                kw = dict(N=1, H=H, W=W, Cin=32, Cout=96, pro=aff, pro_act=pact, act=L.ACT_NONE if simple else (L.ACT_GELU if exact else L.ACT_LRELU02),
                          split_k=1, flags=(_EXACT if exact else 0) | (_NOSTREAM if tw == 32 and not exact else 0))
                cases[f"halo_x3_{tw}_{pname}_{'simple' if simple else 'act'}"] = _c(f'conv3x3_halo_x3_kernel<{tw}>', launched, X_, **dict(kw, **_awkward(i, 32, 96)))
                i += 1
    # ---- its single-fp16 16 x 16 form (CONV_X1_HALO16): <16, 0, SIMPLE_EPI, true, true, false, true>
    for simple in (True, False):
        k_ = f'conv3x3_halo_x3_kernel<16, 0, {_b(simple)}, true, true, false, true>'
        cases[f"x1_halo16_{'simple' if simple else 'act'}"] = _c(k_, k_, X1_, N=3, H=16, W=16, Cin=32, Cout=32, act=L.ACT_NONE if simple else L.ACT_SILU,
                                                                  flags=L.CONV_X1_HALO16, in_amax=True, amax=True, stats=simple, res_ld=0 if simple else 36, **_X1_DATA)
    # ---- the 64-pixel split-K producer: <PRO, SC, NCH>, NCH = chunks per K range where every range has 4, 8 or 16 (else 0)
    for pname, (pact, sc) in {'raw': (L.PRO_NONE, False), 'aff': (L.PRO_NONE, True), 'swish': (L.PRO_SWISH, False), 'affswish': (L.PRO_SWISH, True)}.items():
        for nch, Cin in ((0, 96), (4, 128), (8, 256), (16, 512)):
            launched = f'conv3x3_x3p_kernel<{pact}, {_b(sc)}, {nch}> + conv_splitk_reduce4_kernel'
            kw = dict(N=1, H=16, W=16, Cin=Cin, Cout=64, pro=sc, pro_act=pact, split_k=2)
            cases[f'x3p_{pname}_nch{nch}'] = _c('conv3x3_halo_x3_kernel<16>', launched, X_, **dict(kw, **_awkward(i, Cin, 64, fused=False)))
            i += 1
    # ---- the 64-pixel blocks with the streaming kernel's values: <PRO, AFF, NCH>, NCH = Cin / 16 where that is 4, 8, 16 or 32 (else 0)
    for pname, (pact, aff) in {'raw': (L.PRO_NONE, False), 'aff': (L.PRO_NONE, True), 'affswish': (L.PRO_SWISH, True)}.items():
        for nch, Cin in ((0, 48), (4, 64), (8, 128), (16, 256), (32, 512)):
            kw = dict(dict(N=1, H=8, W=32, Cin=Cin, Cout=64, pro=aff, pro_act=pact, split_k=1), **_awkward(i, Cin, 64))
            launched = f'conv3x3_x3q_kernel<{pact}, {_b(aff)}, {nch}>' + (' + conv_stats_replica_kernel' if kw.get('stats') else '')
            cases[f'x3q_{pname}_nch{nch}'] = _c('conv3x3_halo_x3s_kernel', launched, X_, **kw)
            i += 1
    # ---- exact-f32 halo kernel <TW, PRO>, bf16 halo kernel <IN_BF16, TW, SIMPLE_EPI>
    for tw, (H, W) in ((16, (16, 16)), (32, (8, 32))):
        for pact, pname in ((L.PRO_NONE, 'raw'), (L.PRO_SWISH, 'swish'), (L.PRO_RELU, 'relu')):
            kw = dict(N=1, H=H, W=W, Cin=16, Cout=32, pro=pact != L.PRO_NONE, pro_act=pact, split_k=1)
            cases[f'halo_f32_{tw}_{pname}'] = _c(f'conv3x3_halo_f32_kernel<{tw}>', f'conv3x3_halo_f32_kernel<{tw}, {pact}>', F_, **dict(kw, **_awkward(i, 16, 32, fused=False)))
            i += 1
        for inb in (False, True):
            for simple in (True, False):
                kw = dict(N=1, H=H, W=W, Cin=32, Cout=64, in_bf16=inb, act=L.ACT_NONE if simple else L.ACT_LRELU02, split_k=1)
                cases[f"halo3_{'bf16in' if inb else 'f32in'}_{tw}_{'simple' if simple else 'act'}"] = _c(
                    f'conv3x3_halo3_kernel<{_b(inb)}, {tw}>', f'conv3x3_halo3_kernel<{_b(inb)}, {tw}, {_b(simple)}>', B_, **dict(kw, **_awkward(i, 32, 64, fused=False)))
                i += 1


_grow(CONV_CASES)
CONV_CASES.update({
    # ---- the first bf16 halo kernel on a 32-wide map (the prologue fused into its staging step)
    'halo_bf16_pro_fused_32': _c('conv3x3_halo3_kernel<false, 32>', 'conv3x3_halo_kernel<false, 32>', B_, N=3, H=8, W=32, Cin=32, Cout=64, pro=True,
                                 pro_act=L.PRO_SWISH, split_k=1, pro_amp=0.8, x_amp=0.7, w_amp=0.1),
    # ---- the single-fp16 phase kernel (CONV_X1_UP2), and a call whose amax slots hold stale values: the launch zeroes them first
    'up2_x1s': _c('conv3x3_halo_x3_kernel<32, x2 phases, true>', 'conv3x3_up2_x1s_kernel', X1_, N=3, H=8, W=32, Cin=32, Cout=64, upsample=2, in_amax=True,
                  amax=True, flags=L.CONV_X1_UP2, out_ld=80, out_off=12),
    'x3s_stale_amax': _c('conv3x3_halo_x3s_kernel', 'zero_u32_kernel + conv3x3_halo_x3s_kernel<0, false, false>', X_, N=3, H=8, W=32, Cin=32, Cout=64,
                         split_k=1, in_amax=True, amax=True, amax_stale=True, flags=_NSP),
    # ---- conv_x3_kernel<tile, PLAIN, ONE, KSL, DEEP, KAL, X1>: canonical K slices on the block-tile kernel (CONV_GEMM_LAT_TILES: two K steps per
    # slice, then the four-step form of Cin = 512 and of Cin = 1024 on eight slices)
    'x3_gemm_kslice2': _c('gemm_x3l_kernel<4>', 'conv_x3_kernel<2, 2, 1, 1, true, true, true, true, false, false>', X_, N=3, H=64, W=1, Cin=256, Cout=32, k=1,
                          in_ld=264, in_off=4, res_ld=36, in_amax=True, amax=True, flags=L.CONV_GEMM_LAT_TILES),
    'x3_gemm_kslice4': _c('gemm_x3l_kernel<4>', 'conv_x3_kernel<2, 2, 1, 1, true, true, true, true, true, false>', X_, N=1, H=128, W=1, Cin=512, Cout=96, k=1,
                          out_ld=104, out_off=4, act=L.ACT_GELU, in_amax=True, flags=L.CONV_GEMM_LAT_TILES),
    'x3_gemm_kslice4_deep': _c('gemm_x3l_kernel<8>', 'conv_x3_kernel<2, 2, 1, 1, true, true, true, true, true, false>', X_, N=1, H=64, W=1, Cin=1024, Cout=32, k=1,
                               in_amax=True, amax=True, flags=L.CONV_GEMM_LAT_TILES),
    # ---- the 128 x 128 tile: a launch of few rows keeps it only with statistics it must emit itself (CONV_NO_SMALL_PARTIALS: no replica kernel)
    'x3_t2_gemm': _c('conv_x3_kernel<2, 2, 2, 2, true, true>', 'conv_x3_kernel<2, 2, 2, 2, true, true, false, true, false, false>', X_, N=1, H=384, W=1, Cin=48,
                     Cout=96, k=1, split_k=1, stats=True, amax=True, in_amax=True, in_ld=56, in_off=4, flags=_NSP),
    'x3_t2_gemm_pro': _c('conv_x3_kernel<2, 2, 2, 2, false, true>', 'conv_x3_kernel<2, 2, 2, 2, false, true, false, true, false, false>', X_, N=2, H=384, W=1, Cin=48,
                         Cout=96, k=1, split_k=1, pro=True, pro_act=L.PRO_SWISH, stats=True, flags=_NSP),
    'x3_t2_gather': _c('conv_x3_kernel<2, 2, 2, 2, true, false>', 'conv_x3_kernel<2, 2, 2, 2, true, false, false, true, false, false>', X_, N=1, H=32, W=48, Cin=16,
                       Cout=96, stride=2, split_k=1, stats=True, res_ld=100, flags=_NSP),
    'x3_t2_gather_pro': _c('conv_x3_kernel<2, 2, 2, 2, false, false>', 'conv_x3_kernel<2, 2, 2, 2, false, false, false, true, false, false>', X_, N=1, H=32, W=48,
                           Cin=16, Cout=128, stride=2, split_k=1, pro=True, pro_act=L.PRO_RELU, stats=True, act=L.ACT_LRELU02, flags=_NSP),
    'x3_t2_stats_replica': _c('conv_x3_kernel<2, 2, 2, 2, true, false>',
                              'conv_x3_kernel<2, 2, 1, 1, true, false, false, true, false, false> + conv_x3_gather_stats_replica_kernel', X_, N=3, H=32, W=48,
                              Cin=16, Cout=96, stride=2, split_k=1, stats=True, amax=True, in_amax=True),
    # ---- ... and the one form that cannot be small: more than 262144 output rows on the 64 x 64 tile take the shallow pipeline
    'x3_gather_shallow': _c('conv_x3_kernel<2, 2, 1, 1, true, false>', 'conv_x3_kernel<2, 2, 1, 1, true, false, false, false, false, false>', X_, N=1, H=1026, W=1026,
                            Cin=16, Cout=48, stride=2, in_amax=True),
    # ---- the single-fp16 forms of conv_x3_kernel: im2col and (CONV_X1_GEMM) the 1x1 GEMM, on both tiles
    'x1_im2col': _c('conv_x3_kernel<2, 2, 1, 1, true, 0, 0, 1, 0, 1>', 'conv_x3_kernel<2, 2, 1, 1, true, false, false, true, false, true>', X1_, N=3, H=16, W=16,
                    Cin=32, Cout=64, stride=2, split_k=1, in_amax=True, amax=True, stats=True),
    'x1_gemm': _c('conv_x3_kernel<2, 2, 1, 1, true, 1, 0, 1, 0, 1>', 'conv_x3_kernel<2, 2, 1, 1, true, true, false, true, false, true>', X1_, N=1, H=100, W=1, Cin=64,
                  Cout=48, k=1, split_k=1, in_ld=72, in_off=4, out_ld=56, out_off=4, res_ld=52, act=L.ACT_LRELU01, flags=L.CONV_X1_GEMM),
    'x1_t2_im2col': _c('conv_x3_kernel<2, 2, 2, 2, true, 0, 0, 1, 0, 1>', 'conv_x3_kernel<2, 2, 2, 2, true, false, false, true, false, true>', X1_, N=1, H=32, W=48,
                       Cin=32, Cout=96, stride=2, split_k=1, stats=True, flags=_NSP),
    'x1_t2_gemm': _c('conv_x3_kernel<2, 2, 2, 2, true, 1, 0, 1, 0, 1>', 'conv_x3_kernel<2, 2, 2, 2, true, true, false, true, false, true>', X1_, N=2, H=384, W=1,
                     Cin=64, Cout=96, k=1, split_k=1, stats=True, amax=True, in_amax=True, flags=L.CONV_X1_GEMM | _NSP),
})


class _Geom:
    """The derived sizes and the optional-tensor list of one convolution case."""

    def __init__(self, kw):
        g = dict(k=3, stride=1, in_off=0, out_off=0, res_ld=0, aux=False, pro=False, pro_act=L.PRO_NONE, act=L.ACT_NONE, split_k=0,
                 stats=False, amax=False, in_amax=False, in2_cin1=0, reflect=False, upsample=0, in_bf16=False, out_bf16=False,
                 bk256=False, ln=False, flags=0, launch=True, pro_amp=0.2, bias_amp=1.0, w_amp=0.05, w_peak=1, w_floor=0.0, x_amp=2.0, amax_stale=False)
        g.update(kw)
        self.__dict__.update(g)
        k = self.k
        pad = g.get('pad', k // 2)
        self.pad_t, self.pad_l = g.get('pad_t', pad), g.get('pad_l', pad)
        Hv, Wv = (2 * self.H, 2 * self.W) if self.upsample else (self.H, self.W)
        self.Ho = g.get('Ho', (Hv + 2 * self.pad_t - k) // self.stride + 1)
        self.Wo = g.get('Wo', (Wv + 2 * self.pad_l - k) // self.stride + 1)
        self.cin1 = self.in2_cin1 if self.in2_cin1 else self.Cin           # channels read from `in`
        self.in_ld = g.get('in_ld', self.cin1)
        self.out_ld = g.get('out_ld', self.Cout)
        self.x1 = self.mma == L.MMA_X1                                     # weight_x3 is the hi-only fp16 twin
        self.x3 = self.mma in (L.MMA_X3, L.MMA_X1) and self.Cin % 16 == 0  # the call brings weight_x3


def _conv_args(g, t):
    """keep_conv2d_args of case geometry ``g`` on tensors ``t`` (name -> tensor, or name -> fake address for the host-only plan)."""
    def p(name):
        v = t.get(name)
        return v.data_ptr() if isinstance(v, torch.Tensor) else v
    a = L.conv_args(
        inp=p('x'), weight=p('w'), bias=p('bias'), out=p('out'), pro_scale=p('pro_scale'), pro_shift=p('pro_shift'), residual=p('res'),
        aux=p('aux'), workspace=p('ws'), N=g.N, H=g.H, W=g.W, Cin=g.Cin, Cout=g.Cout, KH=g.k, KW=g.k, stride=g.stride, pad_t=g.pad_t,
        pad_l=g.pad_l, Ho=g.Ho, Wo=g.Wo, in_ld=g.in_ld, out_ld=g.out_ld, res_ld=g.res_ld, upsample=g.upsample, pro_act=g.pro_act,
        epi_act=g.act, aux_w=AUX_W, split_k=g.split_k, dtype=L.BF16 if g.in_bf16 else L.F32, mma=g.mma, weight_bf16=p('wb'),
        stats_out=p('stats'), stats_P=t.get('stats_P', 0), bk256=int(g.bk256), out_dtype=L.BF16 if g.out_bf16 else L.F32,
        weight_x3=p('wx3'), x3_acc_scale=float(t.get('acc_scale', 1.0)), x3_in_amax=p('in_amax'), x3_out_amax=p('amax'),
        x3_out_amax_zeroed=1 if g.amax and not g.amax_stale else 0, in2=p('x2'), in2_cin1=g.in2_cin1, pad_mode=L.PAD_REFLECT if g.reflect else L.PAD_ZERO,
        ln_gamma=p('ln_gamma'), ln_beta=p('ln_beta'), ln_eps=LN_EPS if g.ln else 0.0, flags=g.flags, plan_ref_images=0)
    return a


def _fake_tensors(g):
    """name -> the address modulo 16 every tensor of geometry ``g`` will have (allocations are 16-byte aligned, slices start ``off``
    elements in): all the host-only plan queries look at."""
    base = 0x10000
    isz = 2 if g.in_bf16 else 4
    t = {'x': base + g.in_off * isz, 'w': base, 'bias': base, 'out': base + g.out_off * (2 if g.out_bf16 else 4)}
    if g.pro:
        t['pro_scale'] = t['pro_shift'] = base
    if g.res_ld:
        t['res'] = base
    if g.aux:
        t['aux'] = base
    if g.mma == L.MMA_BF16:
        t['wb'] = base
    if g.x3:
        t['wx3'] = base
    if g.in_amax:
        t['in_amax'] = base
    if g.in2_cin1:
        t['x2'] = base
    if g.ln:
        t['ln_gamma'] = t['ln_beta'] = base
    if g.split_k > 1:
        t['ws'] = base
    return t


def conv_case_plan(name, kw=None):
    """keep_conv2d_plan of a table case without a GPU: pointers only contribute their alignment.  ``kw``: a variant of the
    case's geometry (the exact-f32 twin of an x3 case, tests/test_gpu_case_values.py) instead of the table's own."""
    expect, _, kw0 = CONV_CASES[name]
    g = _Geom(kw0 if kw is None else kw)
    return expect, g, L.conv2d_plan(_conv_args(g, _fake_tensors(g)))


def conv_case_launched(name):
    """keep_conv2d_launch_plan of a table case without a GPU, for the arguments the tests launch: the plan's split-K with its workspace,
    the statistics partials and amax slots the case asks for."""
    _, g, plan = conv_case_plan(name)
    t = _fake_tensors(g)
    if plan.split_k > 1:
        t['ws'] = 0x10000
    if g.stats:
        t['stats'], t['stats_P'] = 0x10000, plan.stats_P
    if g.amax:
        t['amax'] = 0x10000 + 12
    a = _conv_args(g, t)
    a.split_k = plan.split_k
    return L.conv2d_launch_plan(a)


def conv_case_x(name, g):
    """The input payload of case ``name`` (channels [0, cin1) of `in`)."""
    return rnd(name + 'x', (g.N, g.H, g.W, g.cin1), g.x_amp) + 0.3


def _conv_regions(name, kw=None, x=None):
    """(geometry, plan, regions, extra arguments) of a table case; the tensors depend on ``name`` alone, so a variant geometry
    ``kw`` (see conv_case_plan) gets the same data, with ``x`` replacing the input payload where the variant reads another one."""
    expect, g, plan = conv_case_plan(name, kw)
    assert kw is not None or plan.kernel.decode() == expect, (name, plan.kernel.decode(), expect)
    tb = CONV_TILE_BYTES
    idt = BF16 if g.in_bf16 else F32
    N, Cin, Cout = g.N, g.Cin, g.Cout
    x = conv_case_x(name, g) if x is None else x
    w = rnd(name + 'w', (Cout, g.k, g.k, Cin), g.w_amp)
    if g.w_peak > 1:      # every w_peak-th input channel at full amplitude, the others at 1 / w_peak of it: a sum of few dominant terms
        w = w * torch.where(torch.arange(Cin) % g.w_peak == 0, 1.0, g.w_floor or 1.0 / g.w_peak)
    R = [FP.single('x', x.to(idt), ld=g.in_ld, off=g.in_off, tile_bytes=tb), FP.single('w', w.reshape(Cout, -1), tile_bytes=tb),
         FP.single('bias', rnd(name + 'b', (1, Cout)) * g.bias_amp, tile_bytes=tb),
         FP.output('out', (N * g.Ho * g.Wo, Cout), BF16 if g.out_bf16 else F32, ld=g.out_ld, off=g.out_off, tile_bytes=tb)]
    extra = {}
    if g.pro:
        R.append(FP.single('pro_scale', rnd(name + 'ps', (N, Cin)) * g.pro_amp + 1, tile_bytes=tb))
        R.append(FP.single('pro_shift', rnd(name + 'ph', (N, Cin)) * g.pro_amp, tile_bytes=tb))
    if g.res_ld:
        R.append(FP.single('res', rnd(name + 'r', (N * g.Ho * g.Wo, Cout)), ld=g.res_ld, tile_bytes=tb))
    if g.aux:
        R.append(FP.single('aux', rnd(name + 'a', (N * g.Ho * g.Wo, Cout)), tile_bytes=tb))
    if g.mma == L.MMA_BF16:
        R.append(FP.single('wb', w.reshape(Cout, -1).to(BF16), tile_bytes=tb))
    if g.x3:
        wsrc = ops.up2_phase_weights(w) if g.upsample == L.UPSAMPLE_X2_PHASES else w
        sc = ops.x3_scale_for(float(wsrc.abs().max()))
        wx3 = (wsrc.reshape(-1, Cin) * sc).to(torch.float16).view(torch.int16) if g.x1 else ops.split_x3(wsrc.reshape(-1, Cin), sc)
        R.append(FP.single('wx3', wx3.reshape(wx3.shape[0], -1), tile_bytes=tb))
        extra['acc_scale'] = 1.0 / sc
    if g.in_amax:      # (any upper bound of max |x| per image works: the true one, in [N] floats with nothing behind it)
        xin = x.float()
        if g.pro:      # x3_in_amax bounds what enters the product: the input behind the GroupNorm affine (an activation never raises it)
            rows = {n: d for r in R for n, (_, _, d) in r.windows.items() if n in ('pro_scale', 'pro_shift')}
            xin = xin * rows['pro_scale'].reshape(N, 1, 1, Cin) + rows['pro_shift'].reshape(N, 1, 1, Cin)
        R.append(FP.single('in_amax', xin.reshape(N, -1).abs().amax(1).reshape(1, N), tile_bytes=tb))
    if g.in2_cin1:
        R.append(FP.single('x2', rnd(name + 'x2', (N * g.H * g.W, Cin - g.cin1)), tile_bytes=tb))
    if g.ln:
        R.append(FP.single('ln_gamma', rnd(name + 'lg', (1, Cout)) * 0.2 + 1, tile_bytes=tb))
        R.append(FP.single('ln_beta', rnd(name + 'lb', (1, Cout)) * 0.2, tile_bytes=tb))
    if plan.split_k > 1:      # exactly the bytes the plan reports; scratch, not an output
        assert plan.workspace_bytes == plan.split_k * N * g.Ho * g.Wo * Cout * 4
        R.append(FP.output('ws', (1, plan.workspace_bytes // 4), tile_bytes=tb, compare=False))
    if g.stats:
        assert plan.stats_P > 0, (name, 'the case asks for statistics the plan cannot emit')
        R.append(FP.output('stats', (1, N * plan.stats_P * Cout * 2), tile_bytes=tb))
        extra['stats_P'] = plan.stats_P
    if g.amax:         # slots 3 .. 3 + N of an 11-slot arena the caller zeroed: the neighbours are other launches' maxima
        assert plan.out_amax_ok, (name, 'the case asks for x3_out_amax the plan cannot fill')
        R.append(FP.Region(1, 11, {'amax': (3, N, torch.full((1, N), AMAX_STALE if g.amax_stale else 0.0))}, F32, 'rw', tb))
    return g, plan, R, extra


@pytest.mark.parametrize('name', [n for n, (_, _, kw) in CONV_CASES.items() if kw.get('launch', True)])
def test_conv2d_footprint(name):
    g, plan, regions, extra = _conv_regions(name)
    launched = CONV_CASES[name][1]

    def launch(t):
        a = _conv_args(g, {**t, **extra})
        pl = L.conv2d_plan(a)
        sig = (pl.kernel, pl.split_k, pl.workspace_bytes, pl.stats_P, pl.out_amax_ok)
        assert sig == (plan.kernel, plan.split_k, plan.workspace_bytes, plan.stats_P, plan.out_amax_ok), (name, sig)
        a.split_k = pl.split_k
        assert L.conv2d_launch_plan(a) == launched, (name, L.conv2d_launch_plan(a), launched)      # of the very arguments launched below
        L.conv2d_launch(a)
        return sig

    out = FP.run(launch, regions, 'cuda')
    assert float(out['out'].float().abs().max()) > 0


# ------------------------------------------------------------------------------------------------ keep_attention
def _attn(name, *, mma, B, H, Lq, Lk, D, Dv=None, mode=0, packed=False, o_ld=None, o_off=0, amax=False, in_bf16=False, flags=0, ws=True,
          T=0, seg_len=0, img_h=0, img_w=0, ksplit=0, shift=0, kv_rot=0, n_img=0, lk_rows=None, scale_mul=1.0, amp=1.0):
    """``scale_mul``: keep_attention_args.scale = scale_mul / sqrt(D); ``amp``: amplitude of v (q, k: +-1 uniform)."""
    return dict(name=name, mma=mma, B=B, H=H, Lq=Lq, Lk=Lk, D=D, Dv=D if Dv is None else Dv, mode=mode, packed=packed, o_ld=o_ld, o_off=o_off,
                amax=amax, in_bf16=in_bf16, flags=flags, ws=ws, T=T, seg_len=seg_len, img_h=img_h, img_w=img_w, ksplit=ksplit, shift=shift,
                kv_rot=kv_rot, n_img=n_img, lk_rows=lk_rows, scale_mul=scale_mul, amp=amp)


_BF = dict(scale_mul=8.0, amp=4.0)      # the bf16 class's data: peaked scores and large values, so that every optional input is felt
ATTN_CASES = [
    _attn('f32_ragged', mma=F_, B=2, H=2, Lq=250, Lk=200, D=32, o_ld=72, o_off=4),
    _attn('f32_dv', mma=F_, B=1, H=1, Lq=250, Lk=200, D=64, Dv=2),
    _attn('bf16_ragged', mma=B_, B=2, H=2, Lq=250, Lk=200, D=32, scale_mul=8.0, amp=4.0),
    _attn('bf16_in', mma=B_, B=1, H=2, Lq=250, Lk=200, D=64, in_bf16=True, scale_mul=8.0, amp=4.0),
    _attn('x3_ragged', mma=X_, B=2, H=2, Lq=250, Lk=200, D=32, amax=True, o_ld=72, o_off=4),
    _attn('x3_dv', mma=X_, B=1, H=1, Lq=250, Lk=200, D=64, Dv=2),
    _attn('x3_small_heads', mma=X_, B=3, H=8, Lq=200, Lk=250, D=64, amax=True),
    _attn('x3_no_small', mma=X_, B=1, H=8, Lq=200, Lk=250, D=64, flags=L.ATTN_NO_SMALL),
    _attn('x3_sfull_two_pass', mma=X_, B=1, H=1, Lq=256, Lk=256, D=512),
    _attn('x3_sfull2_amax', mma=X_, B=1, H=1, Lq=256, Lk=256, D=512, amax=True),
    _attn('x3_sfull2', mma=X_, B=1, H=1, Lq=256, Lk=256, D=512, flags=L.ATTN_NO_TWO_PASS),
    _attn('x3_sfull', mma=X_, B=1, H=1, Lq=256, Lk=256, D=512, flags=L.ATTN_NO_TWO_PASS | L.ATTN_NO_SFULL2),
    _attn('x3_packed_ws', mma=X_, B=1, H=1, Lq=777, Lk=300, D=128, Dv=64),
    _attn('x3_no_pack', mma=X_, B=1, H=1, Lq=777, Lk=300, D=128, Dv=64, flags=L.ATTN_NO_PACK),
    _attn('f32_mode1', mma=F_, B=3, H=2, Lq=200, Lk=400, D=32, mode=1, T=3, seg_len=200, packed=True, lk_rows=200),
    _attn('x3_mode1', mma=X_, B=3, H=2, Lq=200, Lk=400, D=32, mode=1, T=3, seg_len=200, packed=True, lk_rows=200),
    _attn('bf16_mode1', mma=B_, B=3, H=2, Lq=200, Lk=400, D=32, mode=1, T=3, seg_len=200, packed=True, lk_rows=200, scale_mul=8.0, amp=4.0),
    _attn('f32_mode2', mma=F_, B=8, H=1, Lq=24, Lk=24, D=32, mode=2, img_h=8, img_w=12, ksplit=2, shift=0, kv_rot=1, n_img=2),
    _attn('x3_mode2_shift', mma=X_, B=8, H=1, Lq=24, Lk=24, D=32, mode=2, img_h=8, img_w=12, ksplit=2, shift=2, kv_rot=1, n_img=2),
    _attn('f32_mode2_shift', mma=F_, B=8, H=1, Lq=24, Lk=24, D=32, mode=2, img_h=8, img_w=12, ksplit=2, shift=2, kv_rot=1, n_img=2),
    _attn('x3_mode2', mma=X_, B=8, H=1, Lq=24, Lk=24, D=32, mode=2, img_h=8, img_w=12, ksplit=2, shift=0, kv_rot=0, n_img=2),
    # ---- every remaining instantiation plan_attention can send a call to (tests/test_host_logic.py:
    # test_attention_table_reaches_every_instantiation asks keep_attention_plan for each case and for the whole universe)
    # exact-f32: <4,2>, <4,4> on the chunked D > 128 staging, <1,2>, <1,4> with two dv slices; four waves on shifted windows
    _attn('f32_w4_dv2', mma=F_, B=1, H=2, Lq=250, Lk=200, D=64),
    _attn('f32_w4_dv4_chunked', mma=F_, B=1, H=1, Lq=100, Lk=77, D=256, Dv=128, o_ld=136, o_off=4),
    _attn('f32_w1_dv2', mma=F_, B=3, H=2, Lq=20, Lk=50, D=48),
    _attn('f32_w1_dv4', mma=F_, B=1, H=1, Lq=20, Lk=50, D=128, Dv=160),
    _attn('f32_w4_mode2_shift', mma=F_, B=8, H=1, Lq=48, Lk=48, D=32, mode=2, img_h=12, img_w=16, ksplit=2, shift=3, kv_rot=1, n_img=2),
    # bf16 operands on fp32 inputs: the same four shapes, one wave and four waves on shifted windows
    _attn('bf16_w4_dv2', mma=B_, B=1, H=2, Lq=250, Lk=200, D=64, **_BF),
    _attn('bf16_w4_dv4_chunked', mma=B_, B=1, H=1, Lq=100, Lk=77, D=256, Dv=128, o_ld=136, o_off=4, **_BF),
    _attn('bf16_w1_dv2', mma=B_, B=3, H=2, Lq=20, Lk=50, D=48, **_BF),
    _attn('bf16_w1_dv4', mma=B_, B=1, H=1, Lq=20, Lk=50, D=128, Dv=160, **_BF),
    _attn('bf16_w1_mode2_shift', mma=B_, B=8, H=1, Lq=24, Lk=24, D=32, mode=2, img_h=8, img_w=12, ksplit=2, shift=2, kv_rot=1, n_img=2, **_BF),
    _attn('bf16_w4_mode2_shift', mma=B_, B=8, H=1, Lq=48, Lk=48, D=32, mode=2, img_h=12, img_w=16, ksplit=2, shift=3, kv_rot=1, n_img=2, **_BF),
    # bf16 inputs: <1|4, false>, the region-mask instantiation <1|2|4, true> on shifted 48-token windows, mode 1
    _attn('bf16in_dv1', mma=B_, B=1, H=2, Lq=250, Lk=200, D=32, Dv=8, in_bf16=True, **_BF),
    _attn('bf16in_dv4', mma=B_, B=1, H=1, Lq=100, Lk=77, D=128, in_bf16=True, **_BF),
    _attn('bf16in_masked_dv1', mma=B_, B=8, H=1, Lq=48, Lk=48, D=32, mode=2, img_h=12, img_w=16, ksplit=2, shift=3, kv_rot=1, n_img=2, in_bf16=True, **_BF),
    _attn('bf16in_masked_dv2', mma=B_, B=8, H=1, Lq=48, Lk=48, D=64, mode=2, img_h=12, img_w=16, ksplit=2, shift=3, kv_rot=1, n_img=2, in_bf16=True, **_BF),
    _attn('bf16in_masked_dv4', mma=B_, B=8, H=1, Lq=48, Lk=48, D=128, mode=2, img_h=12, img_w=16, ksplit=2, shift=3, kv_rot=1, n_img=2, in_bf16=True, **_BF),
    _attn('bf16in_mode1', mma=B_, B=3, H=2, Lq=100, Lk=200, D=32, mode=1, T=3, seg_len=100, lk_rows=100, in_bf16=True, **_BF),
    # x3, Q in registers (D <= 128): <4,4>, <1,2> with range probes, <1,4>; four waves on shifted windows with the window tables in LDS
    _attn('x3_nq8_w4_dv4', mma=X_, B=1, H=1, Lq=200, Lk=77, D=128),
    _attn('x3_nq8_w1_dv2', mma=X_, B=3, H=2, Lq=20, Lk=50, D=48, amax=True),
    _attn('x3_nq8_w1_dv4', mma=X_, B=1, H=1, Lq=20, Lk=50, D=128),
    _attn('x3_nq8_w4_mode2_shift', mma=X_, B=8, H=1, Lq=48, Lk=48, D=32, mode=2, img_h=12, img_w=16, ksplit=2, shift=3, kv_rot=1, n_img=2),
    # x3, D = 256 under 256 queries: 16 Q steps in registers
    _attn('x3_nq16_dv1', mma=X_, B=1, H=1, Lq=100, Lk=77, D=256, Dv=2),
    _attn('x3_nq16_dv2', mma=X_, B=1, H=2, Lq=100, Lk=77, D=256, Dv=64),
    _attn('x3_nq16_dv4_amax', mma=X_, B=2, H=1, Lq=100, Lk=77, D=256, amax=True, o_ld=264, o_off=4),
    _attn('x3_nq16_mode1', mma=X_, B=3, H=2, Lq=100, Lk=200, D=256, Dv=32, mode=1, T=3, seg_len=100, packed=True, lk_rows=100),
    _attn('x3_nq16_mode2_shift', mma=X_, B=8, H=1, Lq=48, Lk=48, D=256, Dv=64, mode=2, img_h=12, img_w=16, ksplit=2, shift=3, kv_rot=1, n_img=2),
    # x3, D >= 384 over more than 256 keys or in mode 1 / 2: Q and K re-staged per 128-wide chunk
    _attn('x3_nq0_dv1', mma=X_, B=1, H=2, Lq=40, Lk=300, D=384, Dv=32),
    _attn('x3_nq0_dv4_amax', mma=X_, B=2, H=1, Lq=40, Lk=300, D=384, amax=True, o_ld=392, o_off=4),
    _attn('x3_nq0_d512_dv2', mma=X_, B=1, H=1, Lq=40, Lk=300, D=512, Dv=64),
    _attn('x3_nq0_mode1', mma=X_, B=3, H=1, Lq=40, Lk=80, D=384, Dv=32, mode=1, T=3, seg_len=40, packed=True, lk_rows=40),
    _attn('x3_nq0_mode2_shift', mma=X_, B=8, H=1, Lq=48, Lk=48, D=384, Dv=32, mode=2, img_h=12, img_w=16, ksplit=2, shift=3, kv_rot=1, n_img=2),
    # x3 on pre-packed K / V^T (>= 256 queries, D = 128 or 256); the GMFlow product form: 270-token windows, D = Dv = 128, tables in LDS
    _attn('x3_packed_dv1', mma=X_, B=1, H=2, Lq=300, Lk=77, D=128, Dv=32),
    _attn('x3_packed_gmflow', mma=X_, B=8, H=1, Lq=270, Lk=270, D=128, mode=2, img_h=36, img_w=30, ksplit=2, shift=9, kv_rot=1, n_img=2),
    _attn('x3_packed_mode1', mma=X_, B=3, H=1, Lq=256, Lk=512, D=128, Dv=64, mode=1, T=3, seg_len=256, packed=True, lk_rows=256),
    _attn('x3_packed_d256_dv1', mma=X_, B=1, H=1, Lq=256, Lk=77, D=256, Dv=2),
    _attn('x3_packed_d256_dv2', mma=X_, B=1, H=1, Lq=300, Lk=200, D=256, Dv=64),
    _attn('x3_packed_d256_dv4_amax', mma=X_, B=2, H=1, Lq=270, Lk=77, D=256, amax=True, o_ld=264, o_off=4),
    # x3 over at most 256 keys, D >= 384: all scores of a block in LDS, ragged key and query counts
    _attn('x3_sfull_dv1', mma=X_, B=1, H=1, Lq=100, Lk=77, D=512, Dv=2),
    _attn('x3_sfull_dv2', mma=X_, B=1, H=2, Lq=100, Lk=200, D=384, Dv=64),
    _attn('x3_sfull_dv4_amax', mma=X_, B=2, H=1, Lq=100, Lk=77, D=384, amax=True),
    _attn('x3_sfull2_ragged', mma=X_, B=1, H=1, Lq=100, Lk=77, D=512, Dv=4),
    _attn('x3_small_lower_edge', mma=X_, B=1, H=2, Lq=64, Lk=33, D=64),
    # shifted windows of more than 4096 tokens: a four-wave launch WITHOUT the window tables (pixels and regions recomputed per key tile)
    _attn('x3_mode2_no_tables', mma=X_, B=4, H=1, Lq=4224, Lk=4224, D=32, mode=2, img_h=132, img_w=128, ksplit=2, shift=33, n_img=1, scale_mul=8.0),
]
# one attention step touches at most a 128-query tile of q / o and a 32-key tile of k / v rows (<= 3 * 512 floats wide here: the widest
# row is the 1096-float q | k | v row of 'x3_nq16_mode1')
ATTN_TILE_BYTES = 128 * 3 * 512 * 4


def _attn_case_args(c):
    """``args(t)``: the keep_attention_args of case ``c`` on the tensors (or made-up addresses) ``t``; and the scratch the library asks for
    with these shapes (0 for a case that passes none)."""
    B, H, Lq, Lk, D, Dv = c['B'], c['H'], c['Lq'], c['Lk'], c['D'], c['Dv']
    krows = c['lk_rows'] or Lk                                 # rows of k / v per batch in memory (mode 1: seg_len; keys come from two frames)
    if c['packed']:        # one [rows, q | k | v] buffer with 4 gap columns on either side
        assert krows == Lq
        ld = 2 * H * D + H * Dv + 8
        qs = ks = vs = (Lq * ld, ld)
    else:
        qs, ks, vs = (Lq * H * D, H * D), (krows * H * D, H * D), (krows * H * Dv, H * Dv)
    o_ld = c['o_ld'] or H * Dv
    per_b = c['ksplit'] ** 2 if c['mode'] == 2 else 1          # mode 2: [n_img, img_h * img_w, C] tensors, batch stride = image stride
    qs, ks, vs = ((s_[0] * per_b, s_[1]) for s_ in (qs, ks, vs))

    def args(t):
        a = L.AttnArgs()
        a.struct_size = ctypes.sizeof(L.AttnArgs)
        for f, val in dict(q=t['q'], k=t['k'], v=t['v'], o=t['o'], q_bs=qs[0], q_ts=qs[1], q_hs=D, k_bs=ks[0], k_ts=ks[1], k_hs=D, v_bs=vs[0],
                           v_ts=vs[1], v_hs=Dv, o_bs=Lq * o_ld * per_b, o_ts=o_ld, o_hs=Dv, B=B, H=H, Lq=Lq, Lk=Lk, D=D, Dv=Dv, scale=attn_scale(c),
                           mode=c['mode'], T=c['T'], seg_len=c['seg_len'], img_h=c['img_h'], img_w=c['img_w'], ksplit=c['ksplit'],
                           shift=c['shift'], kv_rot=c['kv_rot'], n_img=c['n_img'], mma=c['mma'], in_dtype=L.BF16 if c['in_bf16'] else L.F32,
                           q_amax=t.get('q_amax'), k_amax=t.get('k_amax'), v_amax=t.get('v_amax'), flags=c['flags']).items():
            setattr(a, f, val.data_ptr() if isinstance(val, torch.Tensor) else val)
        return a

    # the scratch the library asks for with these shapes (pointers do not enter)
    need = L.attention_workspace_bytes(args(_attn_fake(c))) if c['ws'] else 0
    return args, need


def _attn_fake(c):
    return {n_: 0x10000 for n_ in ('q', 'k', 'v', 'o') + (('q_amax', 'k_amax', 'v_amax') if c['amax'] else ())}


def attn_case_plan(case):
    """keep_attention_plan (host C) for one attention case as ``attn_case_launch`` launches it: the case's own arguments on made-up
    aligned addresses, with the workspace the case really passes."""
    args, need = _attn_case_args(case)
    a = args(_attn_fake(case))
    if need:
        a.workspace, a.workspace_bytes = 0x10000, need
    return L.attention_plan(a)


def attn_case_launch(case):
    """(regions, launch) of one attention case: the operands with their real strides, the output slice, the range maxima and the
    scratch the library asks for, embedded at exactly that size."""
    c = dict(case)
    B, H, Lq, Lk, D, Dv = c['B'], c['H'], c['Lq'], c['Lk'], c['D'], c['Dv']
    name, tb = 'at' + c['name'], ATTN_TILE_BYTES
    idt = BF16 if c['in_bf16'] else F32
    krows = c['lk_rows'] or Lk
    q, k, v = rnd(name + 'q', (B, Lq, H * D), dtype=idt), rnd(name + 'k', (B, krows, H * D), dtype=idt), rnd(name + 'v', (B, krows, H * Dv), c['amp'], dtype=idt)
    if c['packed']:        # each operand of the q | k | v buffer is nobody's surroundings
        ld = 2 * H * D + H * Dv + 8
        R = [FP.Region(B * Lq, ld, {'q': (4, H * D, q), 'k': (4 + H * D, H * D, k), 'v': (4 + 2 * H * D, H * Dv, v)}, idt, 'r', tb)]
    else:
        R = [FP.single('q', q, tile_bytes=tb), FP.single('k', k, tile_bytes=tb), FP.single('v', v, tile_bytes=tb)]
    R.append(FP.output('o', (B * Lq, H * Dv), ld=c['o_ld'] or H * Dv, off=c['o_off'], tile_bytes=tb))
    if c['amax']:
        for n_, t_ in (('q_amax', q), ('k_amax', k), ('v_amax', v)):
            R.append(FP.single(n_, t_.float().reshape(B, -1).abs().amax(1).reshape(1, B), tile_bytes=tb))
    args, need = _attn_case_args(c)
    if need:
        R.append(FP.output('ws', (1, (need + 3) // 4), tile_bytes=tb, compare=False))

    def launch(t):
        a = args(t)
        now = L.attention_workspace_bytes(a)
        assert now == need or not c['ws'], (now, need)
        if need:
            a.workspace, a.workspace_bytes = t['ws'].data_ptr(), need
        L._check(L.load().keep_attention(ctypes.byref(a), L._stream()), 'keep_attention')
        return now

    return R, launch


@pytest.mark.parametrize('case', ATTN_CASES, ids=[c['name'] for c in ATTN_CASES])
def test_attention_footprint(case):
    R, launch = attn_case_launch(case)
    out = FP.run(launch, R, 'cuda')
    assert float(out['o'].abs().max()) > 0


def test_attention_cases_reach_the_workspace_forms():
    """The table's packed-K/V case really gets a workspace from the library, and the NO_PACK twin does not (host-side query)."""
    def need(c):
        a = L.AttnArgs()
        a.struct_size = ctypes.sizeof(L.AttnArgs)
        for f in ('B', 'H', 'Lq', 'Lk', 'D', 'Dv', 'mode', 'mma', 'flags'):
            setattr(a, f, c[f])
        a.q_ts = a.k_ts = c['H'] * c['D']
        a.v_ts = a.o_ts = c['H'] * c['Dv']
        a.q_hs = a.k_hs = c['D']
        a.v_hs = a.o_hs = c['Dv']
        a.q_bs, a.k_bs, a.v_bs, a.o_bs = c['Lq'] * a.q_ts, c['Lk'] * a.k_ts, c['Lk'] * a.v_ts, c['Lq'] * a.o_ts
        return L.attention_workspace_bytes(a)
    by = {c['name']: c for c in ATTN_CASES}
    assert need(by['x3_packed_ws']) > 0 and need(by['x3_no_pack']) == 0
    assert need(by['x3_sfull_two_pass']) == 256 * 256 * 4 and need(by['x3_sfull2']) == 0


# ------------------------------------------------------------------------------------------------ the flat entry points
# Every builder states the parameters of its case ONCE, as its own arguments (constants such as the activation, eps or a threshold are
# keyword defaults): ``_k`` binds them and hands them on as the third element of the case, so the launch below and the float64
# restatement in tests/flat_ref.py read the same numbers.
def u8(name, shape):
    return (op_input('fp:' + name, shape) * 127.5 + 127.5).clamp(0, 255).to(torch.uint8)


def _call(fn, *args):
    L.call(fn, *args)


def _in(name, data, **kw):
    return FP.single(name, data, **kw)


def _k(cid, builder, *a, **kw):
    """One table case: (case id, builder thunk -> (regions, launch[, canon]), the builder's bound parameters by name)."""
    b = inspect.signature(builder).bind(*a, **kw)
    b.apply_defaults()
    return cid, (lambda: builder(*a, **kw)), dict(b.arguments)


AMAX_SLOTS, AMAX_OFF = 9, 2          # the amax arena of the flat cases: the case's N slots start at slot 2 of 9
AMAX_STALE = 3e38                    # what the case's own slots hold before a `zeroed = 0` call (the library must reset them)


def _amax_region(n, zeroed):
    return FP.Region(1, AMAX_SLOTS, {'amax': (AMAX_OFF, n, torch.zeros(1, n) if zeroed else torch.full((1, n), AMAX_STALE))}, F32, 'rw')


def _affine_act(n, hw, c, act=L.ACT_RELU):
    x = rnd('aa', (n, hw, c), 2.0)
    R = [_in('x', x), _in('s', rnd('aas', (n, c)) + 1.5), _in('h', rnd('aah', (n, c))), FP.output('o', (n * hw, c))]
    return R, lambda t: _call('keep_affine_act', t['x'], t['s'], t['h'], t['o'], n, hw, c, act)


def _gm_join(n, hw, c, with_a):
    R = [_in('a', rnd('ja', (n, hw, c))), _in('b', rnd('jb', (n, hw, c))), _in('sb', rnd('jsb', (n, c)) + 1.5), _in('hb', rnd('jhb', (n, c))),
         FP.output('o', (n * hw, c))]
    if with_a:
        R += [_in('sa', rnd('jsa', (n, c)) + 1.5), _in('ha', rnd('jha', (n, c)))]
    return R, lambda t: _call('keep_gm_join', t['a'], t.get('sa'), t.get('ha'), t['b'], t['sb'], t['hb'], t['o'], n, hw, c)


def _chan_stats(n, hw, c, ld, P):
    R = [_in('x', rnd('cs', (n * hw, c)), ld=ld), FP.output('part', (1, n * P * c * 2))]
    return R, lambda t: _call('keep_chan_stats', t['x'], t['part'], n, hw, c, ld, P)


def _norm_finalize(n, hw, c, G, P, affine, eps=1e-6):
    part = rnd('nf', (n, P, c, 2)).abs() * 3 + 1
    part[..., 1] = part[..., 1] + part[..., 0] ** 2          # sumsq >= sum^2 / count: a variance that is not negative
    R = [_in('part', part.reshape(1, -1)), FP.output('scale', (n, c)), FP.output('shift', (n, c))]
    if affine:
        R += [_in('g', rnd('nfg', (1, c)) + 1.5), _in('b', rnd('nfb', (1, c)))]
    return R, lambda t: _call('keep_norm_finalize', t['part'], t.get('g'), t.get('b'), t['scale'], t['shift'], n, hw, c, G, P, eps)


def _group_stats(n, hw, c, G, eps=1e-6, affine=True):
    R = [_in('x', rnd('gs', (n, hw, c), 2.0)), FP.output('scale', (n, c)), FP.output('shift', (n, c))]
    if affine:
        R += [_in('g', rnd('gsg', (1, c)) + 1.5), _in('b', rnd('gsb', (1, c)))]
    return R, lambda t: _call('keep_group_stats', t['x'], t.get('g'), t.get('b'), t['scale'], t['shift'], n, hw, c, G, eps)


def _norm_act_bf16(n, hw, c, in_bf16, act=L.PRO_SWISH, affine=True):
    x = rnd('nab', (n, hw, c), 2.0, BF16 if in_bf16 else F32)
    R = [_in('x', x), FP.output('o', (n * hw, c), BF16)]
    if affine:
        R += [_in('s', rnd('nabs', (n, c)) + 1.5), _in('h', rnd('nabh', (n, c)))]
    return R, lambda t: _call('keep_norm_act_bf16', t['x'], t.get('s'), t.get('h'), t['o'], n, hw, c, act, L.BF16 if in_bf16 else L.F32)


def _absmax(n, r, c, ld, zeroed=1):
    R = [_in('x', rnd('am', (n * r, c), 3.0), ld=ld), _amax_region(n, zeroed)]
    return R, lambda t: _call('keep_absmax', t['x'], t['amax'], n, r, c, ld, r * ld, zeroed)


def _layernorm(m, c, res, pos_rows, eps=1e-5):
    R = [_in('x', rnd('ln', (m, c), 2.0)), _in('g', rnd('lng', (1, c)) + 1.5), _in('b', rnd('lnb', (1, c))), FP.output('o', (m, c))]
    if res:
        R.append(_in('res', rnd('lnr', (m, c))))
    if pos_rows:
        R += [_in('pos', rnd('lnp', (pos_rows, c))), FP.output('o2', (m, c))]
    return R, lambda t: _call('keep_layernorm', t['x'], t['g'], t['b'], t.get('res'), t['o'], t.get('pos'), pos_rows, t.get('o2'), m, c, eps)


def _layernorm_amax(n, rows, c, eps=1e-5, zeroed=1):
    m = n * rows
    R = [_in('x', rnd('lna', (m, c), 2.0)), _in('g', rnd('lnag', (1, c)) + 1.5), _in('b', rnd('lnab', (1, c))), _in('res', rnd('lnar', (m, c))),
         FP.output('o', (m, c)), _amax_region(n, zeroed)]
    return R, lambda t: _call('keep_layernorm_amax', t['x'], t['g'], t['b'], t['res'], t['o'], m, c, eps, rows, t['amax'], zeroed)


def _geglu(m, f):
    R = [_in('x', rnd('gg', (m, 2 * f), 2.0)), FP.output('o', (m, f))]
    return R, lambda t: _call('keep_geglu', t['x'], t['o'], m, f)


def _geglu_amax(n, rows, f, zeroed=1):
    R = [_in('x', rnd('gga', (n * rows, 2 * f), 2.0)), FP.output('o', (n * rows, f)), _amax_region(n, zeroed)]
    return R, lambda t: _call('keep_geglu_amax', t['x'], t['o'], n, rows, f, t['amax'], zeroed)


def _argmax_gather(m, ncodes, dim):
    R = [_in('logits', rnd('ag', (m, ncodes), 4.0)), _in('cb', rnd('agc', (ncodes, dim))), FP.output('idx', (1, m), torch.int32),
         FP.output('margin', (1, m)), FP.output('o', (m, dim)),
         FP.Region(1, 5, {'status': (1, 1, torch.zeros(1, 1, dtype=torch.int32))}, torch.int32, 'rw')]
    return R, lambda t: _call('keep_argmax_gather', t['logits'], t['cb'], None, t['idx'], t['margin'], t['o'], m, ncodes, dim, t['status'])


def _nonfinite_flag(n):
    R = [_in('x', rnd('nff', (1, n))), FP.Region(1, 5, {'status': (1, 1, torch.zeros(1, 1, dtype=torch.int32))}, torch.int32, 'rw')]
    return R, lambda t: _call('keep_nonfinite_flag', t['x'], n, t['status'])


def _vq_nearest(m, ncodes, dim):
    R = [_in('z', rnd('vq', (m, dim))), _in('cb', rnd('vqc', (ncodes, dim))), FP.output('idx', (1, m), torch.int32)]
    return R, lambda t: _call('keep_vq_nearest', t['z'], t['cb'], t['idx'], m, ncodes, dim)


def _kalman(n, hw, c):
    R = [_in('a', rnd('ka', (n, hw, c))), _in('b', rnd('kb', (n, hw, c))), _in('g', rnd('kg', (n, hw)).abs()), FP.output('o', (n * hw, c))]
    return R, lambda t: _call('keep_kalman_update', t['a'], t['b'], t['g'], t['o'], n, hw, c)


def _flow_warp(n, h, w, c):
    # flow up to +-1.5 image sizes: most samples straddle or leave the border, where the zero-padding clamps live
    flow = rnd('fw', (n, h, w, 2)) * torch.tensor([1.5 * w, 1.5 * h])
    flow[0, 0, 0] = torch.tensor([-0.5, -0.5])
    flow[0, h - 1, w - 1] = torch.tensor([0.5, 0.5])
    R = [_in('x', rnd('fwx', (n * h * w, c))), _in('flow', flow.reshape(-1, 2)), FP.output('o', (n * h * w, c))]
    return R, lambda t: _call('keep_flow_warp', t['x'], t['flow'], t['o'], n, h, w, c)


def _convex_upsample(n, h, w, k):
    R = [_in('mask', rnd('cu', (n * h * w, 9 * k * k), 3.0)), _in('flow', rnd('cuf', (n * h * w, 2), 5.0)), FP.output('o', (n * k * h * k * w, 2))]
    return R, lambda t: _call('keep_convex_upsample', t['mask'], t['flow'], t['o'], n, h, w, k)


def _bilinear_upscale(planes, h, w, s):
    R = [_in('x', rnd('bu', (planes * h, w))), FP.output('o', (planes * h * s, w * s))]
    return R, lambda t: _call('keep_bilinear_upscale', t['x'], t['o'], planes, h, w, s)


def _nchw_to_nhwc(n, c, hw, mode):
    R = [_in('x', rnd('cl', (n * c, hw))), FP.output('o', (n * hw, c))]
    return R, lambda t: _call('keep_nchw_to_nhwc', t['x'], t['o'], n, c, hw, mode)


def _nhwc_to_nchw(n, c, hw):
    R = [_in('x', rnd('cf', (n * hw, c))), FP.output('o', (n * c, hw))]
    return R, lambda t: _call('keep_nhwc_to_nchw', t['x'], t['o'], n, c, hw)


def _rgb_s2d(n, h, w):
    R = [_in('x', rnd('s2d', (n * 3 * h, w))), FP.output('o', (n * (h // 2) * (w // 2), 16))]
    return R, lambda t: _call('keep_rgb_s2d', t['x'], t['o'], n, h, w)


def _add_bcast(total, tsize, alpha=-0.5):
    R = [_in('a', rnd('ab', (1, total))), _in('t', rnd('abt', (1, tsize))), FP.output('o', (1, total))]
    return R, lambda t: _call('keep_add_bcast', t['a'], t['t'], t['o'], total, tsize, alpha)


def _concat2(m, c1, c2, ld):
    R = [_in('a', rnd('c2a', (m, c1))), _in('b', rnd('c2b', (m, c2))), FP.output('o', (m, ld))]
    return R, lambda t: _call('keep_concat2', t['a'], t['b'], t['o'], m, c1, c2, ld)


def _tensor2img(npix):
    R = [_in('x', rnd('t2i', (npix, 3), 1.2)), FP.output('o', (npix, 3), torch.uint8)]
    return R, lambda t: _call('keep_tensor2img', t['x'], t['o'], npix)


def _img2tensor(npix, fn='keep_img2tensor'):
    R = [_in('x', u8('i2t', (npix, 3))), FP.output('o', (npix, 3))]
    return R, lambda t: _call(fn, t['x'], t['o'], npix)


def _comfy_to_bgr(npix):
    R = [_in('x', rnd('c2b8', (npix, 3)).abs()), FP.output('o', (npix, 3), torch.uint8)]
    return R, lambda t: _call('keep_comfy_to_bgr_u8', t['x'], t['o'], npix)


def _channel_argmax(m, c, ld):
    R = [_in('x', rnd('ca', (m, c)), ld=ld), FP.output('o', (1, m), torch.uint8)]
    return R, lambda t: _call('keep_channel_argmax', t['x'], t['o'], m, c, ld)


def _maxpool3s2(n, h, w, c):
    R = [_in('x', rnd('mp', (n * h * w, c))), FP.output('o', (n * ((h - 1) // 2 + 1) * ((w - 1) // 2 + 1), c))]
    return R, lambda t: _call('keep_maxpool3s2', t['x'], t['o'], n, h, w, c)


def _dwconv(n, h, w, c, stride, act=L.ACT_LRELU01, bias=True):
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    R = [_in('x', rnd('dw', (n * h * w, c))), _in('w', rnd('dww', (9, c))), FP.output('o', (n * ho * wo, c))]
    if bias:
        R.append(_in('b', rnd('dwb', (1, c))))
    return R, lambda t: _call('keep_dwconv3x3', t['x'], t['w'], t.get('b'), t['o'], n, h, w, c, stride, act)


def _maxpool2d(n, h, w, c, in_ld, out_ld, k, stride, pad, ceil):
    f = math.ceil if ceil else math.floor
    ho, wo = f((h + 2 * pad - k) / stride) + 1, f((w + 2 * pad - k) / stride) + 1
    R = [_in('x', rnd('m2', (n * h * w, c)), ld=in_ld, off=in_ld - c - 4 if in_ld > c + 4 else 0),
         FP.output('o', (n * ho * wo, c), ld=out_ld, off=out_ld - c if out_ld > c else 0)]
    return R, lambda t: _call('keep_maxpool2d', t['x'], t['o'], n, h, w, c, in_ld, out_ld, k, stride, pad, ho, wo)


def _slice_copy(n, h, w, c, src_ld, dst_ld, up):
    hs, ws_ = (h >> up, w >> up)
    R = [_in('src', rnd('sc', (n * hs * ws_, c)), ld=src_ld, off=src_ld - c), FP.output('dst', (n * h * w, c), ld=dst_ld, off=4)]
    return R, lambda t: _call('keep_slice_copy', t['src'], t['dst'], n, h, w, c, src_ld, dst_ld, up)


def _channel_shuffle2(rows, half, a_ld, b_ld):
    R = [_in('a', rnd('sha', (rows, half)), ld=a_ld), _in('b', rnd('shb', (rows, half)), ld=b_ld, off=b_ld - half), FP.output('o', (rows, 2 * half))]
    return R, lambda t: _call('keep_channel_shuffle2', t['a'], t['b'], t['o'], rows, half, a_ld, b_ld)


def _yolo_decode(n, ny, nx, stride=8.0, row0=5, rows_after=2):
    rows_total = row0 + 3 * ny * nx + rows_after
    R = [_in('raw', rnd('yd', (n * ny * nx, 48), 3.0)), _in('anch', rnd('yda', (1, 6)).abs() * 30 + 4),
         FP.output('pred', (n * rows_total, 16), init=torch.zeros(n * rows_total, 16))]
    return R, lambda t: _call('keep_yolo_decode', t['raw'], t['pred'], n, ny, nx, stride, t['anch'], row0, rows_total)


def _yolo_letterbox(n, h, w, rh, rw, top, left, h2, w2, swap_rb=1):
    R = [_in('x', u8('lb', (n * h * w, 3))), FP.output('o', (n * h2 * w2, 3))]
    return R, lambda t: _call('keep_yolo_letterbox_u8', t['x'], t['o'], n, h, w, rh, rw, top, left, h2, w2, swap_rb)


def _canon_dets(n, cap):
    """keep_yolo_select / keep_retina_decode append their survivors in ARRIVAL order (one atomic counter per frame; the ABI says so and
    keep_retina_nms orders them afterwards): the rows of a frame are a set.  Compared: the counts, and -- for frames whose survivors
    all fit -- the rows sorted by their last column (the unique row / anchor index).  Which rows an overflowing frame drops is
    open, so only its count is compared."""
    def canon(outs):
        cnt = outs['counts'].reshape(-1).tolist()
        d = outs['dets'].reshape(n, cap, 16)
        rows = [d[i, :c][torch.argsort(d[i, :c, 15])] if c <= cap else d[i, :0] for i, c in enumerate(cnt)]
        return {'counts': outs['counts'], 'dets': torch.cat(rows)}
    return canon


def _yolo_select(n, p, cap, thr=0.3):
    pred = rnd('ys', (n, p, 16)).abs()
    R = [_in('pred', pred.reshape(n * p, 16)), FP.output('dets', (n * cap, 16), init=torch.zeros(n * cap, 16)),
         FP.Region(1, n + 4, {'counts': (2, n, torch.zeros(1, n, dtype=torch.int32))}, torch.int32, 'rw')]
    return R, lambda t: _call('keep_yolo_select', t['pred'], t['dets'], t['counts'], n, p, cap, thr), _canon_dets(n, cap)


def _upsample_add(n, h, w, hb, wb, c):
    R = [_in('a', rnd('ua', (n * h * w, c))), _in('b', rnd('ub', (n * hb * wb, c))), FP.output('o', (n * h * w, c))]
    return R, lambda t: _call('keep_upsample_add', t['a'], t['b'], t['o'], n, h, w, hb, wb, c)


def _act_inplace(n, act):
    R = [FP.single('x', rnd('ai', (1, n), 3.0), role='rw')]
    return R, lambda t: _call('keep_act_inplace', t['x'], n, act)


def _sorted_dets(n, cap, cnt):
    """Distinct, descending-free scores and plausible boxes: dets [n, cap, 16] with cnt[i] valid rows."""
    d = rnd('nms', (n, cap, 16)).abs() * 40
    d[..., 2:4] = d[..., 0:2] + 10 + rnd('nmsw', (n, cap, 2)).abs() * 30
    d[..., 4] = torch.linspace(0.05, 0.95, n * cap)[torch.from_numpy(np.random.RandomState(0).permutation(n * cap))].reshape(n, cap)
    d[..., 15] = torch.arange(cap, dtype=torch.float32)
    return d


def _retina_nms(n, cap, cnt, ordered, iou=0.4):
    d = _sorted_dets(n, cap, cnt)
    counts = torch.tensor([cnt], dtype=torch.int32).repeat(1, n)
    counts[0, -1] = max(cnt - 3, 0)
    R = [_in('dets', d.reshape(n * cap, 16)), _in('counts', counts), FP.output('o', (n * cap, 16), init=torch.zeros(n * cap, 16)),
         FP.output('oc', (1, n), torch.int32)]
    if ordered:
        # ranks 0 .. counts[n] must name valid rows: order the valid rows only
        order = torch.stack([torch.argsort(torch.where(torch.arange(cap) < int(counts[0, i]), d[i, :, 4], torch.tensor(-1.0)),
                                           descending=True).to(torch.int32) for i in range(n)])
        R.append(_in('order', order.reshape(n, cap)))
        return R, lambda t: _call('keep_retina_nms_ordered', t['dets'], t['counts'], t['order'], t['o'], t['oc'], n, cap, iou)
    return R, lambda t: _call('keep_retina_nms', t['dets'], t['counts'], t['o'], t['oc'], n, cap, iou)


def _retina_decode(n, p, cap, var0=0.1, var1=0.2, sx=640.0, sy=480.0, thr=0.5):
    R = [_in('heads', rnd('rd', (n * p, 32), 2.0)), _in('priors', rnd('rdp', (2 * p, 4)).abs() * 0.5 + 0.05),
         FP.output('dets', (n * cap, 16), init=torch.zeros(n * cap, 16)),
         FP.Region(1, n + 4, {'counts': (2, n, torch.zeros(1, n, dtype=torch.int32))}, torch.int32, 'rw')]
    return R, lambda t: _call('keep_retina_decode', t['heads'], t['priors'], t['dets'], t['counts'], n, p, cap, var0, var1, sx, sy, thr), _canon_dets(n, cap)


def _gauss(ntap):
    x = torch.arange(ntap, dtype=torch.float32) - ntap // 2
    k = torch.exp(-x * x / (2 * (0.3 * ((ntap - 1) * 0.5 - 1) + 0.8) ** 2))
    return (k / k.sum()).reshape(1, ntap)


def _sep_filter(n, h, w, ntap, classes):
    R = [_in('kern', _gauss(ntap)), FP.output('tmp', (n * h, w), compare=False), FP.output('dst', (n * h, w))]
    if classes:
        R += [_in('cls', (u8('sfc', (n * h, w)) % 19)), _in('lut', rnd('sfl', (1, 19)).abs() * 255)]
        return R, lambda t: _call('keep_sep_filter', None, t['cls'], t['lut'], t['tmp'], t['dst'], n, h, w, t['kern'], ntap)
    R.append(_in('src', rnd('sfs', (n * h, w)).abs() * 255))
    return R, lambda t: _call('keep_sep_filter', t['src'], None, None, t['tmp'], t['dst'], n, h, w, t['kern'], ntap)


def _u8_to_f32(n):
    R = [_in('x', u8('u2f', (1, n))), FP.output('o', (1, n))]
    return R, lambda t: _call('keep_u8_to_f32', t['x'], t['o'], n)


def _f32_round_u8(n):
    R = [_in('x', rnd('f2u', (1, n), 300.0)), FP.output('o', (1, n), torch.uint8)]
    return R, lambda t: _call('keep_f32_round_u8', t['x'], t['o'], n)


def _d2s(m):
    return (ctypes.c_double * 6)(*m)


# destination -> source maps: a rotation + scale whose source window hangs over the frame edge on two sides
_HANG = (0.93, -0.37, -6.3, 0.37, 0.93, -4.8)


def _warp_affine(h, w, dh, dw, m, border=(135, 133, 132)):
    R = [_in('src', u8('wa', (h * w, 3))), FP.output('dst', (dh * dw, 3), torch.uint8)]
    return R, lambda t: _call('keep_warp_affine_u8', t['src'], h, w, t['dst'], dh, dw, _d2s(m), *border)


def _warp_ones(h, w, fh, fw, m):
    R = [FP.output('dst', (h, w))]
    return R, lambda t: _call('keep_warp_ones', t['dst'], h, w, fh, fw, _d2s(m))


def _erode(h, w, k):
    R = [_in('src', (rnd('er', (h, w)) > -0.6).float()), FP.output('tmp', (h, w), compare=False), FP.output('dst', (h, w))]
    return R, lambda t: _call('keep_erode_rect', t['src'], t['tmp'], t['dst'], h, w, k)


def _draw_box(h, w, fh, fw, m, box, thickness=2):
    R = [FP.single('frame', u8('db', (h * w, 3)), role='rw')]
    return R, lambda t: _call('keep_draw_box', t['frame'], h, w, fh, fw, thickness, _d2s(m), *box)


def _paste_face(h, w, fh, fw, m, box, frame_mask, mask_border=3):
    R = [FP.single('frame', rnd('pf', (h * w, 3)).abs() * 255, role='rw'), _in('face', u8('pff', (fh * fw, 3)))]
    if frame_mask:      # a soft mask already in frame space [H, W]
        R.append(_in('mask', rnd('pfm', (h, w)).abs()))
    else:
        R.append(_in('mask', rnd('pfm', (fh, fw)).abs() * 255))
    return R, lambda t: _call('keep_paste_face', t['frame'], h, w, t['face'], t['mask'], fh, fw, _d2s(m), *box, -1 if frame_mask else mask_border)


def _lanczos(n, h, w, h2, w2, unaligned=False):
    lib = L.load(check_device=False)

    def table(S, D):
        ofs, coef = np.zeros(D, np.int32), np.zeros(D * 8, np.int16)
        assert lib.keep_lanczos4_tables(S, D, ofs.ctypes.data, coef.ctypes.data) == 0
        return torch.from_numpy(ofs).reshape(1, D), torch.from_numpy(coef).reshape(D, 8)
    (xo, xc), (yo, yc) = table(w, w2), table(h, h2)
    src = u8('lz', (n * h * w, 3))
    R = FP.unaligned_u8(src, n * h2 * w2 * 3) if unaligned else [_in('src', src), FP.output('dst', (n * h2 * w2, 3), torch.uint8)]
    R += [_in('xo', xo), _in('xc', xc), _in('yo', yo), _in('yc', yc)]

    def launch(t):
        assert (t['src'].data_ptr() % 16, t['dst'].data_ptr() % 16) == ((5, 11) if unaligned else (0, 0))
        _call('keep_resize_lanczos4_u8', t['src'], t['dst'], n, h, w, h2, w2, t['xo'], t['xc'], t['yo'], t['yc'])
    return R, launch


def _token_linear(m, n_out, out_bf16, k=128, bias=True):
    R = [_in('x', rnd('tl', (m, k))), _in('w', rnd('tlw', (n_out, k), 0.1, BF16)), FP.output('o', (m, n_out), BF16 if out_bf16 else F32)]
    if bias:
        R.append(_in('b', rnd('tlb', (1, n_out))))
    return R, lambda t: _call('keep_token_linear', t['x'], t['w'], t.get('b'), t['o'], m, k, n_out, L.BF16 if out_bf16 else L.F32)


def _gm_mlp(m, c=128):
    C = c
    R = [_in('a', rnd('ma', (m, C))), _in('b', rnd('mb', (m, C))), _in('w0', rnd('mw0', (8 * C, 2 * C), 0.05, BF16)),
         _in('w2', rnd('mw2', (C, 8 * C), 0.05, BF16)), FP.output('o', (m, C))]
    return R, lambda t: _call('keep_gm_mlp', t['a'], t['b'], t['w0'], t['w2'], t['o'], m, C)


def gm_ffn_weights(hidden, c=128):
    """The plain fp32 weights W0 [hidden, 2C] / W2 [C, hidden] the keep_gm_ffn_x3 cases split into fp16 halves (the reference reads these)."""
    return rnd('fw0', (hidden, 2 * c), 0.05), rnd('fw2', (c, hidden), 0.05)


def _gm_ffn_x3(m, hidden, c=128, eps=1e-5, exact_act=0):
    C = c
    w0, w2 = gm_ffn_weights(hidden, C)
    w2 = ops.ffn_w2_perm(w2)
    s0, s2 = ops.x3_scale_for(float(w0.abs().max())), ops.x3_scale_for(float(w2.abs().max()))
    w0x, w2x = ops.split_x3(w0, s0), ops.split_x3(w2, s2)
    R = [_in('src', rnd('fs', (m, C))), _in('msg', rnd('fm', (m, C))), _in('w0', w0x.reshape(hidden, -1)), _in('w2', w2x.reshape(C, -1)),
         _in('g', rnd('fg', (1, C)) * 0.2 + 1), _in('b', rnd('fb', (1, C)) * 0.2), FP.output('o', (m, C))]
    return R, lambda t: _call('keep_gm_ffn_x3', t['src'], t['msg'], t['w0'], 1.0 / s0, t['w2'], 1.0 / s2, t['g'], t['b'], eps, t['o'], m, C, hidden, exact_act)


# entry point -> [(case id, builder thunk, parameters)]: one aligned and one ragged size each (element counts that are no multiple of 4,
# odd H / W, C off the vector width where the ABI allows it, M off the block), border-crossing geometry for the samplers.  The values
# of every case are judged by tests/test_gpu_flat_values.py against tests/flat_ref.py.
#
# Branches of the launchers (csrc/keep_ops.hip, csrc/keep_paste.hip) and the case that reaches each:
#   keep_chan_stats    one `cbase` pass, several pixels per pass (C = 64: 4 rows)      -> aligned
#                      C < 256 not dividing 256 (C = 6: 42 rows, idle lanes)           -> ragged
#                      two `cbase` passes, the second 64 wide (C = 320)                -> c320
#                      P not dividing HW (35 pixels in 4 chunks of 9, 9, 9, 8)         -> p_ragged
#   keep_layernorm     layernorm_kernel, C % 4 == 0                                    -> aligned (M = 64 < 4096), ragged (C = 36)
#                      layernorm128_kernel (C == 128, M >= 4096), ragged last block    -> c128_stream
#   keep_absmax        dense rows (ld == C)                                            -> aligned
#                      scalar channel slice (C % 4 != 0, ld > C)                       -> ragged
#                      vectorised channel slice (C % 4 == 0, ld > C); 300 float4s per image,
#                      so the (row, column) walk takes a second step that wraps the column  -> slice_vec4
#                      absmax_zero_kernel (zeroed = 0)                                 -> unzeroed
#   keep_layernorm_amax / keep_geglu_amax   the library's own zero-fill (zeroed = 0)   -> unzeroed
#   keep_group_stats   scalar form (C / G = 2) -> aligned; float4 form (C / G = 4) -> ragged; NULL gamma / beta, one channel per group -> instance_no_affine
#   keep_norm_act_bf16 float32 input, swish -> aligned; bf16 input -> ragged_bf16in; NULL scale / shift (plain cast), no activation -> cast_only;
#                      ReLU -> relu_bf16in
#   keep_layernorm_amax  one atomic per block (its four rows in one image) -> aligned; per wave (a block across two images, rows beyond M) -> ragged
#   keep_comfy_to_bgr_u8  four-pixel body -> aligned; body + three-pixel tail -> ragged; tail without a body -> tail_only
#   keep_token_linear  N = 128 -> aligned; N = 384, bf16 output -> ragged_bf16out; N = 256, NULL bias, M below one tile -> n256_no_bias
#   keep_affine_act / keep_gm_join   float4 form (C % 4 == 0) -> aligned; scalar form (C = 6) -> ragged
#   keep_act_inplace   float4 body -> aligned (ReLU); float4 body + scalar tail is not reachable (n % 4 == 0 is required): the ragged case
#                      has 195 float4s, no multiple of the block; the exp-based SiLU -> ragged; erff GELU -> gelu; leaky 0.1 -> lrelu01
#   keep_sep_filter    float source, 5 taps -> float; class map through the LUT, 9 taps wider than the 5 x 7 image -> classes_ragged
#   keep_dwconv3x3     stride 1 -> aligned; stride 2 on an odd map -> ragged_s2; no bias, no activation -> no_bias
#   keep_yolo_select / keep_retina_decode   every frame fits -> aligned; a fitting frame beside overflowing ones -> ragged_overflow
# caps of the two compacting selectors: `aligned` holds every frame's survivors, `ragged_overflow` holds those of at least one frame and
# overflows on another (tests/test_host_logic.py asserts both from the float64 reference)
YS_CAP_ALIGNED, YS_CAP_RAGGED, RD_CAP_ALIGNED, RD_CAP_RAGGED = 128, 8, 512, 33
FLAT_CASES = {
    'keep_chan_stats': [_k('aligned', _chan_stats, 2, 256, 64, 64, 4), _k('ragged', _chan_stats, 3, 35, 6, 9, 2), _k('c320', _chan_stats, 2, 40, 320, 320, 2),
                        _k('p_ragged', _chan_stats, 3, 35, 6, 9, 4)],
    'keep_norm_finalize': [_k('gn32', _norm_finalize, 2, 256, 64, 32, 4, True), _k('in', _norm_finalize, 3, 35, 6, 6, 2, False)],
    'keep_group_stats': [_k('aligned', _group_stats, 2, 64, 64, 32), _k('ragged', _group_stats, 3, 35, 12, 3),
                         _k('instance_no_affine', _group_stats, 3, 35, 12, 12, eps=1e-5, affine=False)],
    'keep_affine_act': [_k('aligned', _affine_act, 2, 64, 32), _k('ragged', _affine_act, 3, 35, 6)],
    'keep_norm_act_bf16': [_k('aligned', _norm_act_bf16, 2, 64, 32, False), _k('ragged_bf16in', _norm_act_bf16, 3, 35, 8, True),
                           _k('cast_only', _norm_act_bf16, 3, 35, 8, False, act=L.PRO_NONE, affine=False), _k('relu_bf16in', _norm_act_bf16, 3, 35, 8, True, act=L.PRO_RELU)],
    'keep_gm_mlp': [_k('aligned', _gm_mlp, 256), _k('ragged', _gm_mlp, 300)],
    'keep_gm_ffn_x3': [_k('aligned', _gm_ffn_x3, 256, 256), _k('ragged', _gm_ffn_x3, 777, 96)],
    'keep_token_linear': [_k('aligned', _token_linear, 256, 128, False), _k('ragged_bf16out', _token_linear, 777, 384, True),
                          _k('n256_no_bias', _token_linear, 35, 256, False, bias=False)],
    'keep_gm_join': [_k('aligned', _gm_join, 2, 64, 32, True), _k('ragged_identity', _gm_join, 3, 35, 6, False)],
    'keep_absmax': [_k('aligned', _absmax, 2, 64, 32, 32), _k('ragged', _absmax, 3, 35, 6, 9), _k('slice_vec4', _absmax, 3, 100, 12, 20),
                    _k('unzeroed', _absmax, 3, 35, 6, 9, zeroed=0)],
    'keep_layernorm': [_k('aligned', _layernorm, 64, 128, True, 16), _k('ragged', _layernorm, 35, 36, False, 0),
                       _k('c128_stream', _layernorm, 4099, 128, True, 0)],
    'keep_geglu': [_k('aligned', _geglu, 64, 128), _k('ragged', _geglu, 35, 20)],
    'keep_layernorm_amax': [_k('aligned', _layernorm_amax, 2, 64, 128), _k('ragged', _layernorm_amax, 3, 35, 36),
                            _k('unzeroed', _layernorm_amax, 3, 35, 36, zeroed=0)],
    'keep_geglu_amax': [_k('aligned', _geglu_amax, 2, 64, 128), _k('ragged', _geglu_amax, 3, 35, 20), _k('unzeroed', _geglu_amax, 3, 35, 20, zeroed=0)],
    'keep_argmax_gather': [_k('aligned', _argmax_gather, 64, 1024, 256), _k('ragged', _argmax_gather, 35, 1024, 256)],
    'keep_nonfinite_flag': [_k('aligned', _nonfinite_flag, 4096), _k('ragged', _nonfinite_flag, 777)],
    'keep_vq_nearest': [_k('aligned', _vq_nearest, 64, 1024, 256), _k('ragged', _vq_nearest, 35, 1024, 256)],
    'keep_kalman_update': [_k('aligned', _kalman, 2, 64, 32), _k('ragged', _kalman, 3, 35, 6)],
    'keep_flow_warp': [_k('aligned', _flow_warp, 2, 8, 16, 4), _k('ragged_3ch', _flow_warp, 3, 5, 7, 3), _k('one_pixel', _flow_warp, 1, 1, 1, 3)],
    'keep_convex_upsample': [_k('aligned', _convex_upsample, 2, 8, 8, 4), _k('ragged', _convex_upsample, 3, 5, 7, 8)],
    'keep_bilinear_upscale': [_k('aligned', _bilinear_upscale, 3, 8, 8, 4), _k('ragged', _bilinear_upscale, 9, 5, 7, 4)],
    'keep_nchw_to_nhwc': [_k('aligned', _nchw_to_nhwc, 2, 16, 64, 0), _k('ragged_gm', _nchw_to_nhwc, 3, 3, 35, 1)],
    'keep_rgb_s2d': [_k('aligned', _rgb_s2d, 2, 16, 16), _k('ragged', _rgb_s2d, 3, 10, 14)],
    'keep_nhwc_to_nchw': [_k('aligned', _nhwc_to_nchw, 2, 32, 64), _k('ragged', _nhwc_to_nchw, 3, 3, 35)],
    'keep_add_bcast': [_k('aligned', _add_bcast, 4096, 256), _k('ragged', _add_bcast, 777, 37)],
    'keep_concat2': [_k('aligned', _concat2, 64, 128, 2, 144), _k('ragged', _concat2, 35, 5, 2, 9)],
    'keep_tensor2img': [_k('aligned', _tensor2img, 256), _k('ragged', _tensor2img, 35)],
    'keep_img2tensor': [_k('aligned', _img2tensor, 256), _k('ragged', _img2tensor, 35)],
    'keep_bgr_u8_to_comfy': [_k('aligned', _img2tensor, 256, 'keep_bgr_u8_to_comfy'), _k('ragged', _img2tensor, 35, 'keep_bgr_u8_to_comfy')],
    'keep_comfy_to_bgr_u8': [_k('aligned', _comfy_to_bgr, 256), _k('ragged', _comfy_to_bgr, 35), _k('tail_only', _comfy_to_bgr, 3)],
    'keep_channel_argmax': [_k('aligned', _channel_argmax, 256, 19, 32), _k('ragged', _channel_argmax, 35, 19, 19)],
    'keep_maxpool3s2': [_k('aligned', _maxpool3s2, 2, 8, 8, 64), _k('ragged', _maxpool3s2, 3, 5, 7, 12)],
    'keep_dwconv3x3': [_k('aligned', _dwconv, 2, 8, 8, 32, 1), _k('ragged_s2', _dwconv, 3, 5, 7, 12, 2),
                       _k('no_bias', _dwconv, 1, 5, 7, 4, 1, act=L.ACT_NONE, bias=False)],
    'keep_retina_nms': [_k('aligned', _retina_nms, 2, 64, 64, False), _k('ragged', _retina_nms, 3, 50, 37, False)],
    'keep_retina_nms_ordered': [_k('aligned', _retina_nms, 2, 64, 64, True), _k('ragged', _retina_nms, 3, 50, 37, True)],
    'keep_maxpool2d': [_k('stem_ceil', _maxpool2d, 3, 5, 7, 8, 8, 16, 2, 2, 0, True), _k('spp', _maxpool2d, 1, 5, 7, 4, 16, 16, 5, 1, 2, False)],
    'keep_slice_copy': [_k('aligned', _slice_copy, 2, 8, 8, 32, 32, 64, 0), _k('ragged_up', _slice_copy, 3, 10, 14, 4, 12, 24, 1)],
    'keep_channel_shuffle2': [_k('aligned', _channel_shuffle2, 64, 32, 64, 32), _k('ragged', _channel_shuffle2, 35, 4, 12, 12)],
    'keep_yolo_decode': [_k('aligned', _yolo_decode, 2, 8, 8), _k('ragged', _yolo_decode, 3, 5, 7)],
    'keep_yolo_letterbox_u8': [_k('resize', _yolo_letterbox, 2, 20, 30, 16, 24, 4, 4, 24, 32), _k('copy_ragged', _yolo_letterbox, 3, 5, 7, 5, 7, 1, 0, 7, 7),
                               _k('one_pixel', _yolo_letterbox, 1, 9, 11, 1, 1, 0, 0, 1, 1)],
    'keep_yolo_select': [_k('aligned', _yolo_select, 2, 256, YS_CAP_ALIGNED), _k('ragged_overflow', _yolo_select, 3, 35, YS_CAP_RAGGED)],
    'keep_upsample_add': [_k('aligned', _upsample_add, 2, 10, 14, 5, 7, 64), _k('ragged', _upsample_add, 3, 9, 13, 5, 7, 12)],
    'keep_act_inplace': [_k('aligned', _act_inplace, 4096, L.ACT_RELU), _k('ragged', _act_inplace, 780, L.ACT_SILU), _k('gelu', _act_inplace, 780, L.ACT_GELU),
                         _k('lrelu01', _act_inplace, 780, L.ACT_LRELU01)],
    'keep_retina_decode': [_k('aligned', _retina_decode, 2, 256, RD_CAP_ALIGNED), _k('ragged_overflow', _retina_decode, 3, 35, RD_CAP_RAGGED)],
    'keep_sep_filter': [_k('float', _sep_filter, 2, 16, 16, 5, False), _k('classes_ragged', _sep_filter, 3, 5, 7, 9, True)],
    'keep_u8_to_f32': [_k('aligned', _u8_to_f32, 4096), _k('ragged', _u8_to_f32, 777)],
    'keep_f32_round_u8': [_k('aligned', _f32_round_u8, 4096), _k('ragged', _f32_round_u8, 777)],
    'keep_warp_affine_u8': [_k('inside', _warp_affine, 16, 16, 8, 8, (1, 0, 2.5, 0, 1, 3.25)), _k('hangs_over', _warp_affine, 13, 17, 11, 9, _HANG),
                            _k('one_pixel', _warp_affine, 5, 7, 1, 1, (1, 0, 6.5, 0, 1, 4.5))],
    'keep_warp_ones': [_k('inside', _warp_ones, 16, 16, 8, 8, (1, 0, -2.5, 0, 1, -3.25)), _k('off_frame', _warp_ones, 13, 17, 11, 9, _HANG)],
    'keep_draw_box': [_k('inside', _draw_box, 16, 16, 8, 8, (1, 0, -2.5, 0, 1, -3.25), (2, 3, 12, 13)),
                      _k('edge', _draw_box, 13, 17, 11, 9, _HANG, (0, 0, 17, 13))],
    'keep_erode_rect': [_k('aligned', _erode, 16, 16, 3), _k('k_larger_than_image', _erode, 5, 7, 9)],
    'keep_paste_face': [_k('inside', _paste_face, 16, 16, 8, 8, (1, 0, -2.5, 0, 1, -3.25), (2, 3, 12, 13), False),
                        _k('over_the_edge', _paste_face, 13, 17, 11, 9, _HANG, (0, 0, 17, 13), False),
                        _k('frame_mask', _paste_face, 13, 17, 11, 9, _HANG, (5, 0, 17, 9), True)],
    'keep_resize_lanczos4_u8': [_k('up', _lanczos, 2, 8, 8, 16, 16), _k('ragged', _lanczos, 3, 5, 7, 3, 100), _k('one_pixel', _lanczos, 1, 5, 7, 1, 1),
                                _k('unaligned', _lanczos, 3, 5, 7, 3, 100, unaligned=True)],
}
# launchers the convolution / attention tables above cover
STRUCT_LAUNCHERS = {'keep_conv2d': CONV_CASES, 'keep_attention': ATTN_CASES}
# entry points of include/keep_hip.h that launch nothing (host-only C)
HOST_ONLY = {'keep_abi_version', 'keep_last_error', 'keep_device_ok', 'keep_sizeof_conv2d_args', 'keep_sizeof_attention_args',
             'keep_conv2d_plan', 'keep_attention_workspace_bytes', 'keep_lanczos4_tables'}


def flat_case(fn, cid):
    """(regions, launch, canon or None, parameters) of one flat case."""
    builder, params = {c: (b, p) for c, b, p in FLAT_CASES[fn]}[cid]
    regions, launch, *canon = builder()
    return regions, launch, (canon[0] if canon else None), params


@pytest.mark.parametrize('fn,case', [(fn, cid) for fn, cases in FLAT_CASES.items() for cid, _, _ in cases])
def test_flat_op_footprint(fn, case):
    regions, launch, canon, _ = flat_case(fn, case)
    # outputs the kernel legitimately leaves partly unwritten (rows beyond a count) were given an initial value; everything else
    # must come out finite
    FP.run(launch, regions, 'cuda', canon=canon)
