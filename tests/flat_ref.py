"""Plain restatements of the flat ``keep_*`` entry points of include/keep_hip.h and the judge that compares one launch of a
footprint-table case (tests/test_gpu_footprint.py: FLAT_CASES) with them.  torch / numpy on the CPU only: no GPU, no library.
tests/test_gpu_flat_values.py feeds the judge device outputs; tests/test_host_logic.py feeds it doctored references (it must bite) and
checks that every optional input of every case moves the reference by far more than the tolerance.

A reference is computed from the case's PAYLOAD tensors (name -> [rows, C] tensor, as the table put them into the strided buffers) and
the case's parameters (the builder's own arguments, handed on by the table), and restates the ABI text, not the kernel.  It returns
``{output name: spec}``; a spec is one of

    exact(ref)               bit for bit (``ref`` in the output's dtype)
    arith(ref64, tol)        err = max |out - ref| <= tol * scale, scale = max(1, max |ref|)   (abi_ref.measure)
    arith(ref64, None, r32)  no tolerance of its own: tol * scale = max(8 * err32, 2^-22 * scale), err32 = the error of the SAME restatement
                             evaluated in float32 on the CPU (``r32``); 8 covers another summation order and the device's expf / erff
    bf16(ref64)              against the RNE bf16 rounding of the reference, one bf16 ulp at scale (2^-8 * scale)
    stats(...)               statistics partials summed over P against the float64 sums, bound HW * 2^-24 * sum |x| (resp. sum x^2)
    amax(of, n)              every slot bit-equal to max |.| of the DEVICE's own output `of` (keep_absmax: of the input); the other
                             slots of the 9-slot arena still hold what they held
    argmin(d)                idx == float64 arg-min on every row whose margin exceeds 1e-5 * max |d|; at most 1 % of the rows left out
    dets(...)                counts exact; the surviving set (last column) equal for every score farther than 1e-6 from the threshold;
                             rows of fitting frames sorted by the last column, in the arith class

Classes, tolerances and where they come from (tests named are in tests/test_gpu_kernels.py unless another module is given; "measured":
max over the table's cases of the float32-restatement error and the bound max(8 x err32, 2^-22 x scale) it gives, taken on the CPU):

    entry point               class        tolerance        source
    keep_chan_stats           reduction    HW 2^-24 sum|x|  abi_ref.judge_conv (statistics rule)
    keep_norm_finalize        reduction    2e-4             test_chan_stats_and_norm_finalize_on_their_own_output (check's default)
    keep_group_stats          reduction    2e-5             test_group_stats_small_matches_two_pass
    keep_affine_act           f32-arith    2e-4             test_affine_act_and_gm_join (check's default)
    keep_gm_join              f32-arith    2e-4             test_affine_act_and_gm_join
    keep_norm_act_bf16        bf16         2^-8             abi_ref: one bf16 ulp at scale against RNE(reference)
    keep_gm_mlp               matrix       2e-3             test_gm_mlp_fused_matches_two_gemms (bf16 operands, bf16 hidden activations)
    keep_gm_ffn_x3            matrix       2e-5             test_gm_ffn_x3_fused_kernel (unrounded operands)
    keep_token_linear         matrix       2e-5 (+2^-8)     test_token_linear_streaming_gemm; bf16 output: abi_ref's one ulp at scale
    keep_absmax               exact/amax   bits             test_absmax_paths
    keep_layernorm            reduction    2e-5             test_layernorm_variants
    keep_layernorm_amax       reduction    2e-5 + amax      test_layernorm_variants, test_layernorm_and_geglu_with_fused_range_maxima
    keep_geglu                f32-arith    1e-5             test_geglu_concat_addbcast
    keep_geglu_amax           f32-arith    1e-5 + amax      the same
    keep_argmax_gather        exact        bits; margin 1e-6   test_argmax_gather_and_ties
    keep_nonfinite_flag       exact        bits             test_argmax_never_launders_non_finite_logits
    keep_vq_nearest           index        margin 1e-5 max|d|, <= 1 % left out   test_vq_nearest_at_scale_ragged_and_ties
    keep_kalman_update        f32-arith    1e-6             test_kalman_update_and_flow_warp
    keep_flow_warp            f32-arith    1e-5             test_kalman_update_and_flow_warp (oracle/keep_oracle.py:flow_warp in float64)
    keep_convex_upsample      f32-arith    1e-5             test_convex_upsample_and_layouts
    keep_bilinear_upscale     f32-arith    1e-6             test_bilinear_upscale_matches_torch
    keep_nchw_to_nhwc         exact (mode 0) / f32-arith 1e-6 (mode 1)   test_convex_upsample_and_layouts
    keep_rgb_s2d              f32-arith    1e-6             mode 1's tolerance (test_rgb_s2d_... demands the bits of mode 1's output)
    keep_nhwc_to_nchw         exact        bits             test_nhwc_to_nchw_is_a_permutation
    keep_add_bcast            f32-arith    measured         err32 3.0e-08 at scale 1.5, bound 3.5e-07 (2^-22 x scale; test_geglu_concat_addbcast has torch.allclose's default only)
    keep_concat2              exact        bits             test_geglu_concat_addbcast
    keep_tensor2img           exact        bits             test_tensor2img_img2tensor_bit_exact (oracle/converters_oracle.py)
    keep_img2tensor           exact        bits             the same
    keep_bgr_u8_to_comfy      exact        bits             test_bgr_u8_to_comfy_equals_the_host_converter_on_every_value
    keep_comfy_to_bgr_u8      exact        bits             test_comfy_to_bgr_u8_equals_the_host_converter_on_every_boundary
    keep_channel_argmax       exact        bits             ABI: lowest index on ties
    keep_maxpool3s2           exact        bits             test_maxpool3s2_is_max_pool2d_3_2_1
    keep_dwconv3x3            f32-arith    2e-6             test_gpu_facelib.py: test_dwconv3x3_vs_torch_grouped_convolution
    keep_retina_nms           exact        bits             test_gpu_facelib.py: test_retina_decode_on_the_device_equals_the_host_decoder
    keep_retina_nms_ordered   exact        bits             test_gpu_facelib.py: test_retina_tied_frames_...
    keep_maxpool2d            exact        bits             test_gpu_facelib.py: test_yolo_helper_kernels_vs_torch
    keep_slice_copy           exact        bits             the same
    keep_channel_shuffle2     exact        bits             the same
    keep_yolo_decode          f32-arith    2e-5             the same
    keep_yolo_letterbox_u8    exact        bits             test_gpu_facelib.py: test_yolo_letterbox_kernel_vs_oracle (oracle/facelib_oracle.py)
    keep_yolo_select          dets         measured         err32 3.0e-08 (single float32 operations) at scale 254 (the row-index column), bound 6.1e-05 (2^-22 x scale)
    keep_upsample_add         exact        bits (float32)   test_upsample_add_is_nearest_interpolate_plus_add
    keep_act_inplace          exact (ReLU, leaky) / f32-arith 2e-4 (GELU, sigmoid, SiLU)   test_act_inplace_every_activation
    keep_retina_decode        dets         measured         err32 4.7e-05 at scale 520 / 4.5e-05 at scale 633, bound 3.7e-04 / 3.6e-04 (8 x err32)
    keep_sep_filter           exact        bits             test_gpu_paste.py: test_parse_mask_blur_is_bit_exact (oracle/paste_oracle.py:sep_filter_f32)
    keep_u8_to_f32            exact        bits             test_u8_to_f32_and_f32_round_u8_every_value
    keep_f32_round_u8         exact        bits             the same
    keep_warp_affine_u8       exact        bits             test_gpu_paste.py: test_crop_warp_align_warp_face_is_bit_exact
    keep_warp_ones            exact        bits             test_warp_ones_and_erode_rect_on_their_own (the existing test demands bits)
    keep_draw_box             exact        bits             test_gpu_paste.py (paste_faces with draw_box)
    keep_erode_rect           exact        bits             test_warp_ones_and_erode_rect_on_their_own
    keep_paste_face           exact        bits             test_gpu_paste.py: test_paste_small_frame_and_upscaled_matrix (the paste tests demand bits)
    keep_resize_lanczos4_u8   exact        bits             test_gpu_upscale_factor.py / tests/cv_lanczos_ref.py

keep_sep_filter, keep_warp_ones and keep_paste_face are short float32 chains whose order oracle/paste_oracle.py fixes operation by
operation and whose existing tests demand bits; they are judged bit for bit here too.  Buffers declared ``compare=False`` (tmp) are not
outputs and are not judged.
"""
import contextlib
import math

import numpy as np
import torch
import torch.nn.functional as F

import converters_oracle as CO
import cv_lanczos_ref as LZ
import facelib_oracle as FO
import keep_oracle as O
import paste_oracle as PO
from abi_ref import ACT_LRELU01, ACT_LRELU02, ACT_NONE, ACT_RELU, BF16_ULP, PRO_NONE, SENSITIVITY, _act, _act_pro, bf16r, measure  # noqa: F401

F64, F32 = torch.float64, torch.float32
KEEP_F32, KEEP_BF16 = 0, 1                      # hiplib.F32 / hiplib.BF16 (tests/test_host_logic.py compares)
AMAX_SLOTS, AMAX_OFF, AMAX_MARK = 9, 2, 5.5     # the arena of the flat amax cases; what the plain run puts into the neighbouring slots
VQ_MARGIN, VQ_MAX_SKIPPED = 1e-5, 0.01
THRESHOLD_BAND = 1e-6
MEASURED_FACTOR, MEASURED_FLOOR = 8.0, 2.0 ** -22


def payloads(regions, fn=None, params=None):
    """name -> payload tensor of every region that has one (the data the table put into the strided buffers), as [rows, C].  keep_gm_ffn_x3
    is handed split-fp16 weight images; its reference reads the plain weights they were made from (``w0_plain`` / ``w2_plain``)."""
    t = {n: d.reshape(r.rows, C) for r in regions for n, (_, C, d) in r.windows.items() if d is not None}
    if fn == 'keep_gm_ffn_x3':
        import test_gpu_footprint as T
        t['w0_plain'], t['w2_plain'] = T.gm_ffn_weights(params['hidden'], params['c'])
    return t


# ------------------------------------------------------------------------------------------------ specs
def exact(ref):
    return dict(kind='exact', ref=ref)


def arith(ref, tol, ref32=None, what='f32-arith', dtype=F32):
    assert (tol is None) != (ref32 is None)
    return dict(kind='arith', ref=ref.to(F64), tol=tol, ref32=None if ref32 is None else ref32.to(F32), what=what, dtype=dtype)


def bf16(ref):
    return dict(kind='bf16', ref=ref.to(F64))


def spec_tol(s):
    """(tol relative to scale, scale, err32 or None) of an arith / bf16 spec."""
    sc = max(1.0, float(s['ref'].abs().max())) if s['ref'].numel() else 1.0
    if s['kind'] == 'bf16':
        return BF16_ULP, sc, None
    if s['tol'] is not None:
        return s['tol'], sc, None
    e32 = float((s['ref32'].to(F64) - s['ref']).abs().max()) if s['ref'].numel() else 0.0
    return max(MEASURED_FACTOR * e32, MEASURED_FLOOR * sc) / sc, sc, e32


def _known(p, *names):
    unknown = set(p) - set(names)
    if unknown:
        raise KeyError(f'flat_ref: parameters it does not know: {sorted(unknown)}')
    return [p[n] for n in names]


def _bc(t, n, c, dt):
    return t.to(dt).reshape(n, 1, c)


# ------------------------------------------------------------------------------------------------ normalisation
def ref_chan_stats(p, t):
    n, hw, c, ld, P = _known(p, 'n', 'hw', 'c', 'ld', 'P')
    x = t['x'].to(F64).reshape(n, hw, c)
    return {'part': dict(kind='stats', n=n, P=P, c=c, hw=hw, sum=x.sum(1), sumsq=(x * x).sum(1), absum=x.abs().sum(1))}


def _scale_shift(mean, var, n, c, G, eps, gamma, beta):
    rstd = (1.0 / torch.sqrt(var + eps)).reshape(n, G, 1).expand(n, G, c // G).reshape(n, c)
    mean = mean.reshape(n, G, 1).expand(n, G, c // G).reshape(n, c)
    scale = rstd if gamma is None else gamma.to(F64).reshape(1, c) * rstd
    shift = -mean * scale if beta is None else beta.to(F64).reshape(1, c) - mean * scale
    return scale, shift


def ref_norm_finalize(p, t, drop=()):
    n, hw, c, G, P, affine, eps = _known(p, 'n', 'hw', 'c', 'G', 'P', 'affine', 'eps')
    part = t['part'].to(F64).reshape(n, P, G, c // G, 2).sum((1, 3))
    cnt = hw * (c // G)
    mean = part[..., 0] / cnt
    var = part[..., 1] / cnt - mean * mean                      # biased
    sc, sh = _scale_shift(mean, var, n, c, G, eps, None if 'g' in drop else t.get('g'), None if 'b' in drop else t.get('b'))
    return {'scale': arith(sc, 2e-4, what='reduction'), 'shift': arith(sh, 2e-4, what='reduction')}


def ref_group_stats(p, t, drop=()):
    n, hw, c, G, eps, affine = _known(p, 'n', 'hw', 'c', 'G', 'eps', 'affine')
    assert ('g' in t) == ('b' in t) == bool(affine)
    x = t['x'].to(F64).reshape(n, hw, G, c // G)
    mean = x.mean((1, 3))
    var = ((x - mean.reshape(n, 1, G, 1)) ** 2).mean((1, 3))
    sc, sh = _scale_shift(mean, var, n, c, G, eps, None if 'g' in drop else t.get('g'), None if 'b' in drop else t.get('b'))
    return {'scale': arith(sc, 2e-5, what='reduction'), 'shift': arith(sh, 2e-5, what='reduction')}


def ref_affine_act(p, t, act=None):
    n, hw, c, a = _known(p, 'n', 'hw', 'c', 'act')
    v = t['x'].to(F64).reshape(n, hw, c) * _bc(t['s'], n, c, F64) + _bc(t['h'], n, c, F64)
    return {'o': arith(_act(v, a if act is None else act).reshape(n * hw, c), 2e-4)}


def ref_norm_act_bf16(p, t, act=None, drop=()):
    n, hw, c, in_bf16, a, affine = _known(p, 'n', 'hw', 'c', 'in_bf16', 'act', 'affine')
    assert (t['x'].dtype == torch.bfloat16) == bool(in_bf16) and ('s' in t) == ('h' in t) == bool(affine)
    v = t['x'].to(F64).reshape(n, hw, c)
    if affine and 'sh' not in drop:                              # scale / shift NULL: a plain cast
        v = v * _bc(t['s'], n, c, F64) + _bc(t['h'], n, c, F64)
    return {'o': bf16(_act_pro(v, a if act is None else act).reshape(n * hw, c))}


def ref_gm_join(p, t, drop=()):
    n, hw, c, with_a = _known(p, 'n', 'hw', 'c', 'with_a')
    a = t['a'].to(F64).reshape(n, hw, c)
    assert ('sa' in t) == ('ha' in t) == bool(with_a)
    if with_a and 'sa' not in drop:
        a = a * _bc(t['sa'], n, c, F64)
    if with_a and 'ha' not in drop:
        a = a + _bc(t['ha'], n, c, F64)
    b = torch.relu(t['b'].to(F64).reshape(n, hw, c) * _bc(t['sb'], n, c, F64) + _bc(t['hb'], n, c, F64))
    return {'o': arith(torch.relu(a + b).reshape(n * hw, c), 2e-4)}


# ------------------------------------------------------------------------------------------------ matrix kernels
def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def ref_gm_mlp(p, t):
    m, c = _known(p, 'm', 'c')
    x = bf16r(torch.cat([t['a'], t['b']], -1))
    h = bf16r(_gelu(x @ t['w0'].to(F64).t()))                   # the hidden activations are rounded to bf16 for the second MFMA
    return {'o': arith(h @ t['w2'].to(F64).t(), 2e-3, what='matrix')}


def ref_gm_ffn_x3(p, t):
    m, hidden, c, eps, exact_act = _known(p, 'm', 'hidden', 'c', 'eps', 'exact_act')
    x = torch.cat([t['src'], t['msg']], -1).to(F64)
    h = _gelu(x @ t['w0_plain'].to(F64).t())
    y = F.layer_norm(h @ t['w2_plain'].to(F64).t(), (c,), t['g'].to(F64).reshape(c), t['b'].to(F64).reshape(c), eps)
    return {'o': arith(y + t['src'].to(F64), 2e-5, what='matrix')}


def ref_token_linear(p, t, drop=()):
    m, n_out, out_bf16, k, bias = _known(p, 'm', 'n_out', 'out_bf16', 'k', 'bias')
    y = bf16r(t['x']) @ t['w'].to(F64).t()
    assert ('b' in t) == bool(bias)
    if bias and 'b' not in drop:
        y = y + t['b'].to(F64).reshape(1, n_out)
    return {'o': arith(y, 2e-5 + (BF16_ULP if out_bf16 else 0.0), what='matrix', dtype=torch.bfloat16 if out_bf16 else F32)}


# ------------------------------------------------------------------------------------------------ range probe, LayerNorm, GEGLU
def ref_absmax(p, t):
    n, r, c, ld, zeroed = _known(p, 'n', 'r', 'c', 'ld', 'zeroed')
    return {'amax': dict(kind='amax', of=t['x'].reshape(n, r * c), n=n)}


def _layernorm(x, g, b, eps, dt):
    x = x.to(dt)
    mu = x.mean(1, keepdim=True)
    var = ((x - mu) ** 2).mean(1, keepdim=True)                  # biased, like nn.LayerNorm
    return (x - mu) / torch.sqrt(var + eps) * g.to(dt).reshape(1, -1) + b.to(dt).reshape(1, -1)


def ref_layernorm(p, t, drop=()):
    m, c, res, pos_rows, eps = _known(p, 'm', 'c', 'res', 'pos_rows', 'eps')
    y = _layernorm(t['x'], t['g'], t['b'], eps, F64)
    assert ('res' in t) == bool(res) and ('pos' in t) == bool(pos_rows)
    out = {'o': arith(y + t['res'].to(F64) if res and 'res' not in drop else y, 2e-5, what='reduction')}
    if pos_rows:
        pos = t['pos'].to(F64)[torch.arange(m) % pos_rows]
        out['o2'] = arith(y if 'pos' in drop else y + pos, 2e-5, what='reduction')
    return out


def ref_layernorm_amax(p, t, drop=()):
    n, rows, c, eps, zeroed = _known(p, 'n', 'rows', 'c', 'eps', 'zeroed')
    y = _layernorm(t['x'], t['g'], t['b'], eps, F64)
    return {'o': arith(y if 'res' in drop else y + t['res'].to(F64), 2e-5, what='reduction'), 'amax': dict(kind='amax', of='o', n=n)}


def _geglu(t, f, dt=F64):
    x = t['x'].to(dt)
    return x[:, :f] * _gelu(x[:, f:])


def ref_geglu(p, t):
    m, f = _known(p, 'm', 'f')
    return {'o': arith(_geglu(t, f), 1e-5)}


def ref_geglu_amax(p, t):
    n, rows, f, zeroed = _known(p, 'n', 'rows', 'f', 'zeroed')
    return {'o': arith(_geglu(t, f), 1e-5), 'amax': dict(kind='amax', of='o', n=n)}


# ------------------------------------------------------------------------------------------------ arg-max, status, nearest code
def ref_argmax_gather(p, t):
    m, ncodes, dim = _known(p, 'm', 'ncodes', 'dim')
    lg = t['logits']
    assert bool(torch.isfinite(lg).all())
    idx = lg.argmax(-1)                                          # torch: the lowest index on ties
    top2 = lg.to(F64).topk(2, -1).values
    return {'idx': exact(idx.to(torch.int32).reshape(1, m)), 'o': exact(t['cb'][idx]), 'margin': arith((top2[:, 0] - top2[:, 1]).reshape(1, m), 1e-6),
            'status': exact(torch.zeros(1, 1, dtype=torch.int32))}


def ref_nonfinite_flag(p, t):
    (n,) = _known(p, 'n')
    bad = not bool(torch.isfinite(t['x']).all())
    return {'status': exact(torch.full((1, 1), 2 if bad else 0, dtype=torch.int32))}


def ref_vq_nearest(p, t):
    m, ncodes, dim = _known(p, 'm', 'ncodes', 'dim')
    z, cb = t['z'].to(F64), t['cb'].to(F64)
    d = (z * z).sum(1, keepdim=True) + (cb * cb).sum(1) - 2 * z @ cb.t()
    return {'idx': dict(kind='argmin', d=d)}


def ref_channel_argmax(p, t):
    m, c, ld = _known(p, 'm', 'c', 'ld')
    return {'o': exact(t['x'].argmax(-1).to(torch.uint8).reshape(1, m))}


# ------------------------------------------------------------------------------------------------ KEEP / GMFlow elementwise
def ref_kalman(p, t):
    n, hw, c = _known(p, 'n', 'hw', 'c')
    g = t['g'].to(F64).reshape(n, hw, 1)
    return {'o': arith(((1 - g) * t['a'].to(F64).reshape(n, hw, c) + g * t['b'].to(F64).reshape(n, hw, c)).reshape(n * hw, c), 1e-6)}


def ref_flow_warp(p, t):
    """oracle/keep_oracle.py:flow_warp (AU:113-144) in float64: grid_sample(zeros, align_corners=True) on the grid 2 v / max(W - 1, 1) - 1,
    v = x + flow.  On a one-pixel axis the un-normalisation ((g + 1) / 2) * (W - 1) is 0 whatever the flow: the pixel itself is sampled."""
    n, h, w, c = _known(p, 'n', 'h', 'w', 'c')
    x = t['x'].to(F64).reshape(n, h, w, c).permute(0, 3, 1, 2)
    out = O.flow_warp(x, t['flow'].to(F64).reshape(n, h, w, 2))
    return {'o': arith(out.permute(0, 2, 3, 1).reshape(n * h * w, c), 1e-5)}


def ref_convex_upsample(p, t):
    n, h, w, k = _known(p, 'n', 'h', 'w', 'k')
    mask = t['mask'].to(F64).reshape(n, h, w, 9 * k * k).permute(0, 3, 1, 2)
    flow = t['flow'].to(F64).reshape(n, h, w, 2).permute(0, 3, 1, 2)
    m = torch.softmax(mask.reshape(n, 1, 9, k, k, h, w), dim=2)
    up = F.unfold(k * flow, [3, 3], padding=1).view(n, 2, 9, 1, 1, h, w)
    ref = torch.sum(m * up, dim=2).permute(0, 1, 4, 2, 5, 3).reshape(n, 2, k * h, k * w)
    return {'o': arith(ref.permute(0, 2, 3, 1).reshape(n * k * h * k * w, 2), 1e-5)}


def ref_bilinear_upscale(p, t):
    planes, h, w, s = _known(p, 'planes', 'h', 'w', 's')
    x = t['x'].to(F64).reshape(1, planes, h, w)
    return {'o': arith(F.interpolate(x, scale_factor=s, mode='bilinear', align_corners=False).reshape(planes * h * s, w * s), 1e-6)}


_GM_MEAN, _GM_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _gm_normalise(x):
    """GF:56-57 then GM/utils.py:55-63 on [n, 3, ...] float64."""
    shape = (1, 3) + (1,) * (x.dim() - 2)
    return (((x + 1) / 2 * 255) / 255.0 - torch.tensor(_GM_MEAN, dtype=F64).reshape(shape)) / torch.tensor(_GM_STD, dtype=F64).reshape(shape)


def ref_nchw_to_nhwc(p, t, mode=None):
    n, c, hw, md = _known(p, 'n', 'c', 'hw', 'mode')
    md = md if mode is None else mode
    x = t['x'].reshape(n, c, hw)
    if md == 0:
        return {'o': exact(x.permute(0, 2, 1).reshape(n * hw, c).contiguous())}
    if md != 1:
        raise ValueError(f'mode {md}')
    return {'o': arith(_gm_normalise(x.to(F64)).permute(0, 2, 1).reshape(n * hw, c), 1e-6)}


def ref_nhwc_to_nchw(p, t):
    n, c, hw = _known(p, 'n', 'c', 'hw')
    return {'o': exact(t['x'].reshape(n, hw, c).permute(0, 2, 1).reshape(n * c, hw).contiguous())}


def ref_rgb_s2d(p, t):
    n, h, w = _known(p, 'n', 'h', 'w')
    v = _gm_normalise(t['x'].to(F64).reshape(n, 3, h, w))
    v = v.reshape(n, 3, h // 2, 2, w // 2, 2).permute(0, 2, 4, 3, 5, 1).reshape(n, h // 2, w // 2, 12)      # channel (dy * 2 + dx) * 3 + c
    return {'o': arith(torch.cat([v, torch.zeros(n, h // 2, w // 2, 4, dtype=F64)], -1).reshape(-1, 16), 1e-6)}


def ref_add_bcast(p, t, alpha=None):
    total, tsize, al = _known(p, 'total', 'tsize', 'alpha')
    al = al if alpha is None else alpha
    idx = torch.arange(total) % tsize

    def f(dt):
        return t['a'].to(dt) + torch.tensor(al, dtype=dt) * t['t'].to(dt)[:, idx]
    return {'o': arith(f(F64), None, f(F32))}


def ref_concat2(p, t):
    m, c1, c2, ld = _known(p, 'm', 'c1', 'c2', 'ld')
    return {'o': exact(torch.cat([t['a'], t['b'], torch.zeros(m, ld - c1 - c2)], -1))}


# ------------------------------------------------------------------------------------------------ converters
def ref_tensor2img(p, t):
    (npix,) = _known(p, 'npix')
    chw = t['x'].numpy().reshape(1, npix, 3).transpose(2, 0, 1)                       # the oracle takes [3, H, W] RGB
    return {'o': exact(torch.from_numpy(CO.net_output_to_bgr_u8(chw)).reshape(npix, 3))}


def ref_img2tensor(p, t):
    npix, fn = _known(p, 'npix', 'fn')
    x = t['x'].numpy().reshape(1, npix, 3)
    if fn == 'keep_img2tensor':
        out = CO.crops_to_net_input([x])[0].transpose(1, 2, 0)
    elif fn == 'keep_bgr_u8_to_comfy':                                               # float32(u8) / 255: one correctly rounded division, RGB
        out = (x[..., ::-1].astype(np.float32) / np.float32(255.0)).astype(np.float32)
    else:
        raise ValueError(fn)
    return {'o': exact(torch.from_numpy(np.ascontiguousarray(out)).reshape(npix, 3))}


def ref_comfy_to_bgr(p, t):
    (npix,) = _known(p, 'npix')
    x = t['x'].numpy().astype(np.float32)
    assert np.isfinite(x).all() and np.abs(x).max() < 1e6
    v = (x * np.float32(255.0)).astype(np.int32).astype(np.uint8)                    # one float32 multiply, truncation, low byte
    return {'o': exact(torch.from_numpy(np.ascontiguousarray(v[:, ::-1])))}


def ref_u8_to_f32(p, t):
    (n,) = _known(p, 'n')
    return {'o': exact(t['x'].to(F32))}


def ref_f32_round_u8(p, t):
    (n,) = _known(p, 'n')
    return {'o': exact(torch.from_numpy(np.round(np.clip(t['x'].numpy(), 0, 255)).astype(np.uint8)))}


# ------------------------------------------------------------------------------------------------ detection trunks
def _nchw(t, n, h, w, c):
    return t.reshape(n, h, w, c).permute(0, 3, 1, 2)


def _rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


def ref_maxpool3s2(p, t):
    n, h, w, c = _known(p, 'n', 'h', 'w', 'c')
    return {'o': exact(_rows(F.max_pool2d(_nchw(t['x'], n, h, w, c), 3, 2, 1)))}


def ref_maxpool2d(p, t):
    n, h, w, c, in_ld, out_ld, k, stride, pad, ceil = _known(p, 'n', 'h', 'w', 'c', 'in_ld', 'out_ld', 'k', 'stride', 'pad', 'ceil')
    return {'o': exact(_rows(F.max_pool2d(_nchw(t['x'], n, h, w, c), k, stride, pad, ceil_mode=bool(ceil))))}


def ref_dwconv(p, t, drop=(), act=None):
    n, h, w, c, stride, a, bias = _known(p, 'n', 'h', 'w', 'c', 'stride', 'act', 'bias')
    wt = t['w'].to(F64).reshape(3, 3, c).permute(2, 0, 1).reshape(c, 1, 3, 3)        # w[ky][kx][c] = weight[c, 0, ky, kx]
    assert ('b' in t) == bool(bias)
    b = t['b'].to(F64).reshape(c) if bias and 'b' not in drop else None
    y = F.conv2d(_nchw(t['x'].to(F64), n, h, w, c), wt, b, stride=stride, padding=1, groups=c)
    return {'o': arith(_rows(_act(y, a if act is None else act)), 2e-6)}


def ref_slice_copy(p, t):
    n, h, w, c, src_ld, dst_ld, u = _known(p, 'n', 'h', 'w', 'c', 'src_ld', 'dst_ld', 'up')
    src = t['src'].reshape(n, h >> u, w >> u, c)
    if u:
        src = src.repeat_interleave(2, 1).repeat_interleave(2, 2)
    return {'dst': exact(src[:, :h, :w].reshape(-1, c).contiguous())}


def ref_channel_shuffle2(p, t):
    rows, half, a_ld, b_ld = _known(p, 'rows', 'half', 'a_ld', 'b_ld')
    return {'o': exact(torch.stack([t['a'], t['b']], -1).reshape(rows, 2 * half))}


def ref_upsample_add(p, t):
    n, h, w, hb, wb, c = _known(p, 'n', 'h', 'w', 'hb', 'wb', 'c')
    up = F.interpolate(_nchw(t['b'], n, hb, wb, c), size=(h, w), mode='nearest')
    return {'o': exact(t['a'] + _rows(up))}                                            # one float32 addition


def ref_act_inplace(p, t, act=None):
    n, a = _known(p, 'n', 'act')
    a = a if act is None else act
    if a in (ACT_NONE, ACT_RELU, ACT_LRELU02, ACT_LRELU01):                            # a selection and at most one float32 multiply
        x = t['x']
        slope = {ACT_NONE: 1.0, ACT_RELU: 0.0, ACT_LRELU02: 0.2, ACT_LRELU01: 0.1}[a]
        return {'x': exact(torch.where(x > 0, x, x * torch.tensor(slope, dtype=F32)) if a != ACT_RELU else torch.relu(x))}
    return {'x': arith(_act(t['x'].to(F64), a), 2e-4)}


def ref_yolo_decode(p, t):
    n, ny, nx, stride, row0, rows_after = _known(p, 'n', 'ny', 'nx', 'stride', 'row0', 'rows_after')
    r = t['raw'].to(F64).reshape(n, ny, nx, 3, 16).permute(0, 3, 1, 2, 4)
    yv, xv = torch.meshgrid(torch.arange(ny), torch.arange(nx), indexing='ij')
    grid = torch.stack((xv, yv), 2).reshape(1, 1, ny, nx, 2).to(F64)
    ag = t['anch'].to(F64).reshape(1, 3, 1, 1, 2)
    o = torch.zeros_like(r)
    o[..., [0, 1, 2, 3, 4, 15]] = r[..., [0, 1, 2, 3, 4, 15]].sigmoid()
    o[..., 0:2] = (o[..., 0:2] * 2.0 - 0.5 + grid) * stride
    o[..., 2:4] = (o[..., 2:4] * 2) ** 2 * ag
    for q in range(5):
        o[..., 5 + 2 * q:7 + 2 * q] = r[..., 5 + 2 * q:7 + 2 * q] * ag + grid * stride
    rows_total = row0 + 3 * ny * nx + rows_after
    pred = torch.zeros(n, rows_total, 16, dtype=F64)                                  # rows outside [row0, row0 + 3 ny nx) keep the caller's zeros
    pred[:, row0:row0 + 3 * ny * nx] = o.reshape(n, -1, 16)
    return {'pred': arith(pred.reshape(-1, 16), 2e-5)}


def ref_yolo_letterbox(p, t, swap_rb=None):
    n, h, w, rh, rw, top, left, h2, w2, sw = _known(p, 'n', 'h', 'w', 'rh', 'rw', 'top', 'left', 'h2', 'w2', 'swap_rb')
    sw = sw if swap_rb is None else swap_rb
    frames = t['x'].numpy().reshape(n, h, w, 3)
    out = np.full((n, h2, w2, 3), 114, np.uint8)
    for i in range(n):
        img = np.ascontiguousarray(frames[i][:, :, ::-1]) if sw else frames[i]
        out[i, top:top + rh, left:left + rw] = FO.cv2_resize_linear_u8(img, rw, rh)
    return {'o': exact((torch.from_numpy(out).float() / 255.0).reshape(-1, 3))}


def _dets_spec(n, cap, thr, score, alive, rows, rows32):
    """score [n, P']: the thresholded quantity (float64); alive [n, P']: the float64 surviving set; rows / rows32 [n, P', 16]."""
    return dict(kind='dets', n=n, cap=cap, thr=thr, score=score, alive=alive, rows=rows, rows32=rows32)


def ref_yolo_select(p, t):
    n, P, cap, thr = _known(p, 'n', 'p', 'cap', 'thr')

    def rows(dt):
        x = t['pred'].to(dt).reshape(n, P, 16)
        conf = x[..., 15] * x[..., 4]
        hw, hh = x[..., 2] / 2, x[..., 3] / 2
        idx = torch.arange(P, dtype=dt).expand(n, P)
        return torch.cat([torch.stack([x[..., 0] - hw, x[..., 1] - hh, x[..., 0] + hw, x[..., 1] + hh, conf], -1), x[..., 5:15], idx[..., None]], -1)
    x = t['pred'].to(F64).reshape(n, P, 16)
    thr64 = float(np.float32(thr))
    conf = x[..., 15] * x[..., 4]
    score = torch.minimum(x[..., 4], conf)                        # both objectness and conf must exceed the threshold
    return {'dets': _dets_spec(n, cap, thr64, torch.stack([x[..., 4], conf], -1), score > thr64, rows(F64), rows(F32))}


def ref_retina_decode(p, t):
    n, P, cap, var0, var1, sx, sy, thr = _known(p, 'n', 'p', 'cap', 'var0', 'var1', 'sx', 'sy', 'thr')

    def rows(dt):
        hd = t['heads'].to(dt).reshape(n, P, 32)
        pr = t['priors'].to(dt).reshape(1, 2 * P, 4)
        cls = hd[..., 0:4].reshape(n, 2 * P, 2)
        box = hd[..., 4:12].reshape(n, 2 * P, 4)
        lm = hd[..., 12:32].reshape(n, 2 * P, 5, 2)
        score = torch.softmax(cls, -1)[..., 1]
        v0, v1 = torch.tensor(var0, dtype=dt), torch.tensor(var1, dtype=dt)
        cxy = pr[..., :2] + box[..., :2] * v0 * pr[..., 2:]
        wh = pr[..., 2:] * torch.exp(box[..., 2:] * v1)
        x1y1 = cxy - wh / 2
        x2y2 = wh + x1y1
        s = torch.tensor([sx, sy], dtype=dt)
        lms = (pr[..., None, :2] + lm * v0 * pr[..., None, 2:]) * s
        idx = torch.arange(2 * P, dtype=dt).expand(n, 2 * P)
        return score, torch.cat([x1y1 * s, x2y2 * s, score[..., None], lms.reshape(n, 2 * P, 10), idx[..., None]], -1)
    score, r64 = rows(F64)
    thr64 = float(np.float32(thr))
    return {'dets': _dets_spec(n, cap, thr64, score[..., None], score > thr64, r64, rows(F32)[1])}


def _nms(p, t, ordered):
    n, cap, cnt, o_, iou = _known(p, 'n', 'cap', 'cnt', 'ordered', 'iou')
    assert bool(o_) == ordered
    d = t['dets'].numpy().reshape(n, cap, 16)
    counts = t['counts'].numpy().reshape(n)
    out, oc = np.zeros((n, cap, 16), np.float32), np.zeros((1, n), np.int32)
    for i in range(n):
        c = int(counts[i])
        if c > cap:
            oc[0, i] = -1
            continue
        rows = d[i, :c]
        if ordered:                                              # the caller's order: rank -> row
            rows = rows[t['order'].numpy().reshape(n, cap)[i, :c]]
            scores = -np.arange(c, dtype=np.float32)
        else:
            scores = rows[:, 4]
            assert len(np.unique(scores)) == c, 'equal scores are handed back to the host (-2): not what this case is about'
        keep = FO._greedy_nms(rows[:, :4], scores, np.float32(iou))
        out[i, :len(keep)] = rows[keep]
        oc[0, i] = len(keep)
    return {'o': exact(torch.from_numpy(out).reshape(n * cap, 16)), 'oc': exact(torch.from_numpy(oc))}


def ref_retina_nms(p, t):
    return _nms(p, t, False)


def ref_retina_nms_ordered(p, t):
    return _nms(p, t, True)


# ------------------------------------------------------------------------------------------------ paste-back
@contextlib.contextmanager
def _dst_to_src(m):
    """The table hands the kernels the destination -> source map itself; oracle/paste_oracle.py derives it from the forward matrix.  Inside
    this block the oracle's inversion answers with the table's six doubles, so both read the same map bit for bit."""
    saved = PO.invert_affine
    PO.invert_affine = lambda _M: np.asarray(m, np.float64).reshape(2, 3)
    try:
        yield None
    finally:
        PO.invert_affine = saved


def ref_sep_filter(p, t):
    n, h, w, ntap, classes = _known(p, 'n', 'h', 'w', 'ntap', 'classes')
    kern = t['kern'].numpy().reshape(ntap)
    if classes:
        src = t['lut'].numpy().reshape(-1)[t['cls'].numpy().astype(np.int64)]
    else:
        src = t['src'].numpy()
    src = src.reshape(n, h, w)
    return {'dst': exact(torch.from_numpy(np.stack([PO.sep_filter_f32(src[i], kern) for i in range(n)])).reshape(n * h, w))}


def ref_warp_affine(p, t, border=None):
    h, w, dh, dw, m, bd = _known(p, 'h', 'w', 'dh', 'dw', 'm', 'border')
    with _dst_to_src(m):
        out = PO.warp_affine_u8(t['src'].numpy().reshape(h, w, 3), None, dw, dh, border=np.array(bd if border is None else border, np.int64))
    return {'dst': exact(torch.from_numpy(out).reshape(dh * dw, 3))}


def ref_warp_ones(p, t):
    h, w, fh, fw, m = _known(p, 'h', 'w', 'fh', 'fw', 'm')
    with _dst_to_src(m):
        return {'dst': exact(torch.from_numpy(PO.warp_affine_f32(np.ones((fh, fw), np.float32), None, w, h)))}


def ref_erode(p, t):
    h, w, k = _known(p, 'h', 'w', 'k')
    return {'dst': exact(torch.from_numpy(PO.erode_rect(t['src'].numpy().reshape(h, w), k)))}


def ref_draw_box(p, t):
    h, w, fh, fw, m, box, thickness = _known(p, 'h', 'w', 'fh', 'fw', 'm', 'box', 'thickness')
    x0, y0, x1, y1 = box
    with _dst_to_src(m):
        hit = PO.border_mask(None, w, h, thickness, (fh, fw))
    inside = np.zeros((h, w), bool)
    inside[y0:y1, x0:x1] = True
    frame = t['frame'].numpy().reshape(h, w, 3).copy()
    frame[hit & inside] = np.array([0, 255, 0], np.uint8)
    return {'frame': exact(torch.from_numpy(frame).reshape(h * w, 3))}


def ref_paste_face(p, t, mask_border=None):
    h, w, fh, fw, m, box, frame_mask, mb = _known(p, 'h', 'w', 'fh', 'fw', 'm', 'box', 'frame_mask', 'mask_border')
    mb = mb if mask_border is None else mask_border
    x0, y0, x1, y1 = box
    frame = t['frame'].numpy().reshape(h, w, 3).astype(np.float32)
    with _dst_to_src(m):
        face = PO.warp_affine_u8(t['face'].numpy().reshape(fh, fw, 3), None, w, h)
        if frame_mask:
            soft = t['mask'].numpy().reshape(h, w).astype(np.float32)
        else:
            mk = t['mask'].numpy().reshape(fh, fw).astype(np.float32).copy()
            if mb > 0:
                mk[:mb, :] = 0; mk[-mb:, :] = 0; mk[:, :mb] = 0; mk[:, -mb:] = 0
            soft = PO.warp_affine_f32((mk / np.float32(255.0)).astype(np.float32), None, w, h)
    soft = soft[:, :, None]
    blend = soft * face.astype(np.float32) + (np.float32(1) - soft) * frame
    out = frame.copy()
    out[y0:y1, x0:x1] = blend[y0:y1, x0:x1]
    return {'frame': exact(torch.from_numpy(out.astype(np.float32)).reshape(h * w, 3))}


def ref_lanczos(p, t):
    n, h, w, h2, w2, _ = _known(p, 'n', 'h', 'w', 'h2', 'w2', 'unaligned')       # (unaligned: where the buffers lie, not what they hold)
    src = t['src'].numpy().reshape(n, h, w, 3)
    for name, (S, D) in (('x', (w, w2)), ('y', (h, h2))):          # the table's coefficient tables are the restated ones
        ofs, coef = LZ.axis_tables(S, D)
        assert np.array_equal(ofs, t[name + 'o'].numpy().reshape(-1)) and np.array_equal(coef, t[name + 'c'].numpy().reshape(D, 8)), name
    return {'dst': exact(torch.from_numpy(np.stack([LZ.resize_lanczos4(src[i], w2, h2) for i in range(n)])).reshape(-1, 3))}


# ------------------------------------------------------------------------------------------------ the table of references
# entry point -> (class, reference)
REFS = {
    'keep_chan_stats': ('reduction', ref_chan_stats), 'keep_norm_finalize': ('reduction', ref_norm_finalize), 'keep_group_stats': ('reduction', ref_group_stats),
    'keep_affine_act': ('f32-arith', ref_affine_act), 'keep_norm_act_bf16': ('bf16', ref_norm_act_bf16), 'keep_gm_mlp': ('matrix', ref_gm_mlp),
    'keep_gm_ffn_x3': ('matrix', ref_gm_ffn_x3), 'keep_token_linear': ('matrix', ref_token_linear), 'keep_gm_join': ('f32-arith', ref_gm_join),
    'keep_absmax': ('amax', ref_absmax), 'keep_layernorm': ('reduction', ref_layernorm), 'keep_geglu': ('f32-arith', ref_geglu),
    'keep_layernorm_amax': ('reduction+amax', ref_layernorm_amax), 'keep_geglu_amax': ('f32-arith+amax', ref_geglu_amax),
    'keep_argmax_gather': ('exact', ref_argmax_gather), 'keep_nonfinite_flag': ('exact', ref_nonfinite_flag), 'keep_vq_nearest': ('index', ref_vq_nearest),
    'keep_kalman_update': ('f32-arith', ref_kalman), 'keep_flow_warp': ('f32-arith', ref_flow_warp), 'keep_convex_upsample': ('f32-arith', ref_convex_upsample),
    'keep_bilinear_upscale': ('f32-arith', ref_bilinear_upscale), 'keep_nchw_to_nhwc': ('exact|f32-arith', ref_nchw_to_nhwc), 'keep_rgb_s2d': ('f32-arith', ref_rgb_s2d),
    'keep_nhwc_to_nchw': ('exact', ref_nhwc_to_nchw), 'keep_add_bcast': ('f32-arith', ref_add_bcast), 'keep_concat2': ('exact', ref_concat2),
    'keep_tensor2img': ('exact', ref_tensor2img), 'keep_img2tensor': ('exact', ref_img2tensor), 'keep_bgr_u8_to_comfy': ('exact', ref_img2tensor),
    'keep_comfy_to_bgr_u8': ('exact', ref_comfy_to_bgr), 'keep_channel_argmax': ('exact', ref_channel_argmax), 'keep_maxpool3s2': ('exact', ref_maxpool3s2),
    'keep_dwconv3x3': ('f32-arith', ref_dwconv), 'keep_retina_nms': ('exact', ref_retina_nms), 'keep_retina_nms_ordered': ('exact', ref_retina_nms_ordered),
    'keep_maxpool2d': ('exact', ref_maxpool2d), 'keep_slice_copy': ('exact', ref_slice_copy), 'keep_channel_shuffle2': ('exact', ref_channel_shuffle2),
    'keep_yolo_decode': ('f32-arith', ref_yolo_decode), 'keep_yolo_letterbox_u8': ('exact', ref_yolo_letterbox), 'keep_yolo_select': ('dets', ref_yolo_select),
    'keep_upsample_add': ('exact', ref_upsample_add), 'keep_act_inplace': ('exact|f32-arith', ref_act_inplace), 'keep_retina_decode': ('dets', ref_retina_decode),
    'keep_sep_filter': ('exact', ref_sep_filter), 'keep_u8_to_f32': ('exact', ref_u8_to_f32), 'keep_f32_round_u8': ('exact', ref_f32_round_u8),
    'keep_warp_affine_u8': ('exact', ref_warp_affine), 'keep_warp_ones': ('exact', ref_warp_ones), 'keep_draw_box': ('exact', ref_draw_box),
    'keep_erode_rect': ('exact', ref_erode), 'keep_paste_face': ('exact', ref_paste_face), 'keep_resize_lanczos4_u8': ('exact', ref_lanczos),
}


def reference(fn, params, t, **variant):
    """The specs of entry point ``fn`` for a case with parameters ``params`` on payloads ``t``.  ``variant``: a deliberately wrong variant
    (an optional input dropped, another activation ...) for the sensitivity checks."""
    if fn not in REFS:
        raise KeyError(f'no reference for {fn}')
    return REFS[fn][1](dict(params), t, **variant)


def case_class(fn, specs):
    """The one class of a case: the entry point's, resolved by the kinds of its specs where the class depends on a parameter."""
    klass = REFS[fn][0]
    if '|' in klass:
        kinds = {s['kind'] for s in specs.values()}
        assert len(kinds) == 1, kinds
        klass = 'exact' if kinds == {'exact'} else 'f32-arith'
    return klass


def removals(fn, params, t):
    """(what, output name, reference spec without it) for every optional input / switch the case uses (tests/test_host_logic.py: each must
    move the reference by SENSITIVITY x tol x scale, or flip bits of an exact output)."""
    p = params
    r = lambda **v: reference(fn, p, t, **v)  # noqa: E731
    if fn == 'keep_layernorm':
        if p['res']:
            yield 'residual', 'o', r(drop=('res',))['o']
        if p['pos_rows']:
            yield 'pos', 'o2', r(drop=('pos',))['o2']
            yield 'out2 is not out', 'o2', dict(r()['o2'], ref=r()['o'].get('ref'))
    if fn == 'keep_layernorm_amax':
        yield 'residual', 'o', r(drop=('res',))['o']
    if fn == 'keep_norm_act_bf16' and p['affine']:
        yield 'scale / shift', 'o', r(drop=('sh',))['o']
    if fn in ('keep_norm_finalize', 'keep_group_stats') and p['affine']:
        yield 'gamma', 'scale', r(drop=('g',))['scale']
        yield 'beta', 'shift', r(drop=('b',))['shift']
    if fn == 'keep_gm_join' and p['with_a']:
        yield 'sa', 'o', r(drop=('sa',))['o']
        yield 'ha', 'o', r(drop=('ha',))['o']
    if fn in ('keep_token_linear', 'keep_dwconv3x3') and p['bias']:
        yield 'bias', 'o', r(drop=('b',))['o']
    if fn in ('keep_affine_act', 'keep_dwconv3x3', 'keep_act_inplace') and p['act'] != ACT_NONE:
        yield 'activation', 'x' if fn == 'keep_act_inplace' else 'o', r(act=ACT_NONE)['x' if fn == 'keep_act_inplace' else 'o']
    if fn == 'keep_norm_act_bf16' and p['act'] != PRO_NONE:
        yield 'activation', 'o', r(act=PRO_NONE)['o']
    if fn == 'keep_add_bcast':
        yield 'alpha', 'o', r(alpha=0.0)['o']
    if fn == 'keep_nchw_to_nhwc' and p['mode']:
        yield 'mode', 'o', dict(r()['o'], ref=r(mode=0)['o']['ref'].to(F64))
    if fn == 'keep_slice_copy' and p['up']:
        full, low = r()['dst']['ref'], t['src'].reshape(p['n'], p['h'] >> 1, p['w'] >> 1, p['c'])
        shifted = torch.zeros_like(full).reshape(p['n'], p['h'], p['w'], p['c'])
        shifted[:, :p['h'] >> 1, :p['w'] >> 1] = low                  # `up` ignored: the source copied pixel for pixel
        yield 'up', 'dst', exact(shifted.reshape(full.shape))
    if fn == 'keep_sep_filter' and p['classes']:
        yield 'classes + lut', 'dst', exact(torch.from_numpy(np.stack([PO.sep_filter_f32(
            t['cls'].numpy().reshape(p['n'], p['h'], p['w'])[i].astype(np.float32), t['kern'].numpy().reshape(-1)) for i in range(p['n'])])).reshape(p['n'] * p['h'], p['w']))
    if fn == 'keep_paste_face' and not p['frame_mask'] and p['mask_border']:
        yield 'mask_border', 'frame', r(mask_border=0)['frame']
    if fn == 'keep_warp_affine_u8':                                   # (a warp that stays inside the source never reads the colour)
        black = r(border=(0, 0, 0))['dst']
        if not torch.equal(black['ref'], r()['dst']['ref']):
            yield 'border colour', 'dst', black
    if fn == 'keep_yolo_letterbox_u8' and p['swap_rb']:
        yield 'swap_rb', 'o', r(swap_rb=0)['o']


# ------------------------------------------------------------------------------------------------ the judge
def with_amax_neighbours(regions):
    """The 9-slot amax arena with the slots around the case's own as windows too, holding a marker, so that the plain run hands them back."""
    import footprint as FP
    out = []
    for r in regions:
        if 'amax' in r.windows:
            off, n, data = r.windows['amax']
            assert (off, r.ld) == (AMAX_OFF, AMAX_SLOTS)
            hi = AMAX_SLOTS - off - n
            r = FP.Region(1, AMAX_SLOTS, {'amax_lo': (0, off, torch.full((1, off), AMAX_MARK)), 'amax': (off, n, data),
                                          'amax_hi': (off + n, hi, torch.full((1, hi), AMAX_MARK))}, F32, 'rw')
        out.append(r)
    return out


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.uint8, 8: torch.int64}[t.element_size()]) if t.dtype.is_floating_point else t


def _judge_dets(what, s, got):
    n, cap, thr = s['n'], s['cap'], s['thr']
    counts = got['counts'].detach().cpu().reshape(n).tolist()
    dets = got['dets'].detach().cpu().reshape(n, cap, 16)
    near = ((s['score'] - thr).abs() <= THRESHOLD_BAND).any(-1)                          # rows the float32 kernel may decide either way
    sure = s['alive'] & ~near
    err, pos = 0.0, None
    ref_rows, ref32 = s['rows'], s['rows32']
    sc = max(1.0, float(ref_rows[s['alive']].abs().max())) if bool(s['alive'].any()) else 1.0
    e32 = float((ref32.to(F64) - ref_rows)[s['alive']].abs().max()) if bool(s['alive'].any()) else 0.0
    tol = max(MEASURED_FACTOR * e32, MEASURED_FLOOR * sc) / sc
    for i in range(n):
        lo, hi = int(sure[i].sum()), int((s['alive'][i] | near[i]).sum())
        assert lo <= counts[i] <= hi, f'{what}: frame {i} counts {counts[i]} survivors, the float64 reference {lo} .. {hi}'
        if counts[i] > cap:
            continue                                                                    # which rows an overflowing frame keeps is open
        rows = dets[i, :counts[i]]
        rows = rows[torch.argsort(rows[:, 15])]
        idx = rows[:, 15].long()
        assert len(set(idx.tolist())) == counts[i], f'{what}: frame {i} holds a row twice'
        have = torch.zeros_like(sure[i])
        have[idx] = True
        assert bool((have | ~sure[i]).all()) and not bool((have & ~(s['alive'][i] | near[i])).any()), \
            f'{what}: frame {i} holds another set of rows than the float64 reference: {sorted(set(idx.tolist()) ^ set(sure[i].nonzero().reshape(-1).tolist()))[:8]}'
        e, _, ps = measure(rows, ref_rows[i, idx]) if counts[i] else (0.0, 1.0, 0)
        if e >= err:
            err, pos = e, (i, ps)
        assert bool((dets[i, counts[i]:] == 0).all()), f'{what}: frame {i} wrote rows beyond its count'
    return err, sc, tol, '-' if pos is None else f'frame {pos[0]} element {pos[1]}', e32


def judge(fn, cid, specs, got):
    """Compare the outputs ``got`` (name -> tensor) of one launch of case (fn, cid) with its specs.  Prints the ``[flat-values]`` line;
    raises AssertionError.  Returns [(output, err, scale, tol)]."""
    klass = case_class(fn, specs)
    what = f'{fn}[{cid}]'
    res = []
    fails = []
    for name, s in specs.items():
        kind = s['kind']
        err = e32 = 0.0
        sc, tol, where = 1.0, 0.0, '-'
        if kind == 'exact':
            g, r = got[name].detach().cpu().reshape(s['ref'].shape), s['ref']
            assert g.dtype == r.dtype, (what, name, g.dtype, r.dtype)
            diff = (_bits(g) != _bits(r)).reshape(-1)
            if bool(diff.any()):
                i = int(diff.nonzero()[0])
                err, where = float(diff.sum()), f'element {i}: {g.reshape(-1)[i].item()!r} vs {r.reshape(-1)[i].item()!r}'
                fails.append(f'{name}: {int(diff.sum())} elements differ in bits, first {where}')
        elif kind in ('arith', 'bf16'):
            tol, sc, e32 = spec_tol(s)
            ref = bf16r(s['ref']) if kind == 'bf16' else s['ref']
            g = got[name].detach().cpu().reshape(ref.shape)
            assert g.dtype == (torch.bfloat16 if kind == 'bf16' else s['dtype']), (what, name, g.dtype)
            err, _, pos = measure(g, ref)
            where = f'element {pos} (row {pos // ref.shape[-1]}, column {pos % ref.shape[-1]})'
            if not err <= tol * sc:
                fails.append(f'{name}: err {err:.3e} > {tol * sc:.3e} (scale {sc:.3g}), worst at {where}')
        elif kind == 'stats':
            n, P, c, hw = s['n'], s['P'], s['c'], s['hw']
            part = got[name].detach().cpu().to(F64).reshape(n, P, c, 2).sum(1)
            for label, have, want, lim in (('sum', part[..., 0], s['sum'], hw * 2.0 ** -24 * s['absum']), ('sumsq', part[..., 1], s['sumsq'], hw * 2.0 ** -24 * s['sumsq'])):
                d = torch.where(torch.isfinite(have), (have - want).abs(), torch.full_like(have, math.inf))
                over = d - lim
                i = int(over.reshape(-1).argmax())
                if float(d.reshape(-1)[i]) >= err:
                    err, sc, tol, where = float(d.reshape(-1)[i]), max(1.0, float(want.abs().max())), float(lim.reshape(-1)[i]), f'{label} of image {i // c} channel {i % c}'
                if not float(over.reshape(-1)[i]) <= 0:
                    fails.append(f'{name}: {label} of image {i // c} channel {i % c}: {float(have.reshape(-1)[i])!r} vs {float(want.reshape(-1)[i])!r}, allowed {float(lim.reshape(-1)[i]):.3e}')
            tol = tol / sc
        elif kind == 'amax':
            n = s['n']
            of = got[s['of']] if isinstance(s['of'], str) else s['of']
            per = of.detach().cpu().float().reshape(n, -1).abs().amax(1)
            slots = got[name].detach().cpu().reshape(n)
            if not torch.equal(_bits(slots), _bits(per)):
                err, where = 1.0, f'slots {slots.tolist()}'
                fails.append(f'{name}: slots {slots.tolist()} != max |.| per image {per.tolist()}')
            for side in ('amax_lo', 'amax_hi'):
                nb = got[side].detach().cpu()
                if not torch.equal(_bits(nb), _bits(torch.full_like(nb, AMAX_MARK))):
                    err = 1.0
                    fails.append(f'{name}: a neighbouring amax slot was written: {side} = {nb.tolist()}')
        elif kind == 'argmin':
            d = s['d']
            top2 = torch.topk(d, 2, dim=1, largest=False)
            clear = (top2.values[:, 1] - top2.values[:, 0]) > VQ_MARGIN * float(d.abs().max())
            idx = got[name].detach().cpu().reshape(-1).long()
            assert got[name].dtype == torch.int32 and idx.numel() == d.shape[0]
            skipped = 1.0 - float(clear.float().mean())
            wrong = (idx != top2.indices[:, 0]) & clear
            err, tol, where = float(wrong.sum()), VQ_MARGIN, f'{int((~clear).sum())} of {d.shape[0]} rows inside the margin'
            if not skipped <= VQ_MAX_SKIPPED:
                fails.append(f'{name}: the margin rule leaves out {skipped:.1%} of the rows (cap {VQ_MAX_SKIPPED:.0%})')
            if bool(wrong.any()):
                i = int(wrong.nonzero()[0])
                fails.append(f'{name}: {int(wrong.sum())} rows with a clear margin got another code, first row {i}: {int(idx[i])} vs {int(top2.indices[i, 0])}')
            if not bool(((idx >= 0) & (idx < d.shape[1])).all()):
                fails.append(f'{name}: an index outside the codebook')
        elif kind == 'dets':
            try:
                err, sc, tol, where, e32 = _judge_dets(what, s, got)
                if not err <= tol * sc:
                    fails.append(f'{name}: rows err {err:.3e} > {tol * sc:.3e} (scale {sc:.3g}), worst at {where}')
            except AssertionError as e:
                err = math.inf
                fails.append(str(e))
        else:
            raise KeyError(kind)
        extra = f' err32 {e32:.3e}' if e32 is not None and (kind == 'dets' or (kind == 'arith' and s['tol'] is None)) else ''
        print(f'[flat-values] {fn} {cid} {name}: [{klass}/{kind}] err {err:.3e} scale {sc:.3g} tol {tol:.3e}{extra} worst at {where}')
        res.append((name, err, sc, tol))
    missing = set(got) - set(specs) - {'amax_lo', 'amax_hi', 'counts'}
    assert not missing, f'{what}: outputs nobody judged: {sorted(missing)}'
    assert not fails, f'{what}: ' + '; '.join(fails)
    return res


# ------------------------------------------------------------------------------------------------ what a device would hand back (host proofs)
def fake_outputs(specs):
    """What a correct kernel would hand back for ``specs``: every reference cast to its output's dtype, one statistics partial holding the
    whole sum, the survivors in index order, the amax slots of the faked output and untouched neighbours."""
    got = {}
    for name, s in specs.items():
        kind = s['kind']
        if kind == 'exact':
            got[name] = s['ref'].clone()
        elif kind == 'arith':
            got[name] = s['ref'].to(F32).to(s['dtype'])
        elif kind == 'bf16':
            got[name] = s['ref'].to(F32).to(torch.bfloat16)
        elif kind == 'stats':
            part = torch.zeros(s['n'], s['P'], s['c'], 2)
            part[:, 0, :, 0], part[:, 0, :, 1] = s['sum'].float(), s['sumsq'].float()
            got[name] = part.reshape(1, -1)
        elif kind == 'argmin':
            got[name] = s['d'].argmin(1).to(torch.int32).reshape(1, -1)
        elif kind == 'dets':
            n, cap = s['n'], s['cap']
            d, cnt = torch.zeros(n, cap, 16), torch.zeros(1, n, dtype=torch.int32)
            for i in range(n):
                rows = s['rows'][i][s['alive'][i]].float()
                cnt[0, i] = len(rows)
                d[i, :min(cap, len(rows))] = rows[:cap]
            got[name], got['counts'] = d.reshape(n * cap, 16), cnt
    for name, s in specs.items():
        if s['kind'] == 'amax':
            of = got[s['of']] if isinstance(s['of'], str) else s['of']
            got[name] = of.float().reshape(s['n'], -1).abs().amax(1).reshape(1, s['n'])
            got['amax_lo'] = torch.full((1, AMAX_OFF), AMAX_MARK)
            got['amax_hi'] = torch.full((1, AMAX_SLOTS - AMAX_OFF - s['n']), AMAX_MARK)
    return got


def _flip(t, i):
    t = t.clone()
    flat = _bits(t).reshape(-1) if t.dtype.is_floating_point else t.reshape(-1)
    flat[i] = flat[i] ^ 1
    return flat.view(t.dtype).reshape(t.shape) if t.dtype.is_floating_point else flat.reshape(t.shape)


def doctored(specs, got):
    """(what, outputs) of every deliberately wrong variant of ``got`` the judge must refuse: per output the LAST element (the ragged tail)
    and a middle one moved by 10 x tol x scale (one bit / one index for exact and index outputs), an amax slot one ulp off, a written
    neighbour slot, a survivor too many."""
    for name, s in specs.items():
        kind = s['kind']
        numel = got[name].numel()
        for label, i in (('last', numel - 1), ('middle', numel // 2)):
            g = dict(got)
            if kind == 'exact':
                g[name] = _flip(got[name], i)
            elif kind in ('arith', 'bf16'):
                tol, sc, _ = spec_tol(s)
                v = got[name].clone()
                v.view(-1)[i] = (v.view(-1)[i].double() + 10 * tol * sc).to(v.dtype)
                g[name] = v
            elif kind == 'stats':
                lim = s['hw'] * 2.0 ** -24 * max(float(s['absum'].max()), float(s['sumsq'].max()))
                v = got[name].clone()
                v.view(-1)[i] += 10 * lim
                g[name] = v
            elif kind == 'argmin':
                v = got[name].clone()
                v.view(-1)[i] = (v.view(-1)[i] + 1) % s['d'].shape[1]
                g[name] = v
            elif kind == 'dets':
                n, cap = s['n'], s['cap']
                cnt = got['counts'].reshape(-1).tolist()
                fits = [f for f in range(n) if 0 < cnt[f] <= cap]
                f = fits[-1] if label == 'last' else fits[0]
                e32 = float((s['rows32'].to(F64) - s['rows'])[s['alive']].abs().max())
                sc = max(1.0, float(s['rows'][s['alive']].abs().max()))
                v = got[name].clone().reshape(n, cap, 16)
                r = cnt[f] - 1 if label == 'last' else cnt[f] // 2
                v[f, r, 14 if label == 'last' else 2] += 10 * max(MEASURED_FACTOR * e32, MEASURED_FLOOR * sc)
                g[name] = v.reshape(n * cap, 16)
            elif kind == 'amax':
                continue
            yield f'{name}: {label} element', g
        if kind == 'amax':
            g = dict(got)
            g[name] = torch.nextafter(got[name], torch.full_like(got[name], 1e30))
            yield f'{name}: one ulp off', g
            g = dict(got)
            g[name] = torch.nextafter(got[name], torch.zeros_like(got[name]))[:, [0] + list(range(1, s['n']))]
            g[name][0, -1] = got[name][0, -1]
            if s['n'] > 1:
                yield f'{name}: first slot one ulp low', g
            for side, j in (('amax_lo', -1), ('amax_hi', 0)):
                g = dict(got)
                g[side] = got[side].clone()
                g[side][0, j] = 0.0
                yield f'{name}: {side} written', g
        if kind == 'dets':
            n, cap = s['n'], s['cap']
            g = dict(got)
            g['counts'] = got['counts'].clone()
            g['counts'][0, 0] += 1
            yield f'{name}: one survivor too many counted', g
            cnt = got['counts'].reshape(-1).tolist()
            f = [f_ for f_ in range(n) if 0 < cnt[f_] <= cap][0]
            dead = int((~s['alive'][f]).nonzero()[0])
            v = got[name].clone().reshape(n, cap, 16)
            v[f, 0, 15] = float(dead)
            g = dict(got)
            g[name] = v.reshape(n * cap, 16)
            yield f'{name}: a row that did not survive', g
            v = got[name].clone().reshape(n, cap, 16)
            v[f, cnt[f], 3] = 1.0
            g = dict(got)
            g[name] = v.reshape(n * cap, 16)
            if cnt[f] < cap:
                yield f'{name}: a row written beyond the count', g
