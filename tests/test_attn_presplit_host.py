"""Host checks (no GPU) of the pre-split window-attention path: what keep_attention_kv_split_plan / keep_conv2d_split_plan answer, the new
entry points in header, binding and library (the core header and its argument structs stay as they are), and the pinned census of the
convolution sources (the split output is a run-time branch of existing instantiations: no kernel symbol and no launch site may appear)."""
import ctypes
import itertools
import os
import re

import pytest

import conv_universe as U
from comfyui_keep_amd.engine import hiplib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 0x10000
C = 128


def attn(h=64, w=64, n_img=4, cross=False, shift=0, **over):
    """The window-attention call of net.py:_gm_layer on an h x w token grid."""
    Lt = h * w
    sq, skv = ((Lt * 3 * C, 3 * C, 0),) * 2 if not cross else ((Lt * C, C, 0), (Lt * 2 * C, 2 * C, 0))
    kw = dict(q=A, k=A, v=A, o=A, q_bs=sq[0], q_ts=sq[1], q_hs=0, k_bs=skv[0], k_ts=skv[1], k_hs=0, v_bs=skv[0], v_ts=skv[1], v_hs=0,
              o_bs=Lt * C, o_ts=C, o_hs=0, B=n_img * 4, H=1, Lq=Lt // 4, Lk=Lt // 4, D=C, Dv=C, scale=C ** -0.5, mode=2, img_h=h, img_w=w, ksplit=2,
              shift=(h // 4) if shift else 0, kv_rot=n_img // 2 if cross else 0, n_img=n_img, mma=L.MMA_X3, in_dtype=L.F32)
    kw.update(over)
    return L.attn_args(**kw)


@pytest.mark.parametrize("h,w,cross,shift", [(hw, hw, c, s) for hw in (64, 32, 128) for c in (False, True) for s in (0, 1)])
def test_eligible_points_plan_the_presplit_kernel_alone(h, w, cross, shift):
    a = attn(h, w, cross=cross, shift=shift)
    pl = L.attention_plan(a, kv_split=True)
    assert pl.kernel == b'attn_x3_presplit_kernel' and pl.scratch_bytes == 0
    assert pl.waves == 4 and pl.dvt == 4 and pl.nslices == 1 and pl.win_tables == 1
    Lk = h * w // 4
    assert pl.lds_bytes == (32 * (2 * C + 8) + C * 72) * 2 + Lk * 4 + (Lk // 32) * 16 + Lk and 2 * pl.lds_bytes <= 160 * 1024
    a.workspace, a.workspace_bytes = A, 1 << 40                     # a workspace changes nothing
    assert L.attention_plan(a, kv_split=True).kernel == b'attn_x3_presplit_kernel'
    # the core entry on the same arguments: the packed form, as before
    assert L.attention_plan(a).kernel == b'attn_pack_kv_x3_kernel<128, 128, false> + attn_x3_kernel<4, 4, 8, true, false>'


REFUSED = {
    'Lq % 128 != 0 (560-token windows)': dict(h=40, w=56),
    'Lk > 4096': dict(h=136, w=136),
    'single fp16': dict(mma=L.MMA_X1, flags=L.ATTN_X1),
    'f32 policy': dict(mma=L.MMA_F32),
    'bf16 policy': dict(mma=L.MMA_BF16),
    'exact-f32 override': dict(flags=L.ATTN_NO_X3),
    'mode 0': dict(mode=0, B=4, Lq=4096, Lk=4096),
    'two heads': dict(H=2, D=64, Dv=64),
    'D = 256': dict(D=256, Dv=256),
    'Dv = 2': dict(Dv=2),
    'range probes': dict(mode=0, B=4, Lq=4096, Lk=4096, q_amax=A, k_amax=A, v_amax=A),
    'k stride not in whole groups': dict(k_ts=3 * C + 4, k_bs=4096 * (3 * C + 4)),
    'misaligned v': dict(v=A + 4),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_calls_outside_the_rule_are_refused(what):
    over = dict(REFUSED[what])
    a = attn(over.pop('h', 64), over.pop('w', 64), **over)
    with pytest.raises(L.KeepHipError) as e:
        L.attention_plan(a, kv_split=True)
    assert e.value.code == L.EUNSUP and 'kv_split' in str(e.value), str(e.value)
    lib = L.load(check_device=False)
    assert lib.keep_attention_kv_split(ctypes.byref(a), None) == L.EUNSUP      # the launch's own answer, before anything is launched


def gemm(M=4096, N=384, c0=128, c1=384, **over):
    kw = dict(inp=A, weight=A, out=A, weight_x3=A, x3_acc_scale=1.0, N=1, H=M, W=1, Cin=C, Cout=N, KH=1, KW=1, stride=1, Ho=M, Wo=1, in_ld=C,
              out_ld=N, mma=L.MMA_X3, dtype=L.F32, out_dtype=L.F32)
    kw.update(over)
    return L.conv_args(**kw), (c0, c1)


def test_gemm_split_output_plans_the_existing_gemm_form():
    for M, N, c0 in itertools.product((384, 4096, 1 << 20), (256, 384), (0, 128)):
        a, cols = gemm(M, N, c0, N)
        assert L.conv2d_split_plan(a, cols).kernel == L.conv2d_plan(a).kernel and L.conv2d_split_plan(a, cols).split_k == 1 and L.conv2d_split_plan(a, cols).workspace_bytes == 0
        assert L.conv2d_launch_plan(a) in ('conv_x3_kernel<2, 2, 1, 1, true, true, false, true, false, false>',
                                           'conv_x3_kernel<2, 2, 2, 2, true, true, false, true, false, false>')


GEMM_REFUSED = {
    'range not a multiple of 128': dict(c1=320),
    'empty range': dict(c0=256, c1=256),
    'range past Cout': dict(c1=512),
    'Cout not a multiple of 128': dict(N=320, c0=0, c1=256),
    'out_ld not a multiple of 128': dict(out_ld=400),
    'rows not a multiple of 128': dict(M=4160),
    'residual': dict(residual=A, res_ld=384),
    'statistics': dict(stats_out=A, stats_P=64),
    'activation': dict(epi_act=L.ACT_GELU),
    'split-K': dict(split_k=2, workspace=A),
    'LayerNorm': dict(N=128, c0=0, c1=128, ln_gamma=A, ln_beta=A, ln_eps=1e-5),
    'prologue': dict(pro_act=L.PRO_RELU),
    '3x3': dict(KH=3, KW=3, pad_t=1, pad_l=1, H=64, W=64, Ho=64, Wo=64),
    'the latency form (K = 512, 256 rows per image)': dict(Cin=512, in_ld=512, M=256),
    'f32 policy': dict(mma=L.MMA_F32),
    'single fp16': dict(mma=L.MMA_X1, flags=L.CONV_X1_GEMM),
    'bf16 output': dict(mma=L.MMA_BF16, out_dtype=L.BF16, weight_bf16=A),
}


@pytest.mark.parametrize("what", sorted(GEMM_REFUSED))
def test_gemm_split_output_is_refused_elsewhere(what):
    a, cols = gemm(**GEMM_REFUSED[what])
    with pytest.raises(L.KeepHipError) as e:
        L.conv2d_split_plan(a, cols)
    assert e.value.code == L.EUNSUP, str(e.value)
    if what not in ('range past Cout', 'empty range', 'range not a multiple of 128', 'LayerNorm', 'split-K', 'single fp16'):
        L.conv2d_plan(a)                                             # the refusal was the split's: the same call without it plans


def test_entry_points_agree_between_header_binding_and_library():
    """The four entry points live in include/keep_cv_hip.h beside the frozen core header: no field was added to the argument structs."""
    header = open(os.path.join(ROOT, 'include', 'keep_cv_hip.h')).read()
    lib = L.load(check_device=False)
    for name, n_args in (('keep_conv2d_split', 4), ('keep_conv2d_split_plan', 4), ('keep_attention_kv_split', 2), ('keep_attention_kv_split_plan', 2)):
        proto = re.search(r'int32_t ' + name + r'\s*\(([^;]*)\);', header).group(1)
        assert len(proto.split(',')) == n_args == len(L._CV_SIGNATURES[name]) and name in L.CV_EXPORTED_SYMBOLS and name not in L.EXPORTED_SYMBOLS
        assert getattr(lib, name).argtypes == L._CV_SIGNATURES[name] and getattr(lib, name).restype is ctypes.c_int32
    assert L.ABI_VERSION == 23 and L.CV_ABI_VERSION == 1
    assert L.ConvArgs._fields_[-1][0] == 'plan_ref_images' and L.AttnArgs._fields_[-1][0] == 'workspace_bytes'
    out = L.ConvPlanOut()
    assert lib.keep_conv2d_split_plan(ctypes.byref(gemm()[0]), 0, 0, ctypes.byref(out)) == L.EINVAL      # an empty range is the core entry's business
    assert lib.keep_conv2d_split(None, 0, 128, None) == L.EINVAL and lib.keep_attention_kv_split(None, None) == L.EINVAL


def test_convolution_census_is_unchanged():
    """Fails early, ahead of tests/test_host_logic.py::test_conv_table_reaches_every_instantiation: the split output added a kernel symbol or a
    launch site to the five convolution sources."""
    assert U.launch_sites() == {'keep_conv.hip': 25, 'keep_conv_x3.hip': 20, 'keep_conv_x3s.hip': 5, 'keep_conv_x3p.hip': 9, 'keep_gemm_x3l.hip': 2}
    assert len(U.census()) == 169


def test_ops_asks_the_library_for_both_halves_of_the_decision(monkeypatch):
    """Ops.kv_split_ok: the attention plan AND the projection's split plan, each the library's own answer, cached per shape; a refusal of
    either (KEEP_EUNSUP) means the packed path, any other error propagates."""
    from comfyui_keep_amd.engine import ops
    o = ops.Ops()
    o.mma = o.attn_mma = L.MMA_X3
    Lt = 64 * 64
    shape = dict(B=16, Lq=Lt // 4, Lk=Lt // 4, D=C, Dv=C, q_str=(Lt * 3 * C, 3 * C, 0), k_str=(Lt * 3 * C, 3 * C, 0), v_str=(Lt * 3 * C, 3 * C, 0),
                 img_h=64, img_w=64, ksplit=2, shift=0, n_img=4)
    asked = []
    attn_plan, split_plan = L.attention_plan, L.conv2d_split_plan
    monkeypatch.setattr(L, 'attention_plan', lambda a, kv_split=False: (asked.append('attn'), attn_plan(a, kv_split=kv_split))[1])
    monkeypatch.setattr(L, 'conv2d_split_plan', lambda a, cols: (asked.append('gemm'), split_plan(a, cols))[1])
    assert o.kv_split_ok(**shape, gemm=(Lt, C, 3 * C, (C, 3 * C))) and asked == ['attn', 'gemm']
    assert o.kv_split_ok(**shape, gemm=(Lt, C, 3 * C, (C, 3 * C))) and asked == ['attn', 'gemm']            # cached
    assert not o.kv_split_ok(**shape, gemm=(Lt, C, 3 * C, (C, 320)))                                        # the GEMM refuses the range
    assert not o.kv_split_ok(**shape, gemm=(Lt, C, 320, (C, 256)))                                          # ... and a Cout that is no multiple of 128
    with pytest.raises(L.KeepHipError) as e:                                                                # a bad call is an error, not a `no`
        o.kv_split_ok(**shape, gemm=(Lt, 0, 3 * C, (C, 3 * C)))
    assert e.value.code == L.EINVAL
