"""GPU suite (-m gpu): GMFlow window attention without the K / V pack pass (KEEP_MMA_X3).

The projection GEMM writes k and v as split-fp16 halves (keep_conv2d_split: per 128-column group [hi x 128 | lo x 128] in
the 512 bytes of the 128 floats) and keep_attention_kv_split reads them (attn_x3_presplit_kernel: window rows gathered through
the LDS pixel table, V through the transposed LDS read).  Every MFMA sees the operand bits the packed path gives it, so the results are
held to ``torch.equal`` against the packed path on the fp32 tensor of the same GEMM, and to the suite's x3 yardstick against fp64.
"""
import math

import pytest
import torch

from abi_ref import win_ref, win_regions, win_shift, win_split, yardstick
import keep_oracle as O
from comfyui_keep_amd.engine import hiplib as L
from comfyui_keep_amd.engine import ops, synth

pytestmark = pytest.mark.gpu
C = 128


def randn(seed, shape, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float32) * scale


def gemm(x, w, split_cols=None, **kw):
    """x [M, 128] @ w[N, 128]^T on the x3 GEMM form with a twin built here (scale 1: the weights are of order 1)."""
    y = ops.conv(x.view(1, -1, 1, x.shape[-1]), w, None, stride=1, pad=0, ksize=1, mma=L.MMA_X3, wx3=ops.split_x3(w, 1.0).view(-1),
                 x3_acc_scale=1.0, bounded=True, split_cols=split_cols, **kw)
    torch.cuda.synchronize()
    return y.view(-1, w.shape[0])


def halves(y, g):
    """(hi, lo) [M, 128] fp16 of 128-column group g of a split output."""
    h = y.view(torch.float16).view(y.shape[0], -1)
    return h[:, g * 256:g * 256 + 128], h[:, g * 256 + 128:g * 256 + 256]


def same_bits(a, b):
    """Equal bit for bit where neither is NaN, and NaN in the same places (a NaN's payload is not part of the contract)."""
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(torch.where(na, torch.zeros_like(a), a).view(torch.int16), torch.where(nb, torch.zeros_like(b), b).view(torch.int16))


# ------------------------------------------------------------------------------------------------ the GEMM's halves
@pytest.mark.parametrize("M", [4 * 1024, 3 * 128, 65 * 128])
@pytest.mark.parametrize("N,c0", [(384, 128), (256, 0)])
def test_gemm_halves_are_the_packs_split_of_the_unsplit_output(M, N, c0):
    """Columns outside [c0, N) equal the un-split launch; inside, hi = (fp16)y and lo = (fp16)(y - (float)hi) of its output -- the pack
    kernel's split, inf / NaN included: one output of 384000 (hi = inf, lo = -inf) and one NaN input row.  M = 4096 and M = 384 (a multiple
    of 128, not of 256) launch the 64 x 64 tile, M = 8320 (the same) the 128 x 128 tile."""
    x, w = randn(M + N, (M, C)), randn(N, (N, C), 1.0 / math.sqrt(C))
    x[5], w[c0 + 7] = 100.0, 30.0            # y[5, c0 + 7] = 128 * 3000
    x[9, 3] = float('nan')
    x, w = x.cuda(), w.cuda()
    y, ys = gemm(x, w), gemm(x, w, split_cols=(c0, N))
    assert y[5, c0 + 7].item() == 384000.0 and torch.isnan(y[9]).all()
    if c0:
        yq, ysq = y[:, :c0], ys[:, :c0]
        assert torch.equal(torch.isnan(yq), torch.isnan(ysq)) and torch.equal(yq.nan_to_num(0.0), ysq.nan_to_num(0.0))
    for g in range(c0 // 128, N // 128):
        yg = y[:, g * 128:(g + 1) * 128]
        hi = yg.half()
        lo = (yg - hi.float()).half()
        got_hi, got_lo = halves(ys, g)
        assert same_bits(got_hi, hi) and same_bits(got_lo, lo), g
    assert torch.isinf(halves(ys, (c0 + 7) // 128)[0][5, 7]) and torch.isinf(halves(ys, (c0 + 7) // 128)[1][5, 7])


@pytest.mark.parametrize("what", ['statistics', 'residual', 'range'])
def test_gemm_refuses_an_ineligible_split(what):
    x, w = randn(1, (1024, C)).cuda(), randn(2, (256, C), 0.1).cuda()
    kw = dict(stats=True) if what == 'statistics' else dict(residual=torch.zeros(1, 1024, 1, 256, device='cuda')) if what == 'residual' else {}
    with pytest.raises(L.KeepHipError) as e:
        gemm(x, w, split_cols=(0, 192) if what == 'range' else (0, 256), **kw)
    assert e.value.code == L.EUNSUP and 'keep_conv2d_split' in str(e.value)


# ------------------------------------------------------------------------------------------------ attention on the split tensor
def gm_gemm_call(h, w, P, shift, cross, seed):
    """``gm_call`` of tests/test_gpu_attention_modes.py with q / k / v coming out of the projection GEMM, as net.py:_gm_layer launches them:
    (fp32 tensors, split tensors, host q / k / v, keyword arguments)."""
    n_img, Lt, ks = 2 * P, h * w, 2
    wqkv = randn(seed + 2, (3 * C, C), 1.0 / math.sqrt(C))
    wqkv[:C] *= 1.5
    wqkv = wqkv.cuda()
    src = randn(seed, (n_img * Lt, C)).cuda()
    if cross:
        tgt = randn(seed + 1, (n_img * Lt, C)).cuda()
        q = gemm(src, wqkv[:C])
        kv, kvs = gemm(tgt, wqkv[C:]), gemm(tgt, wqkv[C:], split_cols=(0, 2 * C))
        dev = (q, kv, ops.offset(kv, C))
        devs = (q, kvs, ops.offset(kvs, C))
        sq, skv = (Lt * C, C, 0), (Lt * 2 * C, 2 * C, 0)
        host = (q.cpu().view(n_img, Lt, C), kv.cpu().view(n_img, Lt, 2 * C)[..., :C], kv.cpu().view(n_img, Lt, 2 * C)[..., C:])
    else:
        qkv, qkvs = gemm(src, wqkv), gemm(src, wqkv, split_cols=(C, 3 * C))
        assert torch.equal(qkv[:, :C], qkvs[:, :C])
        dev = (qkv, ops.offset(qkv, C), ops.offset(qkv, 2 * C))
        devs = (qkvs, ops.offset(qkvs, C), ops.offset(qkvs, 2 * C))
        sq = skv = (Lt * 3 * C, 3 * C, 0)
        host = tuple(t.contiguous() for t in qkv.cpu().view(n_img, Lt, 3 * C).split(C, dim=-1))
    kw = dict(B=n_img * ks * ks, H=1, Lq=Lt // (ks * ks), Lk=Lt // (ks * ks), D=C, Dv=C, scale=1.0 / math.sqrt(C), q_str=sq, k_str=skv, v_str=skv,
              o_str=(Lt * C, C, 0), mode=2, img_h=h, img_w=w, ksplit=ks, shift=(h // ks // 2) if shift else 0, kv_rot=P if cross else 0, n_img=n_img)
    return dev, devs, host, kw


def attend(qkv, kw, mma=L.MMA_X3, **extra):
    o = torch.empty((kw['n_img'] * kw['img_h'] * kw['img_w'], C), device='cuda')
    ops.attention(*qkv, o, mma=mma, **kw, **extra)
    torch.cuda.synchronize()
    return o


def plan_of(qkv, kw, kv_split=False, **extra):
    q, k, v = qkv
    (qb, qt, qh), (kb, kt, kh), (vb, vt, vh), (ob, ot, oh) = kw['q_str'], kw['k_str'], kw['v_str'], kw['o_str']
    rest = {n: kw[n] for n in ('B', 'H', 'Lq', 'Lk', 'D', 'Dv', 'scale', 'mode', 'img_h', 'img_w', 'ksplit', 'shift', 'kv_rot', 'n_img')}
    a = L.attn_args(q=q, k=k, v=v, o=q, q_bs=qb, q_ts=qt, q_hs=qh, k_bs=kb, k_ts=kt, k_hs=kh, v_bs=vb, v_ts=vt, v_hs=vh, o_bs=ob, o_ts=ot, o_hs=oh,
                    in_dtype=L.F32, **dict(dict(mma=L.MMA_X3), **rest, **extra))
    return L.attention_plan(a, kv_split=kv_split)


PRESPLIT_CASES = ([(64, 64, 2, s, c) for s in (0, 1) for c in (False, True)] + [(32, 32, 2, s, c) for s in (0, 1) for c in (False, True)] +
                  [(64, 64, 3, 1, True), (32, 32, 3, 0, True)])


@pytest.mark.parametrize("h,w,P,shift,cross", PRESPLIT_CASES)
def test_presplit_attention_equals_the_packed_path_bit_for_bit(h, w, P, shift, cross):
    """64 x 64 tokens: 1024-token windows; 32 x 32: 256-token windows; shift 0 / half a window, self- and cross-attention, P = 3 with the
    kv_rot wrap-around.  attn_x3_presplit_kernel on the split tensor == attn_pack_kv_x3_kernel + attn_x3_kernel<4,4,8,true> on the fp32
    tensor of the same GEMM, and the suite's yardstick against the fp64 window reference: err_x3 <= max(3 err_f32, 2e-6 scale)."""
    dev, devs, host, kw = gm_gemm_call(h, w, P, shift, cross, seed=31 * h + 7 * P + 2 * shift + cross)
    assert plan_of(devs, kw, kv_split=1).kernel == b'attn_x3_presplit_kernel' and plan_of(devs, kw, kv_split=1).scratch_bytes == 0
    assert plan_of(dev, kw, workspace=0x10000, workspace_bytes=1 << 40).kernel.startswith(b'attn_pack_kv_x3_kernel<128, 128, false> + ')
    o_pack, o_new = attend(dev, kw), attend(devs, kw, kv_split=True)
    assert torch.isfinite(o_new).all() and torch.equal(o_new, o_pack)
    n_img, Lw = 2 * P, kw['Lq']
    step = max(1, Lw // 128)
    rows = torch.unique(torch.cat([torch.arange(step // 2, Lw, step), torch.tensor([0, Lw - 1])]))
    ref = win_ref(*host, h, w, 2, shift, kw['kv_rot'], rows)
    sy, sx = win_shift(h, w, 2, shift)
    cut = lambda o: win_split(o.view(n_img, h * w, -1).cpu(), h, w, 2, sy, sx)[:, rows]  # noqa: E731
    err = lambda o: (cut(o).double() - ref).abs().max().item()  # noqa: E731
    yardstick(f'pre-split {h}x{w} P={P} shift={kw["shift"]} cross={cross}', err(o_new), err(attend(dev, kw, mma=L.MMA_F32)), ref.abs().max().item())


def test_presplit_mask_is_the_reference_additive_minus_100():
    """The planted cross-region key of test_gpu_attention_modes.py::test_mode2_mask_is_the_reference_additive_minus_100 (same construction:
    one query of the bottom-right window of a shifted 32 x 32 grid meets one key of another region whose score exceeds every same-region
    score by 60 - 120) through the pre-split form, same bound.  The tensor is split here as the GEMM splits it."""
    h = w = 32
    ks, P = 2, 3
    n_img, Lw, wh = 2 * P, 256, 16
    sy, sx = win_shift(h, w, ks, True)
    excess = torch.tensor([60.0, 80.0, 95.0, 100.0, 105.0, 120.0], dtype=torch.float64)
    qw, kw_, vw = randn(5, (n_img, 4, Lw, C), 0.3), randn(6, (n_img, 4, Lw, C), 0.3), randn(7, (n_img, 4, Lw, C))
    tq, tk = 2 * wh + 2, 12 * wh + 12
    reg = win_regions(h, w, ks)
    assert reg[3, tq] != reg[3, tk]
    u = randn(8, (C,)).sign()
    qw[:, 3, tq] = u
    for i in range(n_img):
        kw_[i, 3, tk] = u * (round(float(excess[i]) * math.sqrt(C) / C * 64.0) / 64.0)
    vw[:, 3, tk, :] = 8.0

    def to_image(t):
        img = O._merge_cl(t.reshape(n_img * 4, wh, wh, C), ks)
        return torch.roll(img, shifts=(sy, sx), dims=(1, 2)).reshape(n_img, h * w, C)

    qh, kh, vh = to_image(qw), to_image(kw_), to_image(vw)
    qd = torch.cat([qh, kh, vh], dim=-1).reshape(n_img * h * w, 3 * C).cuda()
    qs = qd.clone()
    for g in (1, 2):                         # k and v as [hi x 128 | lo x 128]
        yg = qd[:, g * C:(g + 1) * C]
        hi = yg.half()
        qs[:, g * C:(g + 1) * C] = torch.cat([hi, (yg - hi.float()).half()], dim=-1).view(torch.float32)
    s3 = (h * w * 3 * C, 3 * C, 0)
    kw = dict(B=n_img * 4, H=1, Lq=Lw, Lk=Lw, D=C, Dv=C, scale=1.0 / math.sqrt(C), q_str=s3, k_str=s3, v_str=s3,
              o_str=(h * w * C, C, 0), mode=2, img_h=h, img_w=w, ksplit=ks, shift=wh // 2, kv_rot=0, n_img=n_img)
    ref = win_ref(qh, kh, vh, h, w, ks, True, 0, torch.arange(Lw))
    cut = lambda o: win_split(o.view(n_img, h * w, C).cpu(), h, w, ks, sy, sx)  # noqa: E731
    err = lambda o: (cut(o).double() - ref).abs().max().item()  # noqa: E731
    dev = (qd, ops.offset(qd, C), ops.offset(qd, 2 * C))
    o_new = attend((qs, ops.offset(qs, C), ops.offset(qs, 2 * C)), kw, kv_split=True)
    assert torch.equal(o_new, attend(dev, kw))
    yardstick('pre-split mask semantics', err(o_new), err(attend(dev, kw, mma=L.MMA_F32)), ref.abs().max().item())


# ------------------------------------------------------------------------------------------------ fall-backs
def test_ineligible_shapes_keep_the_packed_path(monkeypatch):
    """40 x 56 tokens (560-token windows, Lq % 128 != 0) and a single-fp16 call: the plan refuses kv_split (KEEP_EUNSUP), Ops.kv_split_ok says
    no, and the call without kv_split plans the packed form as before."""
    dev, _, _, kw = gm_gemm_call(40, 56, 2, 1, False, seed=3)
    with pytest.raises(L.KeepHipError) as e:
        plan_of(dev, kw, kv_split=1)
    assert e.value.code == L.EUNSUP and 'kv_split' in str(e.value)
    shape = {n: kw[n] for n in ('B', 'Lq', 'Lk', 'D', 'Dv', 'q_str', 'k_str', 'v_str', 'img_h', 'img_w', 'ksplit', 'shift', 'n_img')}
    monkeypatch.setattr(ops.DEFAULT, 'attn_mma', L.MMA_X3)
    assert not ops.DEFAULT.kv_split_ok(**shape)
    assert plan_of(dev, kw, workspace=0x10000, workspace_bytes=1 << 40).kernel.startswith(b'attn_pack_kv_x3_kernel<128, 128, false> + ')
    assert torch.isfinite(attend(dev, kw)).all()
    dev, _, _, kw = gm_gemm_call(32, 32, 2, 0, False, seed=4)
    with pytest.raises(L.KeepHipError) as e:
        plan_of(dev, kw, kv_split=1, mma=L.MMA_X1, flags=L.ATTN_X1)
    assert e.value.code == L.EUNSUP and 'kv_split' in str(e.value)
    assert ops.DEFAULT.kv_split_ok(**{n: kw[n] for n in shape})


# ------------------------------------------------------------------------------------------------ the network
def test_gmflow_clip_is_bit_equal_with_and_without_the_presplit_path(gpu_net, monkeypatch):
    """KeepNet._gmflow_clip on two clips of T = 3 at 256 x 256 (32 x 32 features and their 64 x 64 refinement): the pre-split path against the
    same call with its knob off.  Under the x3 policy every eligible layer takes the new path (and the knob removes it); fp32 never does."""
    x = synth.synth_clip(T=3, B=2, size=256, seed=11).cuda()
    seen = []
    real = gpu_net.of.attention
    monkeypatch.setattr(gpu_net.of, 'attention', lambda *a, **k: (seen.append(bool(k.get('kv_split'))), real(*a, **k))[1])
    monkeypatch.setattr(ops, 'ATTN_PRESPLIT', True)
    f_new, n_new = gpu_net._gmflow_clip(x), sum(seen)
    del seen[:]
    monkeypatch.setattr(ops, 'ATTN_PRESPLIT', False)
    f_old = gpu_net._gmflow_clip(x)
    assert not any(seen) and torch.isfinite(f_new).all() and torch.equal(f_new, f_old)
    assert (n_new > 0) == (gpu_net.of.mma == L.MMA_X3), (n_new, gpu_net.of.mma)


def test_gmflow_clip_at_an_ineligible_size_stays_on_the_packed_path(gpu_net, monkeypatch):
    """A 320 x 448 clip: 40 x 56 features, 560-token windows (Lq % 128 != 0).  With the knob on, ``_gm_layer`` asks, the plan refuses, and
    every window-attention call goes out without kv_split on the fp32 projections -- the same bits as with the knob off."""
    x = synth.synth_clip(T=2, B=1, size=448, seed=5)[..., :320, :].contiguous().cuda()
    seen = []
    real = gpu_net.of.attention
    monkeypatch.setattr(gpu_net.of, 'attention', lambda *a, **k: (seen.append((k.get('mode', 0), k['Lq'], bool(k.get('kv_split')))), real(*a, **k))[1])
    monkeypatch.setattr(ops, 'ATTN_PRESPLIT', True)
    f_on = gpu_net._gmflow_clip(x)
    assert (2, 560, False) in seen and not any(s for _, _, s in seen), seen
    monkeypatch.setattr(ops, 'ATTN_PRESPLIT', False)
    assert torch.isfinite(f_on).all() and torch.equal(f_on, gpu_net._gmflow_clip(x))
