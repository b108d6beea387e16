"""GPU suite (-m gpu): keep_attention in every token-addressing mode the product launches, on the split-fp16 (KEEP_MMA_X3)
kernels, against fp64 references built here.  The suite's x3 yardstick for every case:

    err_f32 <= 2e-4 * scale             (the exact-f32 kernel: re-association only)
    err_x3  <= max(3 * err_f32, 2e-6 * scale)

errors = max |out - fp64 reference| over the compared rows, scale = max |reference|.  Where the packed K / V^T path is the
default (x3, D in {128, 256}, Lq >= 256: keep_attn.hip attn_pack_bytes) the un-packed x3 kernel (KEEP_ATTN_NO_PACK) is held to
the same bound.  Attention launches are not recorded in ``ops.DEFAULT.profile``: each docstring names the kernel the case is
meant to reach through the dispatch at the end of keep_attention (rocprofv3 --kernel-trace confirms the names).

Mode 2 references roll / split / mask in the reference's own way (GM/transformer.py:46-105, roll by (wh/2, ww/2));
``test_window_regions_match_the_reference_mask`` ties the region ids used here to keep_oracle.shift_window_mask, which
tests/test_oracle_vs_golden.py pins against the imported reference on square and non-square grids.
"""
import ctypes
import math

import pytest
import torch

import keep_oracle as O
from abi_ref import sparse_causal_ref, win_ref, win_regions, win_shift, win_split, yardstick      # the one fp64 restatement of the modes
from comfyui_keep_amd.engine import hiplib as L
from comfyui_keep_amd.engine import ops

pytestmark = pytest.mark.gpu
TOL = 2e-4
LOG2E = 1.4426950408889634


def randn(seed, shape, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float32) * scale


def err64(got, ref64):
    return (got.detach().double().cpu() - ref64).abs().max().item()


def launch(q, k, v, o_shape, mma, flags=0, **kw):
    o = torch.empty(o_shape, device='cuda')
    ops.DEFAULT.attn_flags = flags
    try:
        ops.attention(q, k, v, o, mma=mma, **kw)
    finally:
        ops.DEFAULT.attn_flags = 0
    torch.cuda.synchronize()
    return o


def workspace_bytes(q, k, v, mma, flags=0, *, q_str, k_str, v_str, o_str, **kw):
    """keep_attention_workspace_bytes for this call: > 0 iff the library will take the packed K / V^T path (or two passes)."""
    a = L.AttnArgs()
    a.struct_size = ctypes.sizeof(L.AttnArgs)
    fields = dict(q=q.data_ptr(), k=k.data_ptr(), v=v.data_ptr(), o=None, q_bs=q_str[0], q_ts=q_str[1], q_hs=q_str[2],
                  k_bs=k_str[0], k_ts=k_str[1], k_hs=k_str[2], v_bs=v_str[0], v_ts=v_str[1], v_hs=v_str[2],
                  o_bs=o_str[0], o_ts=o_str[1], o_hs=o_str[2], mma=mma, in_dtype=L.F32, flags=flags, **kw)
    for key, val in fields.items():
        setattr(a, key, val)
    return L.attention_workspace_bytes(a)


def sample_rows(L_, n=256):
    """~n query rows spread over [0, L_) with the last one included (ragged tail tiles)."""
    step = max(1, L_ // n)
    idx = torch.arange(step // 2, L_, step)
    return torch.unique(torch.cat([idx, torch.tensor([0, L_ - 1])]))


# ------------------------------------------------------------------------------------------------ mode 2: shifted windows
def gm_call(h, w, P, shift, cross, C=128, ks=2, amp=1.5, seed=0):
    """GMFlow window attention as net.py:_gm_layer launches it: self-attention reads q | k | v from one packed [Ltok, 3C]
    buffer (kv_rot = 0), cross-attention a separate q and a [Ltok, 2C] k | v buffer (kv_rot = P: [f0;f1] vs [f1;f0])."""
    n_img, Lt = 2 * P, h * w
    wh = h // ks
    sh = wh // 2 if shift else 0
    if cross:
        qb, kvb = randn(seed, (n_img * Lt, C), amp), randn(seed + 1, (n_img * Lt, 2 * C))
        qd, kvd = qb.cuda(), kvb.cuda()
        q, k, v = qd, kvd, ops.offset(kvd, C)
        sq, skv = (Lt * C, C, 0), (Lt * 2 * C, 2 * C, 0)
        host = (qb.view(n_img, Lt, C), kvb.view(n_img, Lt, 2 * C)[..., :C], kvb.view(n_img, Lt, 2 * C)[..., C:])
        kv_rot = P
    else:
        qkv = randn(seed, (n_img * Lt, 3 * C))
        qkv[:, :C] *= amp
        qd = qkv.cuda()
        q, k, v = qd, ops.offset(qd, C), ops.offset(qd, 2 * C)
        sq = skv = (Lt * 3 * C, 3 * C, 0)
        host = tuple(t.contiguous() for t in qkv.view(n_img, Lt, 3 * C).split(C, dim=-1))
        kv_rot = 0
    kw = dict(B=n_img * ks * ks, H=1, Lq=Lt // (ks * ks), Lk=Lt // (ks * ks), D=C, Dv=C, scale=1.0 / math.sqrt(C),
              q_str=sq, k_str=skv, v_str=skv, o_str=(Lt * C, C, 0), mode=2, img_h=h, img_w=w, ksplit=ks, shift=sh,
              kv_rot=kv_rot, n_img=n_img)
    return (q, k, v), host, kw, kv_rot


def run_yardstick(dev_qkv, o_shape, kw, cut, ref, what, packed):
    """x3, f32 and (where the packed path is the default) un-packed x3 against the fp64 reference; `cut` maps a kernel output
    to the compared rows."""
    q, k, v = dev_qkv
    outs = {}
    for name, mma, flags in (('x3', L.MMA_X3, 0), ('f32', L.MMA_F32, 0)) + ((('x3np', L.MMA_X3, L.ATTN_NO_PACK),) if packed else ()):
        o = launch(q, k, v, o_shape, mma, flags, **kw)
        assert torch.isfinite(o).all(), f'{what} {name}: non-finite output'
        outs[name] = err64(cut(o), ref)
    sc = ref.abs().max().item()
    yardstick(what, outs['x3'], outs['f32'], sc, outs.get('x3np'))
    return outs


def test_window_regions_match_the_reference_mask():
    """The region ids of win_ref give keep_oracle.shift_window_mask (pinned against the reference, non-square included)."""
    for h, w in ((8, 8), (40, 56), (56, 40), (32, 32)):
        reg = win_regions(h, w, 2)
        m = torch.where(reg[:, :, None] != reg[:, None, :], -100.0, 0.0)
        assert torch.equal(m.transpose(1, 2), O.shift_window_mask(h, w, h // 2, w // 2, h // 4, w // 4)), (h, w)


GM_CASES = ([(64, 64, P, s, c) for P in (2, 3) for s in (0, 1) for c in (False, True)] +
            [(32, 32, 2, s, c) for s in (0, 1) for c in (False, True)] +
            [(hw[0], hw[1], 2, s, c) for hw in ((40, 56), (56, 40)) for s in (0, 1) for c in (False, True)] +
            [(8, 8, 2, s, c) for s in (0, 1) for c in (False, True)])


@pytest.mark.parametrize("h,w,P,shift,cross", GM_CASES)
def test_mode2_gmflow_windows_x3(h, w, P, shift, cross):
    """GMFlow shifted-window attention (mode 2, D = Dv = 128, H = 1, ksplit = 2, n_img = 2P).
    Windows of >= 256 tokens (64x64: 1024 with the LDS window tables, Lk <= 4096; 32x32: 256 = gmflow256; 40x56 / 56x40: 560,
    a ragged last key tile, ww = 28 / 20 not a power of two, and a per-axis shift (10, 14) / (14, 10)): the packed path,
    attn_pack_kv_x3_kernel<128,128> + attn_x3_kernel<4,4,8,true>, and with KEEP_ATTN_NO_PACK attn_x3_kernel<4,4,8,false>.
    8x8 (16-token windows, Lq <= 32): the one-wave attn_x3_kernel<1,4,8,false>.  Cross-attention with P = 3 wraps kv_rot."""
    (q, k, v), (qh, kh, vh), kw, kv_rot = gm_call(h, w, P, shift, cross, seed=1000 * h + w + 10 * P + 2 * shift + cross)
    n_img, Lw = 2 * P, kw['Lq']
    packed = Lw >= 256
    assert (workspace_bytes(q, k, v, L.MMA_X3, **kw) > 0) == packed
    if packed:
        assert workspace_bytes(q, k, v, L.MMA_X3, L.ATTN_NO_PACK, **kw) == 0
    rows = sample_rows(Lw)
    ref = win_ref(qh, kh, vh, h, w, 2, shift, kv_rot, rows)
    sy, sx = win_shift(h, w, 2, shift)
    cut = lambda o: win_split(o.view(n_img, h * w, -1).cpu(), h, w, 2, sy, sx)[:, rows]  # noqa: E731
    run_yardstick((q, k, v), (n_img * h * w, 128), kw, cut, ref, f'mode2 {h}x{w} P={P} shift={kw["shift"]} cross={cross}', packed)


@pytest.mark.parametrize("shift", [0, 1])
def test_mode2_windows_without_tables_x3(shift):
    """136x136 grid, 4624-token windows (Lk > 4096): the packed x3 kernel WITHOUT the LDS window tables (region ids and pixels
    recomputed per key tile: win_region / kv_offset), attn_pack_kv_x3_kernel<128,128> + attn_x3_kernel<4,4,8,true>; un-packed
    attn_x3_kernel<4,4,8,false>.  A sample of query rows of every window is referenced."""
    h = w = 136
    (q, k, v), (qh, kh, vh), kw, kv_rot = gm_call(h, w, 2, shift, True, seed=77 + shift)
    assert kw['Lk'] == 4624 and workspace_bytes(q, k, v, L.MMA_X3, **kw) > 0
    rows = sample_rows(kw['Lq'], 160)
    ref = win_ref(qh, kh, vh, h, w, 2, shift, kv_rot, rows)
    sy, sx = win_shift(h, w, 2, shift)
    cut = lambda o: win_split(o.view(4, h * w, -1).cpu(), h, w, 2, sy, sx)[:, rows]  # noqa: E731
    run_yardstick((q, k, v), (4 * h * w, 128), kw, cut, ref, f'mode2 {h}x{w} shift={kw["shift"]} (no tables)', True)


def test_mode2_mask_is_the_reference_additive_minus_100():
    """Mask semantics (GM/transformer.py:24-35,91-92): -100 ADDED to the natural-log-domain score of a cross-region pair, not an
    exclusion.  In the bottom-right window of a shifted 32x32 grid (four regions), one query gets one key of ANOTHER region whose
    score exceeds every same-region score by 60 - 120 (one excess per image): after the -100 the planted key is anything from
    negligible to dominant.  Excluding the key, or adding -100 in the exp2 domain (-69.3 in natural units) or scaling it by
    log2 e twice (-144), moves these rows far beyond the bound (checked on the fp64 model below).  The planted score is spread
    over all 128 channels (q = u, k = beta u, u a sign vector, beta a multiple of 1/64: exact in fp16), as aligned features
    produce it.  Carried by ONE channel (16 x 74.25, both exact in fp16) the same score left the x3 kernel at 17x the f32
    kernel's error on that row (9e-5 at scale 8): the loss is in summing a dot product one term dominates, not in the mask.  Packed attn_x3_kernel<4,4,8,true> (256-token windows), un-packed attn_x3_kernel<4,4,8,false>, and the f32 kernel."""
    h = w = 32
    ks, C, P = 2, 128, 3
    n_img, Lw, wh = 2 * P, 256, 16
    sy, sx = win_shift(h, w, ks, True)
    excess = torch.tensor([60.0, 80.0, 95.0, 100.0, 105.0, 120.0], dtype=torch.float64)
    # window-frame tensors [n_img, k2, Lw, C]: small scores everywhere except the planted pair of window 3
    qw, kw_, vw = randn(5, (n_img, 4, Lw, C), 0.3), randn(6, (n_img, 4, Lw, C), 0.3), randn(7, (n_img, 4, Lw, C))
    tq, tk = 2 * wh + 2, 12 * wh + 12        # rolled-frame (18, 18): region 4; (28, 28): region 8
    reg = win_regions(h, w, ks)
    assert reg[3, tq] != reg[3, tk]
    u = randn(8, (C,)).sign()
    qw[:, 3, tq] = u
    for i in range(n_img):
        kw_[i, 3, tk] = u * (round(float(excess[i]) * math.sqrt(C) / C * 64.0) / 64.0)
    vw[:, 3, tk, :] = 8.0

    def to_image(t):               # window frame -> image frame [n_img, h*w, C] (merge, roll back by (sy, sx))
        img = O._merge_cl(t.reshape(n_img * 4, wh, wh, C), ks)
        return torch.roll(img, shifts=(sy, sx), dims=(1, 2)).reshape(n_img, h * w, C)

    qh, kh, vh = to_image(qw), to_image(kw_), to_image(vw)
    s_all = torch.matmul(qw[:, 3, tq].double()[:, None, :], kw_[:, 3].double().transpose(1, 2))[:, 0] / math.sqrt(C)
    same = reg[3] == reg[3, tq]
    gap = s_all[:, tk] - s_all[:, same].max(dim=1).values
    assert ((gap - excess).abs() < 3.0).all(), gap
    qkv = torch.cat([qh, kh, vh], dim=-1).reshape(n_img * h * w, 3 * C)
    qd = qkv.cuda()
    s3 = (h * w * 3 * C, 3 * C, 0)
    kw = dict(B=n_img * 4, H=1, Lq=Lw, Lk=Lw, D=C, Dv=C, scale=1.0 / math.sqrt(C), q_str=s3, k_str=s3, v_str=s3,
              o_str=(h * w * C, C, 0), mode=2, img_h=h, img_w=w, ksplit=ks, shift=wh // 2, kv_rot=0, n_img=n_img)
    rows = torch.arange(Lw)
    ref = win_ref(qh, kh, vh, h, w, ks, True, 0, rows)
    sc = ref.abs().max().item()
    # the case discriminates: each wrong mask semantics moves the planted rows by far more than the bound
    planted = ref.view(n_img, 4, Lw, C)[:, 3, tq]
    for wrong in (-math.inf, -100.0 / LOG2E, -100.0 * LOG2E):
        alt = win_ref(qh, kh, vh, h, w, ks, True, 0, torch.tensor([tq]), mask_value=wrong).view(n_img, 4, 1, C)[:, 3, 0]
        assert (alt - planted).abs().max().item() > 0.5, wrong
    cut = lambda o: win_split(o.view(n_img, h * w, C).cpu(), h, w, ks, sy, sx)  # noqa: E731
    run_yardstick((qd, ops.offset(qd, C), ops.offset(qd, 2 * C)), (n_img * h * w, C), kw, cut, ref, 'mode2 mask semantics', True)


# ------------------------------------------------------------------------------------------------ mode 0: GMFlow soft-argmax
@pytest.mark.parametrize("h,w,fs,vkind", [(64, 64, 0.5, 'grid'), (64, 64, 2.5, 'grid'), (64, 64, 0.5, 'flow'), (64, 64, 2.5, 'flow'),
                                          (40, 56, 2.5, 'grid'), (40, 56, 2.5, 'flow')])
def test_mode0_softargmax_and_flow_propagation_x3(h, w, fs, vkind):
    """GMFlow global-correlation soft-argmax (V = the pixel grid shared by all pairs, v_str = (0, 2, 0), GM/matching.py:15-34) and
    flow propagation (V = the per-pair flow, v_str = (Ltok*2, 2, 0), GM/transformer.py:363-372) as net.py launches them: P = 2,
    D = 128, Dv = 2.  Physical features: f1 = f0 rolled by (2, -3) px + noise; fs = 2.5 makes the scores span > 50 (peaked).
    Lq >= 256, Dv <= 32: attn_pack_kv_x3_kernel<128,32> + attn_x3_kernel<4,1,8,true>; un-packed attn_x3_kernel<4,1,8,false>.
    Errors are in pixels."""
    P, C = 2, 128
    Lt = h * w
    f0 = randn(11 + h, (P, h, w, C), fs)
    f1 = torch.roll(f0, shifts=(2, -3), dims=(1, 2)) + randn(12 + h, (P, h, w, C), 0.3 * fs)
    f0, f1 = f0.reshape(P, Lt, C), f1.reshape(P, Lt, C)
    gy, gx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing='ij')
    grid = torch.stack([gx, gy], dim=-1).reshape(Lt, 2)
    if vkind == 'grid':
        vh, v_str = grid[None].expand(P, Lt, 2), (0, 2, 0)
        vd = grid.cuda()
    else:
        vflow = randn(13 + h, (P, Lt, 2), 3.0)
        vh, v_str = vflow, (Lt * 2, 2, 0)
        vd = vflow.cuda()
    sF = (Lt * C, C, 0)
    kw = dict(B=P, H=1, Lq=Lt, Lk=Lt, D=C, Dv=2, scale=1.0 / math.sqrt(C), q_str=sF, k_str=sF, v_str=v_str, o_str=(Lt * 2, 2, 0))
    q, k = f0.cuda(), f1.cuda()
    assert workspace_bytes(q, k, vd, L.MMA_X3, **kw) > 0
    rows = sample_rows(Lt, 512)
    s = torch.matmul(f0.double()[:, rows], f1.double().transpose(1, 2)) / math.sqrt(C)
    span = (s.max(-1).values - s.min(-1).values).min().item()
    if fs > 1:
        assert span > 50, span
    ref = torch.matmul(torch.softmax(s, dim=-1), vh.double())
    cut = lambda o: o.view(P, Lt, 2).cpu()[:, rows]  # noqa: E731
    outs = run_yardstick((q, k, vd), (P * Lt, 2), kw, cut, ref, f'mode0 {h}x{w} fs={fs} V={vkind} (px)', True)
    print(f'[mode0 px] {h}x{w} fs={fs} V={vkind}: score span >= {span:.1f}, x3 {outs["x3"]:.3e} px, f32 {outs["f32"]:.3e} px')


# ------------------------------------------------------------------------------------------------ mode 1: Kalman sparse-causal
def sparse_causal_call(Bc, T, Lt, H, D, seed, amp=1.5):
    inner = H * D
    qkv = randn(seed, (Bc * T, Lt, 3 * inner))
    qkv[..., :inner] *= amp
    qd = qkv.cuda()
    s3 = (Lt * 3 * inner, 3 * inner, D)
    kw = dict(B=Bc * T, H=H, Lq=Lt, Lk=2 * Lt, D=D, Dv=D, scale=D ** -0.5, q_str=s3, k_str=s3, v_str=s3,
              o_str=(Lt * inner, inner, D), mode=1, T=T, seg_len=Lt)
    return qkv, (qd, ops.offset(qd, inner), ops.offset(qd, 2 * inner)), kw


@pytest.mark.parametrize("Lt", [256, 200])
@pytest.mark.parametrize("T", [1, 2, 3, 20])
def test_mode1_kalman_sparse_causal_x3(T, Lt):
    """Kalman sparse-causal attention as net.py launches it (packed qkv, H = 8, D = Dv = 48, Lk = 2 Ltok), Bc = 2 clips: the
    latent's 256 tokens and a ragged 200.  D = 48 has no packed path: attn_x3_kernel<4,2,8,false>."""
    Bc, H, D = 2, 8, 48
    qkv, dqkv, kw = sparse_causal_call(Bc, T, Lt, H, D, seed=300 + T + Lt)
    assert workspace_bytes(*dqkv, L.MMA_X3, **kw) == 0
    rows = sample_rows(Lt, 96)
    ref = sparse_causal_ref(qkv, Bc, T, Lt, H, D, rows)
    cut = lambda o: o.view(Bc * T, Lt, H * D).cpu()[:, rows]  # noqa: E731
    run_yardstick(dqkv, (Bc * T * Lt, H * D), kw, cut, ref, f'mode1 T={T} Ltok={Lt}', False)


def test_mode1_sparse_causal_d128_packed_x3():
    """Mode 1 with D = 128 and Lq = 256 (the dispatch takes it; no product caller yet): the packed mode-1 path,
    attn_pack_kv_x3_kernel<128,128> + attn_x3_kernel<4,4,8,true> (sparse-causal key gather inside the pack kernel);
    un-packed attn_x3_kernel<4,4,8,false>."""
    Bc, T, Lt, H, D = 2, 3, 256, 2, 128
    qkv, dqkv, kw = sparse_causal_call(Bc, T, Lt, H, D, seed=401)
    assert workspace_bytes(*dqkv, L.MMA_X3, **kw) > 0
    rows = sample_rows(Lt, 128)
    ref = sparse_causal_ref(qkv, Bc, T, Lt, H, D, rows)
    cut = lambda o: o.view(Bc * T, Lt, H * D).cpu()[:, rows]  # noqa: E731
    run_yardstick(dqkv, (Bc * T * Lt, H * D), kw, cut, ref, 'mode1 D=128 packed', True)


# ------------------------------------------------------------------------------------------------ temporal (mode 0, strided)
@pytest.mark.parametrize("T", [2, 3, 20])
def test_temporal_strided_x3(T):
    """Kalman temporal attention as net.py launches it: batch = spatial token (B = Ltok = 256), tokens = the T frames, read in
    place from [(f d) c] with strides (3 inner, Ltok 3 inner, dh), H = 8, dh = 48.  Lq = T <= 32: attn_x3_kernel<1,2,8,false>."""
    Lt, H, D = 256, 8, 48
    inner = H * D
    qkv = randn(500 + T, (T, Lt, 3 * inner))
    qd = qkv.cuda()
    st = (3 * inner, Lt * 3 * inner, D)
    kw = dict(B=Lt, H=H, Lq=T, Lk=T, D=D, Dv=D, scale=D ** -0.5, q_str=st, k_str=st, v_str=st, o_str=(inner, Lt * inner, D))
    q, k, v = (t.double().permute(1, 0, 2).reshape(Lt, T, H, D).permute(0, 2, 1, 3) for t in qkv.split(inner, dim=-1))
    ref = torch.matmul(torch.softmax(torch.matmul(q, k.transpose(2, 3)) / math.sqrt(D), dim=-1), v)
    ref = ref.permute(0, 2, 1, 3).reshape(Lt, T, inner)
    cut = lambda o: o.view(T, Lt, inner).cpu().permute(1, 0, 2)  # noqa: E731
    run_yardstick((qd, ops.offset(qd, inner), ops.offset(qd, 2 * inner)), (T * Lt, inner), kw, cut, ref, f'temporal T={T}', False)


# ------------------------------------------------------------------------------------------------ loudness, modes 1 and 2
def check_loud(what, got, ref, affected, e32_aff):
    """x3 outputs of rows that read the 1e5 row: non-finite, or correct -- never finite and wrong (the engine's
    keep_nonfinite_flag fallback re-runs a forward whose outputs are non-finite).  Every other row: finite and correct."""
    got = got.detach().double().cpu()
    sc = ref[~affected].abs().max().item()
    tol_aff = max(3.0 * e32_aff, TOL * ref[affected].abs().max().item())
    a_got, a_ref = got[affected], ref[affected]
    fin = torch.isfinite(a_got)
    bad = fin & ((a_got - a_ref).abs() > tol_aff)
    print(f'[loud] {what}: {int((~fin).sum())} of {a_got.numel()} affected outputs non-finite, {int(bad.sum())} finite and wrong')
    assert not bad.any(), f'{what}: {int(bad.sum())} affected outputs finite and wrong (max err {(a_got - a_ref)[bad].abs().max():.3e})'
    u = got[~affected]
    assert torch.isfinite(u).all(), f'{what}: non-finite outputs in rows that never read the 1e5 row'
    return (u - ref[~affected]).abs().max().item(), sc


@pytest.mark.parametrize("operand", ['q', 'k', 'v'])
def test_mode1_loud_on_out_of_range_row_x3(operand):
    """Mode 1 has no range probe: a row of magnitude 1e5 (beyond fp16) in q, k or v of token 5 of frame 1 of clip 0.  Keys of
    frame 1 are read by frame 2 only (frame 0's keys by every frame), so the affected outputs are one batch (q: one row)."""
    Bc, T, Lt, H, D = 2, 3, 256, 8, 48
    inner = H * D
    qkv, _, kw = sparse_causal_call(Bc, T, Lt, H, D, seed=601)
    col = {'q': 0, 'k': inner, 'v': 2 * inner}[operand]
    qkv[1, 5, col:col + inner] = randn(602, (inner,)).sign() * 1e5
    qd = qkv.cuda()
    dqkv = (qd, ops.offset(qd, inner), ops.offset(qd, 2 * inner))
    rows = torch.arange(Lt)
    ref = sparse_causal_ref(qkv, Bc, T, Lt, H, D, rows)
    affected = torch.zeros(Bc * T, Lt, H * D, dtype=torch.bool)
    if operand == 'q':
        affected[1, 5] = True
    else:
        affected[2] = True
    o32 = launch(*dqkv, (Bc * T * Lt, H * D), L.MMA_F32, **kw).view(Bc * T, Lt, H * D)
    assert torch.isfinite(o32).all()
    e32_aff = err64(o32.cpu()[affected], ref[affected])
    e32 = err64(o32.cpu()[~affected], ref[~affected])
    o3 = launch(*dqkv, (Bc * T * Lt, H * D), L.MMA_X3, **kw).view(Bc * T, Lt, H * D)
    e3, sc = check_loud(f'mode1 {operand}', o3, ref, affected, e32_aff)
    yardstick(f'mode1 loud {operand} (unaffected rows)', e3, e32, sc)


@pytest.mark.parametrize("operand", ['q', 'k', 'v'])
def test_mode2_loud_on_out_of_range_row_x3(operand):
    """Mode 2 has no range probe: a row of magnitude 1e5 in q (self), or k / v (cross, kv_rot = P) of one pixel of image 1 on a
    shifted 32x32 grid.  Affected: the windows whose keys come from that pixel of that image (q: the one output row).
    Packed attn_x3_kernel<4,4,8,true> and un-packed attn_x3_kernel<4,4,8,false>."""
    h = w = 32
    P, C, ks = 2, 128, 2
    n_img, Lt = 2 * P, h * w
    cross = operand != 'q'
    (q, k, v), host, kw, kv_rot = gm_call(h, w, P, True, cross, seed=700)
    qh, kh, vh = (t.clone() for t in host)
    pix = 7 * w + 30                               # wraps across the roll on the column axis
    src = {'q': qh, 'k': kh, 'v': vh}[operand]
    src[1, pix] = randn(701, (C,)).sign() * 1e5
    if cross:
        q = qh.reshape(n_img * Lt, C).cuda()
        kv = torch.cat([kh, vh], dim=-1).reshape(n_img * Lt, 2 * C).cuda()
        k, v = kv, ops.offset(kv, C)
    else:
        qkv = torch.cat([qh, kh, vh], dim=-1).reshape(n_img * Lt, 3 * C).cuda()
        q, k, v = qkv, ops.offset(qkv, C), ops.offset(qkv, 2 * C)
    sy, sx = win_shift(h, w, ks, True)
    rows = torch.arange(Lt // 4)
    ref = win_ref(qh, kh, vh, h, w, ks, True, kv_rot, rows)
    marker = torch.zeros(n_img, Lt, 1)
    marker[1, pix] = 1.0
    if operand == 'q':
        affected = win_split(marker, h, w, ks, sy, sx).bool().expand(-1, -1, C).clone()
    else:
        hit = win_split(torch.roll(marker, -kv_rot, 0), h, w, ks, sy, sx).bool().any(dim=1)[:, 0]   # windows reading the pixel
        affected = hit[:, None, None].expand(-1, Lt // 4, C).clone()
    assert 0 < affected.sum() < affected.numel()
    cut = lambda o: win_split(o.view(n_img, Lt, C).cpu(), h, w, ks, sy, sx)  # noqa: E731
    o32 = cut(launch(q, k, v, (n_img * Lt, C), L.MMA_F32, **kw))
    assert torch.isfinite(o32).all()
    e32_aff, e32 = err64(o32[affected], ref[affected]), err64(o32[~affected], ref[~affected])
    for name, flags in (('packed', 0), ('nopack', L.ATTN_NO_PACK)):
        o3 = cut(launch(q, k, v, (n_img * Lt, C), L.MMA_X3, flags, **kw))
        e3, sc = check_loud(f'mode2 {operand} {name}', o3, ref, affected, e32_aff)
        yardstick(f'mode2 loud {operand} {name} (unaffected rows)', e3, e32, sc)
