"""GPU suite (-m gpu): the single-fp16 form of keep_attention (mma = KEEP_MMA_X1 with flags & KEEP_ATTN_X1: the packed D = Dv = 128 form,
attn_pack_kv_x3_kernel<128, 128, true> + attn_x3_kernel<4, 4, 8, true, true>), judged two ways -- both bounds derived, neither measured:

* against its TWIN, fp64 attention (abi_ref.win_ref / heads_ref) on operands rounded as include/keep_hip.h says under KEEP_ATTN_X1:
  q, k and v each rounded once to fp16 as given (the scale multiplies the fp32 scores afterwards).  What the twin does not model is the one
  rounding of every probability to fp16 in front of P.V: 2^-11 relative per term, sum p = 1, a factor 2 for the running rescale --

      |got - twin| <= 2^-10 * max|v| + TOL * max(1, max|twin|)          (TOL: abi_ref's x3-class tolerance)

* against the UNROUNDED fp64 reference: a score moves by at most eps = 2^-10 * scale * max_(q,k) sum_i |q_i| |k_i| (two 2^-11 roundings per
  product), so every softmax weight moves by a factor within exp(+-2 eps), and v by 2^-11 relative --

      |got - ref| <= (exp(2 eps) - 1) * max|v| + 2^-10 * max|v|

The same calls under KEEP_MMA_X3 pass the suite's x3 yardstick, and the x1 output differs from the x3 output by more than x3's own error
(a kernel that quietly ran x3 would not)."""
import ctypes
import math

import pytest
import torch

import footprint as FP
from abi_ref import TOL, heads_ref, win_ref, win_shift, win_split, yardstick
from comfyui_keep_amd.engine import hiplib as L
from comfyui_keep_amd.engine import ops

pytestmark = pytest.mark.gpu
C = 128
X1 = dict(mma=L.MMA_X1, flags=L.ATTN_X1)


def randn(seed, shape, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float32) * scale


def r16(t):
    return t.to(torch.float16).to(torch.float64)


def x1_bytes(B, Lk, H=1):
    """The documented scratch of the flagged call (include/keep_hip.h, KEEP_ATTN_X1)."""
    return B * H * ((Lk + 31) // 32) * (32 * (C + 8) + 128 * 40) * 2


def win_case(h, w, shift, seed, n_img=2, kv_rot=1, ks=2):
    """Mode 2 as net.py:_gm_layer's cross attention launches it: q [n_img * Lt, C], k | v in one [n_img * Lt, 2C] buffer."""
    Lt = h * w
    qb, kvb = randn(seed, (n_img * Lt, C), 1.5), randn(seed + 1, (n_img * Lt, 2 * C))
    host = (qb.view(n_img, Lt, C), kvb.view(n_img, Lt, 2 * C)[..., :C].contiguous(), kvb.view(n_img, Lt, 2 * C)[..., C:].contiguous())
    Lw = Lt // (ks * ks)
    kw = dict(B=n_img * ks * ks, H=1, Lq=Lw, Lk=Lw, D=C, Dv=C, scale=1.0 / math.sqrt(C), mode=2, img_h=h, img_w=w, ksplit=ks,
              shift=(h // ks // 2 if shift else 0), kv_rot=kv_rot, n_img=n_img,
              q_bs=Lt * C, q_ts=C, q_hs=0, k_bs=Lt * 2 * C, k_ts=2 * C, k_hs=0, v_bs=Lt * 2 * C, v_ts=2 * C, v_hs=0, o_bs=Lt * C, o_ts=C, o_hs=0)
    sy, sx = win_shift(h, w, ks, shift)
    rows = torch.arange(Lw)

    def ref(q, k, v):
        return win_ref(q, k, v, h, w, ks, shift, kv_rot, rows)

    def cut(o):
        return win_split(o.view(n_img, Lt, C).double().cpu(), h, w, ks, sy, sx)

    # max over the (q, k) pairs a query meets of sum_i |q_i| |k_i|: image i reads the keys of image (i + kv_rot) % n_img
    qk = max(float((host[0][i].abs().double() @ host[1][(i + kv_rot) % n_img].abs().double().T).max()) for i in range(n_img))
    return dict(name=f'mode2 {h}x{w} shift={kw["shift"]}', kw=kw, host=host, dev=lambda: _dev_win(qb, kvb), o_shape=(n_img * Lt, C), ref=ref, cut=cut, qk=qk)


def _dev_win(qb, kvb):
    kvd = kvb.cuda()
    return qb.cuda(), kvd, ops.offset(kvd, C)


def plain_case(B, Lq, Lk, seed):
    q, k, v = randn(seed, (B, Lq, C), 1.5), randn(seed + 1, (B, Lk, C)), randn(seed + 2, (B, Lk, C))
    kw = dict(B=B, H=1, Lq=Lq, Lk=Lk, D=C, Dv=C, scale=1.0 / math.sqrt(C), mode=0,
              q_bs=Lq * C, q_ts=C, q_hs=C, k_bs=Lk * C, k_ts=C, k_hs=C, v_bs=Lk * C, v_ts=C, v_hs=C, o_bs=Lq * C, o_ts=C, o_hs=C)

    def ref(q_, k_, v_):
        return heads_ref(q_.double(), k_.double(), v_.double(), 1, 1.0 / math.sqrt(C))

    qk = float(torch.matmul(q.abs().double(), k.abs().double().transpose(1, 2)).max())
    return dict(name=f'mode0 B={B} Lq={Lq} Lk={Lk}', kw=kw, host=(q, k, v), dev=lambda: (q.cuda(), k.cuda(), v.cuda()), o_shape=(B * Lq, C), ref=ref,
                cut=lambda o: o.view(B, Lq, C).double().cpu(), qk=qk)


CASES = {
    'mode2_32x32_shift0': lambda: win_case(32, 32, False, 11),
    'mode2_32x32_shift8': lambda: win_case(32, 32, True, 12),
    'mode2_32x64_shift8': lambda: win_case(32, 64, True, 13),      # non-square: 16 x 32 windows of 512 tokens, roll (8, 16)
    'mode0_ragged_keys': lambda: plain_case(2, 288, 300, 14),      # three query blocks (the last one ragged), a 12-key tail tile
}


def call(q, k, v, o, kw, *, mma, flags=0, ws_bytes=None, **over):
    """One keep_attention call with the scratch the library asks for (``ws_bytes``: that many instead; 0 = none); returns the status code."""
    a = L.attn_args(q=q, k=k, v=v, o=o, in_dtype=L.F32, **dict(kw, mma=mma, flags=flags, **over))
    need = L.attention_workspace_bytes(a)
    give = need if ws_bytes is None else ws_bytes
    ws = torch.empty(max(give, 4) // 4 + 4, dtype=torch.float32, device='cuda')
    if give > 0:
        a.workspace, a.workspace_bytes = ws.data_ptr(), give
    rc = L.load().keep_attention(ctypes.byref(a), L._stream())
    torch.cuda.synchronize()
    return rc, need


@pytest.mark.parametrize('name', list(CASES))
def test_x1_against_its_twin_and_the_unrounded_reference(name):
    c = CASES[name]()
    q, k, v = c['dev']()
    qh, kh, vh = c['host']
    outs = {}
    for pol, kwp in (('x1', X1), ('x3', dict(mma=L.MMA_X3)), ('f32', dict(mma=L.MMA_F32))):
        o = torch.full(c['o_shape'], float('nan'), device='cuda')
        rc, need = call(q, k, v, o, c['kw'], **kwp)
        assert rc == 0, (pol, rc, L.load().keep_last_error().decode())
        assert torch.isfinite(o).all(), f'{c["name"]} {pol}: non-finite output'
        outs[pol] = c['cut'](o)
        if pol == 'x1':      # the flagged call asks for exactly the documented scratch, less than the x3 packed form's
            assert need == x1_bytes(c['kw']['B'], c['kw']['Lk']), need
        if pol == 'x3':
            assert need > x1_bytes(c['kw']['B'], c['kw']['Lk'])
    ref = c['ref'](qh, kh, vh)
    twin = c['ref'](r16(qh), r16(kh), r16(vh))
    vmax = float(vh.abs().max())
    e_twin = float((outs['x1'] - twin).abs().max())
    e_ref = float((outs['x1'] - ref).abs().max())
    eps = 2.0 ** -10 * c['kw']['scale'] * c['qk']
    b_twin = 2.0 ** -10 * vmax + TOL * max(1.0, float(twin.abs().max()))
    b_ref = (math.exp(2 * eps) - 1.0) * vmax + 2.0 ** -10 * vmax
    e3, e32 = float((outs['x3'] - ref).abs().max()), float((outs['f32'] - ref).abs().max())
    moved = float((outs['x1'] - outs['x3']).abs().max())
    print(f'[attn-x1] {c["name"]}: err_twin {e_twin:.3e} (bound {b_twin:.3e}) err_ref {e_ref:.3e} (bound {b_ref:.3e}, eps {eps:.3e}) '
          f'x1 - x3 {moved:.3e} err_x3 {e3:.3e}')
    assert e_twin <= b_twin, f'{c["name"]}: |x1 - twin| {e_twin:.3e} > {b_twin:.3e}'
    assert e_ref <= b_ref, f'{c["name"]}: |x1 - fp64 reference| {e_ref:.3e} > {b_ref:.3e}'
    yardstick(f'{c["name"]} (same call, x3)', e3, e32, float(ref.abs().max()))      # the same call under x3 passes its existing class
    # sensitivity: single fp16 is visibly not x3 -- it differs from the x3 output by more than x3 differs from fp64
    assert not torch.equal(outs['x1'], outs['x3']) and moved > 8.0 * max(e3, 1e-7), (moved, e3)


def test_ops_rule_runs_x1_where_admitted_and_x3_elsewhere():
    """Ops.attention with ``attn_x1``: the 256-token windows run the flagged form (the bits of the direct call), a Dv = 2 call stays x3."""
    c = CASES['mode2_32x32_shift8']()
    q, k, v = c['dev']()
    kw = c['kw']
    direct = torch.empty(c['o_shape'], device='cuda')
    assert call(q, k, v, direct, kw, **X1)[0] == 0
    x3 = torch.empty(c['o_shape'], device='cuda')
    assert call(q, k, v, x3, kw, mma=L.MMA_X3)[0] == 0
    o = ops.Ops()
    o.mma = o.attn_mma = L.MMA_X3
    strides = dict(q_str=(kw['q_bs'], kw['q_ts'], 0), k_str=(kw['k_bs'], kw['k_ts'], 0), v_str=(kw['v_bs'], kw['v_ts'], 0), o_str=(kw['o_bs'], kw['o_ts'], 0))
    geo = {n: kw[n] for n in ('B', 'H', 'Lq', 'Lk', 'D', 'Dv', 'scale', 'mode', 'img_h', 'img_w', 'ksplit', 'shift', 'kv_rot', 'n_img')}
    off = o.attention(q, k, v, torch.empty_like(direct), **geo, **strides)
    assert torch.equal(off, x3) and o._attn_x1_route == {}      # the rule is off by default: not even a query
    o.attn_x1 = True
    on = o.attention(q, k, v, torch.empty_like(direct), **geo, **strides)
    torch.cuda.synchronize()
    assert torch.equal(on, direct) and not torch.equal(on, x3) and list(o._attn_x1_route.values()) == [True]
    # the correlation shape (Dv = 2): refused by the library, so the call stays on x3 -- same bits as an Ops without the rule
    P, Lt = 2, 256
    f0, f1, grid = randn(1, (P * Lt, C)).cuda(), randn(2, (P * Lt, C)).cuda(), randn(3, (Lt, 2)).cuda()
    kw2 = dict(B=P, H=1, Lq=Lt, Lk=Lt, D=C, Dv=2, scale=1.0 / math.sqrt(C), q_str=(Lt * C, C, 0), k_str=(Lt * C, C, 0), v_str=(0, 2, 0), o_str=(Lt * 2, 2, 0))
    a = o.attention(f0, f1, grid, torch.empty(P * Lt, 2, device='cuda'), **kw2)
    b = ops.attention(f0, f1, grid, torch.empty(P * Lt, 2, device='cuda'), mma=L.MMA_X3, **kw2)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and sorted(o._attn_x1_route.values()) == [False, True]


def test_refusals_hold_on_the_device():
    """Everything KEEP_MMA_X1 | KEEP_ATTN_X1 does not admit answers KEEP_EUNSUP with a reason and writes nothing; KEEP_MMA_X1 without the bit
    is refused as before."""
    c = CASES['mode0_ragged_keys']()
    q, k, v = c['dev']()
    kw = c['kw']
    lib = L.load()

    def refused(what, text, **over):
        o = torch.full(c['o_shape'], 7.0, device='cuda')
        rc, need = call(q, k, v, o, kw, **dict(X1, **over))
        msg = lib.keep_last_error().decode()
        assert rc == -2 and text in msg and 'KEEP_MMA_X1' in msg, (what, rc, msg)
        assert bool((o == 7.0).all()), what
        return need
    assert refused('no workspace', 'workspace', ws_bytes=0) == x1_bytes(2, 300)
    refused('small workspace', 'workspace', ws_bytes=x1_bytes(2, 300) - 16)
    assert refused('NO_PACK', 'KEEP_ATTN_NO_PACK', flags=L.ATTN_X1 | L.ATTN_NO_PACK) == -1
    assert refused('Lq < 256', 'Lq', Lq=128) == -1
    assert refused('D = 64', 'D = Dv = 128', D=64, q_hs=64, k_hs=64) == -1
    assert refused('Dv = 64', 'D = Dv = 128', Dv=64) == -1
    assert refused('mode 1', 'mode', mode=1, T=2, seg_len=150) == -1
    am = torch.ones(2, device='cuda')
    assert refused('range probes', 'amax', q_amax=am.data_ptr(), k_amax=am.data_ptr(), v_amax=am.data_ptr()) == -1
    assert refused('unaligned rows', '16-byte', q_ts=C + 1) == -1
    o = torch.full(c['o_shape'], 7.0, device='cuda')
    rc, need = call(q, k, v, o, kw, mma=L.MMA_X1)
    assert rc == -1 and need == 0 and 'KEEP_MMA_X1' in lib.keep_last_error().decode() and bool((o == 7.0).all())
    with pytest.raises(L.KeepHipError, match='KEEP_MMA_X1'):
        ops.attention(q, k, v, o, B=2, H=1, Lq=288, Lk=300, D=C, Dv=C, scale=1.0, q_str=(288 * C, C, C), k_str=(300 * C, C, C),
                      v_str=(300 * C, C, C), o_str=(288 * C, C, C), mma=L.MMA_X1)


@pytest.mark.parametrize('name', ['mode2_32x32_shift8', 'mode0_ragged_keys'])
def test_x1_footprint(name):
    """q, k | v, o and the scratch -- at exactly the reported size -- in guarded regions: the write, read and value checks of
    tests/footprint.py all run (a 128-query tile of q / o and a 32-key tile of k | v rows per step)."""
    c = CASES[name]()
    kw = c['kw']
    qh, kh, vh = c['host']
    tb = 128 * 3 * C * 4
    if kw['mode'] == 2:
        kv = torch.cat([kh, vh], dim=-1).reshape(-1, 2 * C)
        R = [FP.single('q', qh.reshape(-1, C), tile_bytes=tb), FP.Region(kv.shape[0], 2 * C, {'k': (0, C, kh.reshape(-1, C)), 'v': (C, C, vh.reshape(-1, C))}, torch.float32, 'r', tb)]
    else:
        R = [FP.single('q', qh.reshape(-1, C), tile_bytes=tb), FP.single('k', kh.reshape(-1, C), tile_bytes=tb), FP.single('v', vh.reshape(-1, C), tile_bytes=tb)]
    need = x1_bytes(kw['B'], kw['Lk'])
    R += [FP.output('o', c['o_shape'], tile_bytes=tb), FP.output('ws', (1, need // 4), tile_bytes=tb, compare=False)]

    def launch(t):
        a = L.attn_args(q=t['q'], k=t['k'], v=t['v'], o=t['o'], in_dtype=L.F32, **dict(kw, **X1))
        now = L.attention_workspace_bytes(a)
        assert now == need, (now, need)
        a.workspace, a.workspace_bytes = t['ws'].data_ptr(), need
        L._check(L.load().keep_attention(ctypes.byref(a), L._stream()), 'keep_attention')
        return now
    out = FP.run(launch, R, 'cuda')
    assert float(out['o'].abs().max()) > 0
