#!/usr/bin/env python
"""Micro-benchmark of keep_attention on the GMFlow swin-window shape (bf16 q/k/v, mode 2), for ablations / rocprofv3.
   python tools/bench_attn.py [n_img] [shift]
   python tools/bench_attn.py --proj [n_img] [forms]     x3 policy: projection GEMM + (pack +) attention as net.py:_gm_layer launches them, 64 x 64
       tokens, shift 0 / 16, self- and cross-attention; `forms` (default packed,presplit) are alternated, 4 rounds of 10 launches each:
       packed = fp32 k / v + attn_pack_kv_x3_kernel + attn_x3_kernel<4,4,8,true>; presplit = split-fp16 k / v from the GEMM + attn_x3_presplit_kernel.
       The cross case also times the q projection, which is the same un-split launch in both forms: its relative difference reads smaller than the
       self case's for the same saving."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

load_package()
from comfyui_keep_amd.engine import ops  # noqa: E402


def proj_bench(n_img, forms):
    import statistics

    from comfyui_keep_amd.engine import hiplib as L
    C, h8, w8 = 128, 64, 64
    Ltok = h8 * w8
    ops.DEFAULT.attn_mma = L.MMA_X3
    g = torch.Generator().manual_seed(0)
    wqkv = (torch.randn(3 * C, C, generator=g) * C ** -0.5).cuda()
    src, tgt = torch.randn(n_img * Ltok, C, generator=g).cuda(), torch.randn(n_img * Ltok, C, generator=g).cuda()
    o = torch.empty(n_img * Ltok, C, device='cuda')

    twins = {w.data_ptr(): ops.split_x3(w, 1.0).view(-1) for w in (wqkv, wqkv[C:])}      # (wqkv[:C] starts where wqkv does: the twin's first rows)

    def gemm(x, w, split_cols):
        kw = {} if split_cols is None else dict(split_cols=split_cols)
        return ops.conv(x.view(n_img, Ltok, 1, C), w, None, stride=1, pad=0, ksize=1, mma=L.MMA_X3, wx3=twins[w.data_ptr()],
                        x3_acc_scale=1.0, bounded=True, **kw).view(-1, w.shape[0])

    def layer(form, cross, shift):
        split = form == 'presplit'
        kw = dict(kv_split=True) if split else {}
        if cross:
            q = gemm(src, wqkv[:C], None)
            kv = gemm(tgt, wqkv[C:], (0, 2 * C) if split else None)
            k, v, sq, skv = kv, ops.offset(kv, C), (Ltok * C, C, 0), (Ltok * 2 * C, 2 * C, 0)
        else:
            q = gemm(src, wqkv, (C, 3 * C) if split else None)
            k, v = ops.offset(q, C), ops.offset(q, 2 * C)
            sq = skv = (Ltok * 3 * C, 3 * C, 0)
        ops.attention(q, k, v, o, B=n_img * 4, H=1, Lq=Ltok // 4, Lk=Ltok // 4, D=C, Dv=C, scale=C ** -0.5, q_str=sq, k_str=skv, v_str=skv,
                      o_str=(Ltok * C, C, 0), mode=2, img_h=h8, img_w=w8, ksplit=2, shift=shift, kv_rot=n_img // 2 if cross else 0, n_img=n_img, **kw)

    for cross in (False, True):
        for shift in (0, 16):
            rounds, outs = {f: [] for f in forms}, {}
            for f in forms:
                layer(f, cross, shift)
                outs[f] = o.clone()
            for _ in range(4):
                for f in forms:
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(10):
                        layer(f, cross, shift)
                    e1.record()
                    torch.cuda.synchronize()
                    rounds[f].append(e0.elapsed_time(e1) * 100.0)
            for f in forms:
                r = rounds[f]
                print(f"proj+attn n_img={n_img:5d} {'cross' if cross else 'self '} shift={shift:2d} {f:9s} median {statistics.median(r):9.1f} us  min {min(r):9.1f} "
                      f"max {max(r):9.1f}  spread {100.0 * (max(r) - min(r)) / statistics.median(r):4.1f} %  rounds {[round(x, 1) for x in r]}")
            if len(forms) > 1:
                print(f"    outputs bit-equal: {all(torch.equal(outs[forms[0]], outs[f]) for f in forms[1:])}")


if len(sys.argv) > 1 and sys.argv[1] == '--proj':
    proj_bench(int(sys.argv[2]) if len(sys.argv) > 2 else 76, (sys.argv[3] if len(sys.argv) > 3 else 'packed,presplit').split(','))
    sys.exit(0)
n_img = int(sys.argv[1]) if len(sys.argv) > 1 else 76
shift = int(sys.argv[2]) if len(sys.argv) > 2 else 16
dt = torch.bfloat16 if not (os.environ.get('F32') or os.environ.get('X3')) else torch.float32
if os.environ.get('X3'):
    from comfyui_keep_amd.engine import hiplib as L
    ops.DEFAULT.attn_mma = L.MMA_X3
C, h8, w8 = 128, 64, 64
Ltok = h8 * w8
qkv = torch.randn(n_img * Ltok, 3 * C, device='cuda').to(dt)
o = torch.empty(n_img * Ltok, C, device='cuda')
s = (Ltok * 3 * C, 3 * C, 0)


def run():
    ops.attention(qkv, ops.offset(qkv, C), ops.offset(qkv, 2 * C), o, B=n_img * 4, H=1, Lq=Ltok // 4, Lk=Ltok // 4, D=C, Dv=C,
                  scale=C ** -0.5, q_str=s, k_str=s, v_str=s, o_str=(Ltok * C, C, 0), mode=2, img_h=h8, img_w=w8, ksplit=2,
                  shift=shift, kv_rot=n_img // 2, n_img=n_img)


for _ in range(3):
    run()
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(10):
    run()
e1.record()
torch.cuda.synchronize()
ms = e0.elapsed_time(e1) / 10
fl = 4.0 * n_img * 4 * (Ltok // 4) ** 2 * C
print(f"swin attention n_img={n_img} shift={shift} {dt}: {ms * 1e3:.1f} us  {fl / ms / 1e9:.1f} TFLOP/s")
if os.environ.get('CHECK'):      # compare with the exact-f32 kernel on the same inputs
    from comfyui_keep_amd.engine import hiplib as L2
    got = o.clone()
    ops.DEFAULT.attn_mma = L2.MMA_F32
    run()
    torch.cuda.synchronize()
    d = (got - o).abs()
    print(f'max |x3 - f32| = {float(d.max()):.3e} (scale {float(o.abs().max()):.3g}); rows off by > 1e-3: '
          f'{int((d.amax(1) > 1e-3).sum())} of {o.shape[0]}')
