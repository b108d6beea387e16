"""Writes tests/golden/carry_T4.npz: the CPU restatement (tests/carry_ref.py, fp32) of a T = 4 clip cut into 2 + 2, the second half started
from the first half's state, each half with the Kalman gains of its own two frames.

    python tests/make_carry_golden.py

Holds the input seed, the code indices and their top-1 / top-2 margins, ``gains[:, 0]`` of the second clip (the value the uncarried
forward never uses), and of the four output frames the 128 x 128 centre crop plus the 32 x 32 strided digest of tests/test_gpu_net.py.
Before writing it checks the pin of tests/test_carry_oracle.py: with the uncut clip's gains forced the two halves ARE the uncut clip."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

from __graft_entry__ import load_package  # noqa: E402

load_package()

import carry_ref as CR  # noqa: E402
import keep_oracle as O  # noqa: E402
from comfyui_keep_amd.engine import synth  # noqa: E402

SEED, T, CUT = 4321, 4, 2
CROP = (192, 320, 192, 320)


def digest(frames):
    """[T,C,H,W] -> the 32 x 32 strided grid of tests/test_gpu_net.py:_digest."""
    _, _, H, Wd = frames.shape
    return frames[:, :, 7::H // 32, 5::Wd // 32][:, :, :32, :32]


def split_run(x, W, force_gains=None):
    """The clip cut at CUT -> (out [1,T,...], aux of the first half, aux of the second half)."""
    fg = (None, None) if force_gains is None else (force_gains[:, :CUT], force_gains[:, CUT:])
    a, aux_a, st = CR.keep_forward_carried(x[:, :CUT], W, force_gains=fg[0])
    b, aux_b, _ = CR.keep_forward_carried(x[:, CUT:], W, state=st, force_gains=fg[1])
    return torch.cat([a, b], 1), aux_a, aux_b


def pin_error(x, W):
    """max |restatement with the uncut clip's gains forced - oracle.keep_forward| over the uncut clip, and whether the indices agree."""
    whole, aux = O.keep_forward(x, W, return_aux=True)
    out, aux_a, aux_b = split_run(x, W, force_gains=aux['gains'])
    same = torch.equal(torch.cat([aux_a['indices'], aux_b['indices']], 1), aux['indices'])
    return float((out - whole).abs().max()), same


def main():
    W = synth.synth_state_dict(seed=0)
    x = synth.synth_clip(T=T, B=1, seed=SEED)
    err, same = pin_error(x, W)
    print('pin: max |carry_ref(forced gains) - keep_forward| =', err, '; indices equal:', same)
    assert err == 0.0 and same
    out, aux_a, aux_b = split_run(x, W)
    logits = torch.cat([aux_a['logits'], aux_b['logits']], 1)[0]
    top2 = logits.topk(2, -1).values
    a, b, c, d = CROP
    path = os.path.join(ROOT, 'tests', 'golden', 'carry_T4.npz')
    np.savez(path, seed=np.int64(SEED), cut=np.int64(CUT), crop=np.array(CROP, np.int64),
             indices=torch.cat([aux_a['indices'], aux_b['indices']], 1)[0].numpy().astype(np.int16),
             margins=(top2[..., 0] - top2[..., 1]).numpy().astype(np.float32),
             gains0_second=aux_b['gains'][0, 0].reshape(-1).numpy().astype(np.float32),
             out_crop=out[0][:, :, a:b, c:d].numpy().astype(np.float32), out_grid=digest(out[0]).numpy().astype(np.float32))
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
