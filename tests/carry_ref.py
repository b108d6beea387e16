"""``oracle.keep_oracle.keep_forward``'s loop with a state in and a state out: what a clip computes when its frame 0 FOLLOWS the last
frame of another clip instead of starting from nothing (the engine's ``KeepNet(x, carry=..., return_state=...)``).

Composed from the oracle's own functions, imported unmodified; the loop body is ``keep_forward``'s, with three differences and no other:
the flow pairs start at the seam (state frame, x[:, 0]); frame 0 takes the ``i > 0`` branch against the state's ``prev_out`` and
``cross_prev``; the Kalman gains may be forced.  The gains are computed on THIS clip's codes only, as the engine does (``gains[:, 0]``,
which the uncarried forward computes and never uses, is used).  tests/test_carry_oracle.py pins it to ``keep_forward``: with the uncut
clip's gains forced, a clip cut in two reproduces the uncut clip exactly."""
import math

import torch

import keep_oracle as O
from comfyui_keep_amd.engine.arch import DEFAULT_ARCH, FUSE_ENCODER_BLOCK, FUSE_GENERATOR_BLOCK, generator_blocks


@torch.no_grad()
def keep_forward_carried(x, W, cfg=None, state=None, force_gains=None, force_indices=None):
    """x [B,T,3,H,W] -> (out [B,T,3,H,W], aux, state after the last frame).  ``state``: None (``keep_forward`` itself) or the third
    return value of the call on the clip in front: {'frame', 'prev_out', 'cross_prev'}."""
    cfg = dict(DEFAULT_ARCH, **(cfg or {}))
    b, t, c, h, w = x.shape
    xf = x if state is None else torch.cat([state['frame'].unsqueeze(1), x], dim=1)
    off = 0 if state is None else 1
    flows = O.get_flow(xf, W) if xf.shape[1] > 1 else None                # pair p = (xf[p], xf[p + 1]); frame i reads pair i - 1 + off
    enc_taps = [FUSE_ENCODER_BLOCK[s] for s in cfg['cft_list']]
    z, feats = O.encoder_forward(x.reshape(-1, c, h, w), W, 'encoder', cfg, enc_taps)
    enc_feat = {k: v.reshape(b, t, *v.shape[1:]) for k, v in feats.items()}
    z_codes = z.reshape(b, t, *z.shape[1:])
    gains = O.kalman_calc_gain(z_codes, W, cfg) if force_gains is None else force_gains
    cft_at = {FUSE_GENERATOR_BLOCK[s]: s for s in cfg['cft_list']}
    cfa_at = {FUSE_GENERATOR_BLOCK[s]: s for s in cfg['cfa_list']}
    gblocks = generator_blocks(cfg)
    side = int(math.sqrt(cfg['latent_size']))
    outs, all_idx, all_logits = [], [], []
    cross_prev, prev_out = ({}, None) if state is None else (dict(state['cross_prev']), state['prev_out'])
    for i in range(t):
        if i == 0 and state is None:
            z_hat = z_codes[:, 0]
        else:
            warped = O.flow_warp(prev_out, flows[:, i - 1 + off].permute(0, 2, 3, 1))
            z_prime, _ = O.encoder_forward(warped, W, 'hq_encoder', cfg)
            g = gains[:, i]
            z_hat = (1 - g) * z_codes[:, i] + g * z_prime
        logits, idx = O.predict_codes(z_hat, W, cfg)
        if force_indices is not None:
            idx = force_indices[:, i]
        y = O.codebook_lookup(idx, W, b, side, cfg['emb_dim'])
        for j, (kind, _, _) in enumerate(gblocks):
            y = O.vq_block(y, W, f'generator.blocks.{j}', kind)
            if j in cft_at:
                s = cft_at[j]
                y = O.cft_fuse(enc_feat[s][:, i], y, W, f'cft.{s}', cfg['cond'])
            if j in cfa_at:
                s = cfa_at[j]
                if i > 0 or state is not None:
                    y = O.cfa_fuse(y, cross_prev[s], W, f'cfa.{s}', cfg['cfa_nhead'], cfg['cfa_dim'])
                cross_prev[s] = y
        prev_out = y
        outs.append(y)
        all_idx.append(idx)
        all_logits.append(logits)
    aux = {'indices': torch.stack(all_idx, 1), 'logits': torch.stack(all_logits, 1), 'gains': gains, 'flows': flows}
    return torch.stack(outs, dim=1), aux, {'frame': x[:, -1], 'prev_out': prev_out, 'cross_prev': dict(cross_prev)}
