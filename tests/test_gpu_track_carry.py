"""GPU suite (-m gpu): a clip that starts from the state its predecessor left (``KeepNet(x, carry=..., return_state=...)``,
``run_clips_u8(after=...)``, KEEP_AMD_TRACK_CARRY; engine/net.py, modules/clip_plan.py, modules/keep_processor.py).

The reference never does this, so there is no reference output to compare the mode with.  What is proved instead:
  * the state is complete and the carried frame 0 runs an interior frame's launches: a clip cut in two, the second half started from
    the first half's state and given the whole clip's Kalman gains, equals the uncut clip BIT FOR BIT (outputs and code indices);
  * a call that takes or returns a state runs eagerly in every graph mode and leaves the net's graph cache alone;
  * chains are batch invariant, a carried 1-frame clip is frame 0 of its carried T = 2 duplicate;
  * the fp16-range fallback re-runs a carried clip from the same incoming state and hands on the re-run's state;
  * the processor's paths run the chain one would run by hand, and are untouched with the knob off."""
import os
import sys

import numpy as np
import pytest
import torch

from comfyui_keep_amd.engine import hiplib as L
from comfyui_keep_amd.engine import ops, synth
from comfyui_keep_amd.engine.arch import DEFAULT_ARCH
from test_gpu_frame_store import Rig, video

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))


def _same_state(a, b):
    if not (torch.equal(a.frame, b.frame) and torch.equal(a.prev_out, b.prev_out) and set(a.cross_prev) == set(b.cross_prev)):
        return False
    for s in a.cross_prev:
        if not torch.equal(a.cross_prev[s], b.cross_prev[s]):
            return False
        if (a.cross_amax[s] is None) != (b.cross_amax[s] is None):
            return False
        if a.cross_amax[s] is not None and not torch.equal(a.cross_amax[s], b.cross_amax[s]):
            return False
    return True


def _to_x(u8):
    """uint8 BGR [T,H,W,3] -> the net's input [1,T,3,H,W]: the kernels ``run_clips_u8`` uses."""
    u8 = u8.cuda().contiguous()
    T, H, W, _ = u8.shape
    f = torch.empty((T, H, W, 3), dtype=torch.float32, device='cuda')
    L.call('keep_img2tensor', u8, f, T * H * W)
    return ops.nhwc_to_nchw(f).view(1, T, 3, H, W)


def _to_u8(o):
    _, T, _, H, W = o.shape
    y = ops.nchw_to_nhwc(o.contiguous().view(T, 3, H, W))
    r8 = torch.empty((T, H, W, 3), dtype=torch.uint8, device='cuda')
    L.call('keep_tensor2img', y, r8, T * H * W)
    return r8.cpu()


def _chain_by_hand(net_, crops_u8, L_):
    """uint8 crops [n,512,512,3] of one track -> the restored uint8 crops of the chain of clips of ``L_``, every call made here."""
    state, out = None, []
    n = crops_u8.shape[0]
    for s in range(0, n, L_):
        last = s + L_ >= n
        res = net_(_to_x(crops_u8[s:s + L_]), carry=state, return_state=not last)
        o, state = (res, None) if last else res
        out.append(_to_u8(o))
    return torch.cat(out).numpy()


# ---- the recurrence goes on --------------------------------------------------------------------------------------------------------
def test_a_cut_clip_with_the_whole_clips_gains_equals_the_uncut_clip_bit_for_bit(gpu_net):
    """X of T = 4: whole; X[:, :2] with the state returned; X[:, 2:] carried -- both halves with the whole clip's gains (they are the one
    thing a cut changes: the gain network attends over the clip).  Everything else the second half needs is in the state: the last input
    frame (seam flow), prev_out, the CFA maps and their maxima."""
    x = synth.synth_clip(T=4, B=1, seed=4321).cuda()
    whole, aux = gpu_net(x, return_aux=True)
    gains = aux['gains']
    assert tuple(gains.shape[:2]) == (1, 4)
    a, aux_a, st = gpu_net(x[:, :2], force_gains=gains[:, :2], return_state=True, return_aux=True)
    assert st.batch == 1 and set(st.cross_prev) == set(DEFAULT_ARCH['cfa_list']) and torch.equal(st.frame, x[:, 1])
    b, aux_b = gpu_net(x[:, 2:], carry=st, force_gains=gains[:, 2:], return_aux=True)
    assert torch.equal(torch.cat([aux_a['indices'], aux_b['indices']], 1), aux['indices'])
    assert torch.equal(aux_b['flows'][:, 0], aux['flows'][:, 1])                     # pair 0 of the carried call is the seam
    assert torch.equal(torch.cat([a, b], 1), whole)
    # forced gains are a hook: without them the first half is today's call, bit for bit, state or no state
    plain = gpu_net(x[:, :2])
    with_state, st2 = gpu_net(x[:, :2], return_state=True)
    assert torch.equal(plain, with_state) and torch.equal(st2.frame, x[:, 1])
    # ... and the carried second half differs from the one restored from nothing
    assert not torch.equal(gpu_net(x[:, 2:], carry=st2), gpu_net(x[:, 2:]))
    # a call with a state in or out is never captured: with replay forced on, the same bits and no new graph
    mode, had = gpu_net.graph_mode, set(gpu_net._graphs)
    try:
        gpu_net.graph_mode = '1'
        g_a, g_st = gpu_net(x[:, :2], return_state=True)
        g_b = gpu_net(x[:, 2:], carry=g_st)
    finally:
        gpu_net.graph_mode = mode
    assert set(gpu_net._graphs) == had and torch.equal(g_a, plain) and torch.equal(g_b, gpu_net(x[:, 2:], carry=st2))


# ---- clip-local gains against the oracle ---------------------------------------------------------------------------------------------
def test_a_cut_clip_with_its_own_gains_vs_the_oracle_restatement(gpu_net):
    """The same cut without forced gains -- each half's gains come from its own two frames, ``gains[:, 0]`` of the second half is used --
    against tests/carry_ref.py (``oracle.keep_forward``'s loop with a state in and out; its result is the fixture
    tests/golden/carry_T4.npz, tests/test_carry_oracle.py pins it to the oracle).  The restatement's code indices are injected, and the
    bounds are those of tests/test_gpu_net.py for outputs with injected indices (<= 1e-3 absolute and <= 3e-4 of the output scale) and
    for gains (<= 2e-4)."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'carry_T4.npz'))
    cut, (c0, c1, c2, c3) = int(g['cut']), (int(v) for v in g['crop'])
    x = synth.synth_clip(T=4, B=1, seed=int(g['seed'])).cuda()
    forced = torch.from_numpy(g['indices'].astype(np.int32)).view(1, 4, -1)
    a, _, st = gpu_net(x[:, :cut], force_indices=forced[:, :cut], return_state=True, return_aux=True)
    b, aux_b = gpu_net(x[:, cut:], carry=st, force_indices=forced[:, cut:], return_aux=True)
    out = torch.cat([a, b], 1)[0].cpu()
    gain_err = float(np.abs(aux_b['gains'][0, 0].reshape(-1).cpu().numpy() - g['gains0_second']).max())
    crop_err = np.abs(out[:, :, c0:c1, c2:c3].numpy() - g['out_crop']).reshape(4, -1).max(1)
    grid = out[:, :, 7::16, 5::16][:, :, :32, :32].numpy()                           # (test_gpu_net.py:_digest at 512 x 512)
    grid_err = np.abs(grid - g['out_grid']).reshape(4, -1).max(1)
    scale = float(np.abs(g['out_grid']).max())
    print(f'[{gpu_net.precision}] gains[:, 0] of the carried clip: max err {gain_err:.3e}; per frame max-abs pixel err, centre crop',
          [round(float(v), 7) for v in crop_err], 'digest', [round(float(v), 7) for v in grid_err], f'; output scale {scale:.3g}')
    assert gain_err <= 2e-4
    err = float(max(crop_err.max(), grid_err.max()))
    assert err <= 1e-3 and err <= 3e-4 * scale, (err, scale)


# ---- chains are batch invariant ------------------------------------------------------------------------------------------------------
def test_two_chains_in_one_call_equal_each_chain_alone(gpu_net):
    """A 2 + 2 chain and a 2 + 1 chain of different content in one ``run_clips_u8(after=...)`` call (the carried clips share no group: two
    lengths) and with both in flight, against each chain alone; the carried 1-frame clip is frame 0 of the carried T = 2 call on the
    duplicated frame."""
    rng = np.random.default_rng(7)
    A = torch.from_numpy(rng.integers(0, 256, (4, 512, 512, 3), dtype=np.uint8))
    B = torch.from_numpy(rng.integers(0, 256, (3, 512, 512, 3), dtype=np.uint8))
    got = gpu_net.run_clips_u8([A[:2], B[:2], A[2:], B[2:]], after=[None, None, 0, 1])
    a = gpu_net.run_clips_u8([A[:2], A[2:]], after=[None, 0])
    b = gpu_net.run_clips_u8([B[:2], B[2:]], after=[None, 0])
    assert [tuple(o.shape) for o in got] == [(2, 512, 512, 3), (2, 512, 512, 3), (2, 512, 512, 3), (1, 512, 512, 3)]
    assert torch.equal(got[0], a[0]) and torch.equal(got[2], a[1]) and torch.equal(got[1], b[0]) and torch.equal(got[3], b[1])
    # two carried clips of one length in ONE group (batch of 2) equal the two alone
    both = gpu_net.run_clips_u8([A[:2], B[:2], A[2:], B[1:3]], after=[None, None, 0, 1], max_b=2)
    alone = gpu_net.run_clips_u8([B[:2], B[1:3]], after=[None, 0], max_b=1)
    assert torch.equal(both[2], a[1]) and torch.equal(both[3], alone[1]) and torch.equal(both[1], b[0])
    # the chain by hand, and the duplicate rule
    o0, st = gpu_net(_to_x(B[:2]), return_state=True)
    assert torch.equal(_to_u8(o0), b[0])
    dup, st_dup = gpu_net(_to_x(torch.cat([B[2:], B[2:]])), carry=st, return_state=True)
    assert torch.equal(_to_u8(dup)[:1], b[1])
    one, st_one = gpu_net(_to_x(B[2:]), carry=st, return_state=True)
    assert tuple(one.shape) == (1, 1, 3, 512, 512) and torch.equal(one, dup[:, :1])
    assert torch.equal(st_one.frame, _to_x(B[2:])[:, 0]) and torch.equal(st_one.prev_out.permute(0, 3, 1, 2), one[:, 0])   # the state after frame 0
    assert not _same_state(st_one, st_dup)
    # the carried clips are not the clips restored from nothing, and after=None is today's call
    free = gpu_net.run_clips_u8([A[:2], A[2:]])
    assert torch.equal(free[0], a[0]) and not torch.equal(free[1], a[1])


# ---- the range fallback ----------------------------------------------------------------------------------------------------------------
def test_x3_overflow_in_a_carried_clip_reruns_it_from_the_same_state_and_hands_on_the_reruns_state(synth_weights):
    """The weights of test_gpu_net.py's fallback test (one transformer MLP leaves the fp16 range on the x3 kernels: a numeric flag, the
    arg-max raises the status word): every call of a chain of three is re-run on the exact-f32 kernels from its incoming state, the
    results and the states handed on are the fp32 policy's."""
    from comfyui_keep_amd.engine.net import KeepNet
    W = dict(synth_weights)
    W['ft_layers.4.linear1.weight'] = W['ft_layers.4.linear1.weight'] * 3.0e5
    W['ft_layers.4.linear2.weight'] = W['ft_layers.4.linear2.weight'] / 3.0e5
    x = synth.synth_clip(T=4, B=1, seed=21).cuda()
    nets = {}
    for pol in ('x3', 'fp32'):
        n = KeepNet(**DEFAULT_ARCH)
        n.load_state_dict(W, strict=True)
        nets[pol] = n.to('cuda').eval().set_precision(pol)
    r1, rs1 = nets['fp32'](x[:, :2], return_state=True)
    r2, rs2 = nets['fp32'](x[:, 2:], carry=rs1, return_state=True)
    assert torch.isfinite(r2).all() and nets['fp32'].x3_fallbacks == 0
    g1, gs1 = nets['x3'](x[:, :2], return_state=True)
    assert nets['x3'].x3_fallbacks == 1 and torch.equal(g1, r1) and _same_state(gs1, rs1)
    g2, gs2 = nets['x3'](x[:, 2:], carry=gs1, return_state=True)
    assert nets['x3'].x3_fallbacks == 2 and torch.equal(g2, r2) and _same_state(gs2, rs2)
    assert nets['x3'].precision == 'x3'
    # the uint8 entry (deferred check): a group that hands a state on is checked before its successor is queued
    u8 = [torch.randint(0, 256, (t, 512, 512, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(3)) for t in (2, 2, 1)]
    got = nets['x3'].run_clips_u8(u8, after=[None, 0, 1])
    ref = nets['fp32'].run_clips_u8(u8, after=[None, 0, 1])
    assert nets['x3'].x3_fallbacks == 5 and all(torch.equal(a, b) for a, b in zip(got, ref))


# ---- the processor -----------------------------------------------------------------------------------------------------------------------
def test_processor_paths_run_the_chain_and_the_knob_off_is_untouched(gpu_net, monkeypatch):
    """5 frames of 512 x 512, one face (only_center_face), clips of 2: knob on, the restored faces of the store path, the streamed path
    without a store and the per-frame path equal the chain [2, 2, 1] run by hand through ``KeepNet``; knob off, they equal the three clips
    restored from nothing -- what the code before the knob computed -- with or without track clips."""
    from test_gpu_track_clips import _run
    net = gpu_net
    rig = Rig(net, monkeypatch, (512, 512), 2, chunk=4)
    frames = video(5, 512, 512, seed=41)
    rig.proc.track_clips = rig.proc.track_carry = False
    off, off_faces, crops, off_plan = _run(rig, frames, env=[('KEEP_AMD_FRAME_STORE', '0')], center=True, clip=2)
    assert off_plan is None and len(crops) == 5
    crops = torch.stack([c if isinstance(c, torch.Tensor) else torch.from_numpy(np.asarray(c)) for c in crops]).cpu()
    free = np.concatenate([o.numpy() for o in net.run_clips_u8([crops[0:2], crops[2:4], crops[4:5]])])
    chain = _chain_by_hand(net, crops, 2)
    assert np.array_equal(chain[:2], free[:2]) and not np.array_equal(chain[2:4], free[2:4]) and not np.array_equal(chain[4], free[4])
    for env in ((), (('KEEP_AMD_FRAME_STORE', '0'),), (('KEEP_AMD_STREAM_PASTE', '0'),)):
        rig.proc.track_clips = rig.proc.track_carry = False
        o, faces, _, plan = _run(rig, frames, env=env, center=True, clip=2)
        assert plan is None and np.array_equal(o, off) and all(np.array_equal(faces[i], free[i]) for i in range(5)), env
        rig.proc.track_clips = True
        o, faces, _, plan = _run(rig, frames, env=env, center=True, clip=2)
        assert np.array_equal(o, off) and all(np.array_equal(faces[i], free[i]) for i in range(5)), env
        rig.proc.track_clips, rig.proc.track_carry = False, True                     # the knob implies track clips
        on, faces, _, plan = _run(rig, frames, env=env, center=True, clip=2)
        if env != (('KEEP_AMD_STREAM_PASTE', '0'),):
            assert plan == ([[0, 1], [2, 3], [4]], list(range(5)), [None, 0, 1]), env
        assert len(faces) == 5 and all(np.array_equal(faces[i], chain[i]) for i in range(5)), env
        assert on.shape == off.shape and not np.array_equal(on, off), env


def test_aligned_sequence_runs_the_chain(gpu_net, monkeypatch):
    """An aligned 5-frame sequence (512 x 512 frames: no resize in the way), clips of 2, on the device-resident path and the per-frame
    one: knob on, the chain by hand; knob off, the clips restored from nothing."""
    import synth_facehelper as SF
    for k in ('KEEP_AMD_GPU_RESIZE', 'KEEP_AMD_GPU_ALIGNED_RESIZE', 'KEEP_AMD_STREAM_GROUPS', 'KEEP_AMD_DETECT_BATCH'):
        monkeypatch.delenv(k, raising=False)
    proc, _ = SF.make_processor(gpu_net, (512, 512), 1)
    proc.keep_restored_faces = True
    frames = video(5, 512, 512, seed=43)
    crops = torch.from_numpy(np.stack(frames))
    free = np.concatenate([o.numpy() for o in gpu_net.run_clips_u8([crops[0:2], crops[2:4], crops[4:5]])])
    chain = _chain_by_hand(gpu_net, crops, 2)
    assert not np.array_equal(chain[2:], free[2:])
    for stream in ('1', '0'):
        monkeypatch.setenv('KEEP_AMD_STREAM_PASTE', stream)
        for knob, want in ((False, free), (True, chain)):
            proc.track_carry = knob
            out = proc.process_frames_u8(frames, 1.0, True, False, False, max_clip_length=2)
            assert isinstance(out, torch.Tensor) == (stream == '1')
            faces = [np.asarray(f) for f in proc.last_restored_faces]
            assert len(faces) == 5 and all(np.array_equal(faces[i], want[i]) for i in range(5)), (stream, knob)
