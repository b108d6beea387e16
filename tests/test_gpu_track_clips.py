"""GPU suite (-m gpu): track clips (KEEP_AMD_TRACK_CLIPS; modules/clip_plan.py, modules/keep_processor.py) and the scatter form of the
batched crop warp (keep_warp_affine_batch_scatter_u8, csrc/keep_paste.hip).

There is no reference to compare the mode with -- the reference never runs its net on one track of a multi-face video.  What is proved
instead: every face's result equals, BIT FOR BIT, the result of that track's clips restored on their own (the engine is batch
invariant), on every path a sequence can take; a single-face video is untouched by the knob; and the scatter entry writes exactly the
crops of the existing entry to exactly the slots it was told."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from comfyui_keep_amd.engine import hiplib as L
from comfyui_keep_amd.engine import paste
from test_gpu_frame_store import WARP_BATCH, Rig, net, video  # noqa: F401  (``net``: the module's fixture)

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))

SCATTER = 'keep_warp_affine_batch_scatter_u8'
BORDER = (135, 133, 132)
POISON = 0x5A


# ---- the scatter entry -----------------------------------------------------------------------------------------------------------
def test_scatter_writes_the_existing_entrys_crops_to_the_named_slots_and_nothing_else(monkeypatch):
    """2 frames of 37 x 53, 33 faces (two launches) into 24 x 40 crops, one of them black, scattered over 40 slots inside a poisoned
    buffer with guards on both sides."""
    N, H, W, DH, DW, F, SLOTS, GUARD = 2, 37, 53, 24, 40, 33, 40, 4096
    rng = np.random.default_rng(17)
    src = torch.from_numpy(rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)).cuda()
    faces = [(i % N, [0.9 + 0.01 * i, 0.0, 0.5 * i - 6.0, 0.0, 0.9 + 0.01 * i, 0.25 * i - 2.0]) for i in range(F)]
    faces[20] = (-1, [0.0] * 6)                                                      # the black crop
    slot_of = [int(s) for s in rng.permutation(SLOTS)[:F]]
    assert slot_of != sorted(slot_of) and len(set(slot_of)) == F
    idx = (C.c_int32 * F)(*[f for f, _ in faces])
    d2s = (C.c_double * (6 * F))(*[v for _, m in faces for v in m])
    slots = (C.c_int32 * F)(*slot_of)
    crop = DH * DW * 3

    # the existing entry on the same inputs: unchanged by the struct change -- every face is its single-frame result
    ref = torch.full((F, DH, DW, 3), POISON, dtype=torch.uint8, device='cuda')
    L.call(WARP_BATCH, src, N, H, W, ref, F, DH, DW, idx, d2s, *BORDER)
    for i, (f, m) in enumerate(faces):
        if f < 0:
            assert not ref[i].any()
            continue
        one = torch.empty((DH, DW, 3), dtype=torch.uint8, device='cuda')
        L.call('keep_warp_affine_u8', src[f], H, W, one, DH, DW, (C.c_double * 6)(*m), *BORDER)
        assert torch.equal(ref[i], one), i

    buf = torch.full((GUARD + SLOTS * crop + GUARD,), POISON, dtype=torch.uint8, device='cuda')
    dst = buf[GUARD:GUARD + SLOTS * crop].view(SLOTS, DH, DW, 3)
    before = src.clone()
    L.call(SCATTER, src, N, H, W, dst, SLOTS, F, DH, DW, idx, slots, d2s, *BORDER)
    torch.cuda.synchronize()
    for f in range(F):
        assert torch.equal(dst[slot_of[f]], ref[f]), f
    unnamed = sorted(set(range(SLOTS)) - set(slot_of))
    assert len(unnamed) == 7 and all(bool((dst[s] == POISON).all()) for s in unnamed)
    assert bool((buf[:GUARD] == POISON).all()) and bool((buf[GUARD + SLOTS * crop:] == POISON).all())
    assert torch.equal(src, before)

    # the python wrapper: frame -> crop matrices, one library call, the same slots
    fwd = [paste.invert_affine(np.array(m, np.float64).reshape(2, 3)) if f >= 0 else None for f, m in faces]
    out = torch.full((SLOTS, DH, DW, 3), POISON, dtype=torch.uint8, device='cuda')
    calls, real = [], L.call
    monkeypatch.setattr(L, 'call', lambda name, *a: (calls.append(name), real(name, *a))[1])
    res = paste.crop_faces_batch(src, [max(f, 0) for f, _ in faces], fwd, out, (DW, DH), slot_of=slot_of)
    monkeypatch.setattr(L, 'call', real)
    plain = torch.empty((F, DH, DW, 3), dtype=torch.uint8, device='cuda')
    paste.crop_faces_batch(src, [max(f, 0) for f, _ in faces], fwd, plain, (DW, DH))
    assert calls == [SCATTER] and res is out
    assert all(torch.equal(out[slot_of[f]], plain[f]) for f in range(F)) and all(bool((out[s] == POISON).all()) for s in unnamed)
    with pytest.raises(ValueError):
        paste.crop_faces_batch(src, [0] * F, fwd, out, (DW, DH), slot_of=slot_of[:-1])
    with pytest.raises(ValueError):
        paste.crop_faces_batch(src, [0] * F, fwd, out[:F - 1], (DW, DH), slot_of=slot_of)
    with pytest.raises(L.KeepHipError, match=SCATTER):
        paste.crop_faces_batch(src, [0] * F, fwd, out, (DW, DH), slot_of=[slot_of[1]] + slot_of[1:])   # a slot named twice
    assert all(torch.equal(out[slot_of[f]], plain[f]) for f in range(F))             # the refused call launched nothing
    torch.cuda.synchronize()


# ---- the claim itself ------------------------------------------------------------------------------------------------------------
def test_plan_restores_every_track_as_if_it_were_alone(gpu_net):
    """Two tracks x five frames of random crops, clips of 3: with the plan every crop equals its track's [3, 2] split restored on its
    own; with the knob off (A0 B0 A1 | B1 A2 B2 | ...) at least one crop does not."""
    import test_host_logic as H   # installs the ComfyUI stubs
    from comfyui_keep_amd.modules.clip_plan import plan_track_clips
    from comfyui_keep_amd.modules.keep_model_loader import KEEPModelPack
    from comfyui_keep_amd.modules.keep_processor import KEEPFaceProcessor
    pack = KEEPModelPack(gpu_net, H._Helper(), None, None, 'KEEP')
    pack.device = torch.device('cuda')
    proc = KEEPFaceProcessor(pack)
    K, N, Lc = 2, 5, 3
    rng = np.random.default_rng(99)
    crops = [np.ascontiguousarray(c) for c in rng.integers(0, 256, (K * N, 512, 512, 3), dtype=np.uint8)]   # crop t * K + j
    clips, slot_of = plan_track_clips([['A', 'B']] * N, Lc)
    assert clips == [[0, 2, 4], [1, 3, 5], [6, 8], [7, 9]]
    got = proc._restore_crops_u8(crops, Lc, members=clips)
    alone = [None] * (K * N)
    for j in range(K):
        track = [crops[t * K + j] for t in range(N)]
        outs = gpu_net.run_clips_u8([torch.from_numpy(np.stack(track[0:3])), torch.from_numpy(np.stack(track[3:5]))])
        for t in range(N):
            alone[t * K + j] = outs[t // 3][t % 3].numpy()
    assert len(got) == K * N and all(g.shape == (512, 512, 3) and g.dtype == np.uint8 for g in got)
    for i in range(K * N):
        assert np.array_equal(got[i], alone[i]), ('crop', i)
    off = proc._restore_crops_u8(crops, Lc)
    assert any(not np.array_equal(off[i], alone[i]) for i in range(K * N))           # the mode does something


# ---- the paths of a sequence -------------------------------------------------------------------------------------------------------
def _run(rig, frames, env=(), center=False, clip=4):
    """One ``process_frames_u8`` call of the rig's processor under ``env`` -> (frames uint8 [n,H,W,3] array, restored faces, the crops
    and the plan the streamed paste was handed -- None on the per-frame path)."""
    for k in ('KEEP_AMD_FRAME_STORE', 'KEEP_AMD_STREAM_PASTE'):
        rig.mp.delenv(k, raising=False)
    for k, v in env:
        rig.mp.setenv(k, v)
    rig.mp.setenv('KEEP_AMD_STREAM_GROUPS', '3')
    for rec in (rig.calls, rig.backgrounds, rig.batches, rig.crop_shapes):
        rec.clear()
    seen = {}
    inner = rig.proc._restore_and_paste_streamed

    def streamed(frames_bgr, crops, *a, **kw):
        seen['crops'], seen['plan'] = crops, kw.get('plan')
        return inner(frames_bgr, crops, *a, **kw)
    rig.mp.setattr(rig.proc, '_restore_and_paste_streamed', streamed)
    rig.helper.begin_sequence()
    if hasattr(rig.helper, 'reads'):
        rig.helper.reads = 0
    try:
        out = rig.proc.process_frames_u8(frames, 1.0, False, center, False, max_clip_length=clip)
    finally:
        rig.mp.setattr(rig.proc, '_restore_and_paste_streamed', inner)
    out = out.cpu().numpy() if isinstance(out, torch.Tensor) else np.stack([np.asarray(f) for f in out])
    return out, [np.asarray(f) for f in rig.proc.last_restored_faces], seen.get('crops'), seen.get('plan')


def _paths_agree(rig, frames, n, K, clip, chunks):
    """Knob on: the default setting (store + streamed paste), no store, no streamed paste -- identical frames and restored faces, and
    those faces are the per-track runs of the engine."""
    net_ = rig.proc.keep_net
    rig.proc.track_clips = True
    got, got_faces, st_crops, st_plan = _run(rig, frames, clip=clip)
    assert rig.crop_shapes == [('Tensor', n * K)] and st_plan is not None            # the store took the sequence
    assert rig.count(SCATTER) == chunks and rig.count(WARP_BATCH) == 0               # one scatter call per chunk
    nostore, nostore_faces, crops, plan = _run(rig, frames, env=[('KEEP_AMD_FRAME_STORE', '0')], clip=clip)
    assert rig.crop_shapes == [('list', n * K)] and rig.count(SCATTER) == 0 and plan == st_plan
    perframe, perframe_faces, none, _ = _run(rig, frames, env=[('KEEP_AMD_STREAM_PASTE', '0')], clip=clip)
    assert none is None and rig.crop_shapes == [] and rig.count(SCATTER) == 0
    assert got.shape == nostore.shape == perframe.shape and got.shape[0] == n
    assert np.array_equal(got, nostore) and np.array_equal(got, perframe)
    assert len(got_faces) == len(nostore_faces) == len(perframe_faces) == n * K
    for i in range(n * K):
        assert np.array_equal(got_faces[i], nostore_faces[i]) and np.array_equal(got_faces[i], perframe_faces[i]), i
    # the store's crop tensor is the crop list laid out by slot
    clips, slot_of = st_plan
    for i in range(n * K):
        assert torch.equal(st_crops[slot_of[i]], crops[i]), i
    # per track: its crops cut into clips of `clip`, each track restored in a run of its own
    assert [len(m) for m in clips] == [min(clip, n - s) for s in range(0, n, clip) for _ in range(K)]
    for j in range(K):
        track = torch.stack([crops[t * K + j] for t in range(n)])
        outs = net_.run_clips_u8([track[s:s + clip] for s in range(0, n, clip)])
        for t in range(n):
            assert np.array_equal(outs[t // clip][t % clip].numpy(), got_faces[t * K + j]), (j, t)
    # ... which is not what the default order gives
    rig.proc.track_clips = False
    off, off_faces, _, off_plan = _run(rig, frames, clip=clip)
    assert off_plan is None and rig.count(SCATTER) == 0 and rig.count(WARP_BATCH) == chunks
    assert any(not np.array_equal(a, b) for a, b in zip(off_faces, got_faces)) and not np.array_equal(off, got)
    return got, got_faces


def test_paths_agree_and_equal_the_per_track_runs(net, monkeypatch):
    """6 frames of 512 x 512 (the smallest frame ``read_image`` leaves alone), 2 face tracks, clips of 4, detection chunks of 4 frames."""
    rig = Rig(net, monkeypatch, (512, 512), 2, chunk=4)
    _paths_agree(rig, video(6, 512, 512, seed=31), 6, 2, 4, chunks=2)


def test_paths_agree_for_small_frames(net, monkeypatch):
    """The same at 480 x 640 (enlarged by ``read_image`` to 512 x 683): the small-frame store."""
    from test_gpu_small_frames import ENLARGE, SmallRig
    rig = SmallRig(net, monkeypatch, (480, 640), 2, chunk=4)
    assert rig.hw2 == (512, 683)
    got, _ = _paths_agree(rig, video(6, 480, 640, seed=32), 6, 2, 4, chunks=2)
    assert got.shape == (6, 512, 683, 3) and rig.proc.gpu_small_frames is True
    assert rig.count(ENLARGE) == 2                                                   # (the last run: the store's small-frame form took it)


def test_single_face_video_is_untouched_by_the_knob(net, monkeypatch):
    """only_center_face: one track on every frame -- the plan is the cut of the flat list and the identity permutation, so knob on equals
    knob off bit for bit, on the store path and without it."""
    rig = Rig(net, monkeypatch, (512, 512), 2, chunk=4)
    frames = video(6, 512, 512, seed=31)
    for env in ((), (('KEEP_AMD_FRAME_STORE', '0'),)):
        rig.proc.track_clips = False
        off, off_faces, _, off_plan = _run(rig, frames, env=env, center=True)
        rig.proc.track_clips = True
        on, on_faces, _, on_plan = _run(rig, frames, env=env, center=True)
        assert off_plan is None and on_plan == ([[0, 1, 2, 3], [4, 5]], list(range(6)))
        assert np.array_equal(on, off) and len(on_faces) == len(off_faces) == 6
        assert all(np.array_equal(a, b) for a, b in zip(on_faces, off_faces))
        assert (on != np.stack(frames)).any()


def test_single_image_restores_every_face_alone(net, monkeypatch):
    """``process_image`` on a frame with two faces: knob on, each restored face is the T = 1 result of its crop; knob off (one clip of
    T = 2, reference quirk P3) the second face is not."""
    rig = Rig(net, monkeypatch, (512, 512), 2, chunk=4)
    frame = video(1, 512, 512, seed=33)[0]
    res = {}
    for knob in (True, False):
        rig.proc.track_clips = knob
        rig.helper.begin_sequence()
        out = rig.proc.process_image(frame, 1.0, False, False, False)
        assert out.shape == frame.shape and (out != frame).any()
        res[knob] = (out, [np.asarray(f) for f in rig.proc.last_restored_faces], [np.asarray(c) for c in rig.helper.cropped_faces])
    crops = res[True][2]
    assert len(crops) == 2 and all(np.array_equal(a, b) for a, b in zip(crops, res[False][2]))
    alone = [net.run_clips_u8([torch.from_numpy(c[None].copy())])[0][0].numpy() for c in crops]
    assert all(np.array_equal(a, b) for a, b in zip(res[True][1], alone))
    assert np.array_equal(res[False][1][0], alone[0]) and not np.array_equal(res[False][1][1], alone[1])
    assert not np.array_equal(res[True][0], res[False][0])
