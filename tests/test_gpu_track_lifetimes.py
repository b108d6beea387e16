"""GPU suite (-m gpu): track lifetimes (KEEP_AMD_TRACK_LIFETIMES; modules/face_tracks.py, modules/keep_processor.py) and the fade at a
lifetime's ends (KEEP_AMD_TRACK_FADE; keep_paste_face_w) through the product's own entry points over tools/synth_facehelper.py.

Nothing in the reference ends a track, so there is no reference output to compare the mode with.  What is proved instead: the frames of
a lifetime and their restored faces equal that lifetime's frames processed as a video of their own, BIT FOR BIT -- on every path a
sequence takes, with the carried state, with scene cuts, with two faces, and with a detector miss inside the lifetime --; frames outside
every lifetime come back as a video without detections returns them; and a faded frame is the composite of the same restored faces with
the weights the rule gives, done by hand through ``GpuPaster``.

The set-up: 512 x 512 frames (the smallest ``read_image`` leaves alone, so the frame store runs), clips of 4, detection chunks of 4, 12
to 14 frames.  The synthetic helper detects every face on every frame, so a wrapper around the smoothers drops detections from the raw
landmarks (as tests/test_gpu_frame_store.py blanks smoothed tracks); its landmarks follow the helper's frame counter, so a sub-video
that starts at frame a starts the counter at a."""
import os
import sys

import numpy as np
import pytest
import torch

from test_gpu_frame_store import Rig, net  # noqa: F401  (``net``: the module's fixture)

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))

W = 'keep_paste_face_w'
PATHS = {'store': (), 'streamed': (('KEEP_AMD_FRAME_STORE', '0'),), 'per-frame': (('KEEP_AMD_STREAM_PASTE', '0'),)}


def video(n, seed, h=512, w=512, lo=0, hi=256):
    return [f for f in np.random.default_rng(seed).integers(lo, hi, (n, h, w, 3), dtype=np.uint8)]


class Drops:
    """Detections (frame, face) taken out of the raw landmarks in front of both smoothers; ``offset``: the video's first frame in the
    numbering of ``drop``."""

    def __init__(self, monkeypatch):
        from comfyui_keep_amd.modules import keep_processor as KP
        self.drop, self.offset = set(), 0
        for name in ('smooth_tracked_faces', 'smooth_center_face'):
            monkeypatch.setattr(KP, name, self._wrap(getattr(KP, name)))

    def _wrap(self, real):
        def smooth(raw, *a, **kw):
            raw = [[lm for j, lm in enumerate(faces) if (t + self.offset, j) not in self.drop] for t, faces in enumerate(raw)]
            return real(raw, *a, **kw)
        return smooth


def run(rig, drops, frames, start=0, drop=(), env=(), clip=4):
    """One ``process_frames_u8`` call with the helper's frame counter at ``start`` -> (frames as a list of uint8 arrays, restored faces,
    the plan the streamed paste was handed or None)."""
    for k in ('KEEP_AMD_FRAME_STORE', 'KEEP_AMD_STREAM_PASTE', 'KEEP_AMD_DETECT_BATCH'):
        rig.mp.delenv(k, raising=False)
    for k, v in env:
        rig.mp.setenv(k, v)
    rig.mp.setenv('KEEP_AMD_STREAM_GROUPS', '3')
    for rec in (rig.calls, rig.backgrounds, rig.batches, rig.crop_shapes):
        rec.clear()
    drops.drop, drops.offset = set(drop), start
    seen = {}
    inner = rig.proc._restore_and_paste_streamed

    def streamed(frames_bgr, crops, *a, **kw):
        seen['plan'] = kw.get('plan')
        return inner(frames_bgr, crops, *a, **kw)
    rig.mp.setattr(rig.proc, '_restore_and_paste_streamed', streamed)
    rig.helper.frame_index = start                       # (not begin_sequence(): that resets the counter)
    try:
        out = rig.proc.process_frames_u8(frames, 1.0, False, False, False, max_clip_length=clip)
    finally:
        rig.mp.setattr(rig.proc, '_restore_and_paste_streamed', inner)
    out = [f for f in out.cpu().numpy()] if isinstance(out, torch.Tensor) else [np.asarray(f) for f in out]
    return out, [np.asarray(f) for f in rig.proc.last_restored_faces], seen.get('plan')


def same_frames(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def knobs(proc, **kw):
    for k in ('track_clips', 'track_carry', 'scene_cuts', 'track_lifetimes'):
        setattr(proc, k, bool(kw.get(k, False)))
    proc.track_max_gap, proc.track_fade = kw.get('max_gap', 10), kw.get('fade', 0)


N, A, B = 12, 3, 9                                       # one face, detected on frames A .. B of N


def outside(n, a, b, faces=(0,)):
    return {(t, j) for t in range(n) for j in faces if t < a or t > b}


@pytest.mark.parametrize('path', list(PATHS))
@pytest.mark.parametrize('variant', ['plain', 'carry', 'cuts'])
def test_a_lifetime_equals_its_frames_processed_as_a_video_of_their_own(net, monkeypatch, path, variant):
    rig = Rig(net, monkeypatch, (512, 512), 1, chunk=4)
    drops = Drops(monkeypatch)
    env = PATHS[path]
    carry = variant == 'carry'
    if variant == 'cuts':                                # a hard cut at frame 6, inside the lifetime: no luma bin is shared
        cut = 6
        frames = video(cut, 61, hi=128) + video(N - cut, 62, lo=128)
        pieces = [(A, cut - 1), (cut, B)]
    else:
        frames = video(N, 60)
        pieces = [(A, B)]
    knobs(rig.proc, track_lifetimes=True, track_carry=carry, scene_cuts=variant == 'cuts')
    out, faces, plan = run(rig, drops, frames, drop=outside(N, A, B), env=env)
    assert rig.count(W) == 0
    assert len(out) == N and len(faces) == B - A + 1                                  # one crop per live frame
    assert rig.crop_shapes == ({'store': [('Tensor', B - A + 1)], 'streamed': [('list', B - A + 1)], 'per-frame': []}[path])
    if variant == 'cuts':
        assert rig.proc.last_scene_cuts == [cut]
        assert rig.proc.last_track_lifetimes == [((0, 0), A, cut - 1, cut - A), ((1, 0), cut, B, B - cut + 1)]
    else:
        assert rig.proc.last_track_lifetimes == [(0, A, B, B - A + 1)]
    if carry and plan is not None:
        assert plan[2] == [None, 0]                                                   # [3-6] then [7-9], which continues it
    # outside the lifetime: what a video without detections returns -- the frames as they came
    for t in list(range(A)) + list(range(B + 1, N)):
        assert np.array_equal(out[t], frames[t]), t
    # inside: the lifetime's frames processed alone, with track clips (and the same carry)
    knobs(rig.proc, track_clips=True, track_carry=carry)
    k = 0
    for a, b in pieces:
        sub, sub_faces, _ = run(rig, drops, frames[a:b + 1], start=a, env=env)
        assert len(sub_faces) == b - a + 1
        assert same_frames(out[a:b + 1], sub), (a, b)
        assert all(np.array_equal(x, y) for x, y in zip(faces[k:k + b - a + 1], sub_faces)), (a, b)
        assert all((out[t] != frames[t]).any() for t in range(a, b + 1))              # (faces were really pasted)
        k += b - a + 1


def test_a_video_without_detections_returns_its_frames(net, monkeypatch):
    rig = Rig(net, monkeypatch, (512, 512), 1, chunk=4)
    drops = Drops(monkeypatch)
    frames = video(5, 63)
    for on in (True, False):
        knobs(rig.proc, track_lifetimes=on)
        out, faces, _ = run(rig, drops, frames, drop=outside(5, 9, 9))
        assert same_frames(out, frames) and faces == [] and rig.crop_shapes == []


def test_two_faces_with_different_lifetimes_each_equal_their_own_sub_video(net, monkeypatch):
    """Face 0 on frames 0-7, face 1 on 4-11: chain 0 and chain 1.  Every track's restored faces equal that track's sub-video processed
    alone (the engine is batch invariant: tests/test_gpu_track_clips.py); where one face is alone in the picture the frames are equal
    too."""
    rig = Rig(net, monkeypatch, (512, 512), 2, chunk=4)
    drops = Drops(monkeypatch)
    frames = video(N, 64)
    life = {0: (0, 7), 1: (4, 11)}
    drop = {(t, j) for j, (a, b) in life.items() for t in range(N) if t < a or t > b}
    knobs(rig.proc, track_lifetimes=True)
    out, faces, _ = run(rig, drops, frames, drop=drop)
    assert rig.proc.last_track_lifetimes == [(0, 0, 7, 8), (1, 4, 11, 8)] and len(faces) == 16
    assert rig.crop_shapes == [('Tensor', 16)]
    order = [(t, j) for t in range(N) for j in (0, 1) if life[j][0] <= t <= life[j][1]]   # frame-major, tracks in key order
    knobs(rig.proc, track_clips=True)
    for j, (a, b) in life.items():
        other = {(t, 1 - j) for t in range(N)}
        sub, sub_faces, _ = run(rig, drops, frames[a:b + 1], start=a, drop=other)
        assert len(sub_faces) == b - a + 1
        mine = [faces[i] for i, (t, jj) in enumerate(order) if jj == j]
        assert all(np.array_equal(x, y) for x, y in zip(mine, sub_faces)), j
        alone = [t for t in range(a, b + 1) if not life[1 - j][0] <= t <= life[1 - j][1]]
        assert len(alone) == 4 and all(np.array_equal(out[t], sub[t - a]) for t in alone), j
    assert all((out[t] != frames[t]).any() for t in range(N))


@pytest.mark.parametrize('carry', [False, True], ids=['plain', 'carry'])
def test_a_one_frame_miss_inside_a_lifetime(net, monkeypatch, carry):
    """One face on frames 2-10 of 14, missed on frame 6.  Today: the track dies at the miss, the same person starts a second track, and
    both are held over the whole video -- 28 crops for 8 detections.  With lifetimes: one track, 9 crops (the miss is interpolated)."""
    n, a, b, miss = 14, 2, 10, 6
    rig = Rig(net, monkeypatch, (512, 512), 1, chunk=4)
    drops = Drops(monkeypatch)
    frames = video(n, 65)
    drop = outside(n, a, b) | {(miss, 0)}
    knobs(rig.proc, track_lifetimes=True, track_carry=carry)
    out, faces, plan = run(rig, drops, frames, drop=drop)
    live = b - a + 1
    print('restored crops', len(faces), 'live frames', live, 'frames', n)
    assert len(faces) == live                                                         # THE assertion that fails without the feature (2 n)
    assert rig.proc.last_track_lifetimes == [(0, a, b, live - 1)]
    assert [len(m) for m in plan[0]] == [4, 4, 1]
    if carry:
        assert plan[2] == [None, 0, 1]                                                # the chain runs through the gap
    sub, sub_faces, sub_plan = run(rig, drops, frames[a:b + 1], start=a, drop=drop)   # the sub-video with the same knobs
    assert rig.proc.last_track_lifetimes == [(0, 0, b - a, live - 1)]
    assert same_frames(out[a:b + 1], sub) and len(sub_faces) == live
    assert all(np.array_equal(x, y) for x, y in zip(faces, sub_faces))
    assert all(np.array_equal(out[t], frames[t]) for t in range(n) if t < a or t > b)
    assert (out[miss] != frames[miss]).any()                                          # the missed frame is restored from the interpolation
    if not carry:
        knobs(rig.proc, track_clips=True)                                             # today's tracks under the same clip rule
        _, off_faces, _ = run(rig, drops, frames, drop=drop)
        assert len(off_faces) == 2 * n


def test_knob_off_is_an_untouched_processor(net, monkeypatch):
    frames = video(8, 66)
    fresh = Rig(net, monkeypatch, (512, 512), 2, chunk=4)
    drops = Drops(monkeypatch)
    drop = {(3, 1)}
    want = run(fresh, drops, frames, drop=drop)
    assert fresh.proc.track_lifetimes is False and not hasattr(fresh.proc, 'last_track_lifetimes') and fresh.count(W) == 0
    rig = Rig(net, monkeypatch, (512, 512), 2, chunk=4)
    knobs(rig.proc, track_lifetimes=True, fade=2)
    on = run(rig, drops, frames, drop=drop)
    assert rig.proc.last_track_lifetimes == [(0, 0, 7, 8), (1, 0, 7, 7)] and rig.count(W) == 0   # every end is an end of the video: no fade
    knobs(rig.proc)
    rig.proc.track_fade = 2                                                           # (a fade without lifetimes is nothing)
    off = run(rig, drops, frames, drop=drop)
    assert rig.count(W) == 0 and off[2] is None
    assert same_frames(off[0], want[0]) and len(off[1]) == len(want[1]) == 24 and all(np.array_equal(x, y) for x, y in zip(off[1], want[1]))
    assert len(on[1]) == 16 and not same_frames(on[0], off[0])


def test_small_frames_with_a_faceless_frame_equal_the_per_frame_path(net, monkeypatch):
    """360 x 480 frames (``read_image`` enlarges them to 512 x 683), one face on frames 0-3 of 6: the faceless frames keep their size, so
    the small-frame form of the store leaves the sequence as it always did -- the result is the per-frame path's."""
    from test_gpu_small_frames import SmallRig
    rig = SmallRig(net, monkeypatch, (360, 480), 1, chunk=4)
    drops = Drops(monkeypatch)
    frames = video(6, 67, 360, 480)
    knobs(rig.proc, track_lifetimes=True)
    drop = outside(6, 0, 3)
    got, got_faces, _ = run(rig, drops, frames, drop=drop)
    assert [f.shape for f in got] == [(512, 683, 3)] * 4 + [(360, 480, 3)] * 2
    ref, ref_faces, _ = run(rig, drops, frames, drop=drop, env=PATHS['per-frame'])
    assert rig.crop_shapes == []
    assert same_frames(got, ref) and len(got_faces) == len(ref_faces) == 4 and all(np.array_equal(x, y) for x, y in zip(got_faces, ref_faces))
    assert np.array_equal(got[4], frames[4]) and np.array_equal(got[5], frames[5])


def test_fade_ramps_the_paste_weight_at_the_ends_of_an_interior_lifetime(net, monkeypatch):
    """``track_fade`` = 2 on the store path, one face on frames 3-9 of 12: frames 3, 4 and 9, 8 are the composite of the SAME restored
    faces at weights 1/3 and 2/3, done here by hand through ``GpuPaster``; frames 5-7 are the unfaded run's."""
    from comfyui_keep_amd.engine import hiplib as L
    from comfyui_keep_amd.engine.paste import GpuPaster
    rig = Rig(net, monkeypatch, (512, 512), 1, chunk=4)
    drops = Drops(monkeypatch)
    inverse, own = [], rig.helper.get_inverse_affine

    def rec(*a, **kw):
        own(*a, **kw)
        inverse.append([np.array(M) for M in rig.helper.inverse_affine_matrices])
    rig.helper.get_inverse_affine = rec
    frames = video(N, 68)
    drop = outside(N, A, B)
    knobs(rig.proc, track_lifetimes=True)
    plain, plain_faces, _ = run(rig, drops, frames, drop=drop)
    assert rig.count(W) == 0
    inverse.clear()
    knobs(rig.proc, track_lifetimes=True, fade=2)
    out, faces, _ = run(rig, drops, frames, drop=drop)
    assert rig.crop_shapes == [('Tensor', B - A + 1)] and rig.count(W) == 4 and len(inverse) == B - A + 1
    assert len(faces) == len(plain_faces) and all(np.array_equal(x, y) for x, y in zip(faces, plain_faces))   # the fade is in the paste alone
    third, two = float(np.float32(1.0 / 3.0)), float(np.float32(2.0 / 3.0))
    weight = {A: third, A + 1: two, B - 1: two, B: third}
    paster = GpuPaster('cuda')
    for t in range(N):
        if t in weight:
            fd = torch.from_numpy(faces[t - A][None]).cuda()
            x = torch.empty(fd.shape, dtype=torch.float32, device='cuda')
            L.call('keep_img2tensor', fd, x, fd.numel() // 3)
            cls = rig.helper.face_parse.engine.classes(x)
            want = paster.paste(frames[t], fd, inverse[t - A], cls, 1.0, False, weights=[weight[t]]).cpu().numpy()
            assert np.array_equal(out[t], want), t
            assert not np.array_equal(out[t], plain[t]) and not np.array_equal(out[t], frames[t]), t
        else:
            assert np.array_equal(out[t], plain[t]), t
