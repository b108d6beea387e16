"""GPU suite (-m gpu): scene cuts (KEEP_AMD_SCENE_CUTS; modules/scene_cuts.py, modules/face_tracks.py, modules/keep_processor.py,
keep_frame_signature_u8) through the product's own entry points over tools/synth_facehelper.py.

Nothing in the reference finds a cut, so there is no reference output to compare the mode with.  What is proved instead: a video made
of scene A then scene B, processed with the knob on, equals A and B processed as two videos, BIT FOR BIT -- output frames and restored
faces, with one face and with two, on every path a sequence takes, with the carried state as well, and for an aligned sequence.

The set-up: A is 5 frames of ``integers(0, 128)``, B 3 frames of ``integers(128, 256)`` at 512 x 512 (no luma bin is shared: the
distance at the boundary is exactly 1), clips of 4, detection chunks of 4: the cut lies inside a chunk and, in the flat order, inside a
clip.  The synthetic helper's landmarks follow its frame counter, not the pixels, so the separate run of B starts the counter at 5:
the two people are framed alike on either side of the cut, which is the case that fools the tracker."""
import os
import sys

import numpy as np
import pytest
import torch

from test_gpu_frame_store import Rig, net  # noqa: F401  (``net``: the module's fixture)

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))

SIG = 'keep_frame_signature_u8'
NA, NB = 5, 3


def scenes(seed=51):
    rng = np.random.default_rng(seed)
    A = [f for f in rng.integers(0, 128, (NA, 512, 512, 3), dtype=np.uint8)]
    B = [f for f in rng.integers(128, 256, (NB, 512, 512, 3), dtype=np.uint8)]
    return A, B


def run(rig, frames, start=0, center=False, clip=4, env=(), aligned=False):
    """One ``process_frames_u8`` call with the helper's frame counter at ``start`` -> (frames uint8 [n,H,W,3], restored faces)."""
    for k in ('KEEP_AMD_FRAME_STORE', 'KEEP_AMD_STREAM_PASTE', 'KEEP_AMD_DETECT_BATCH'):
        rig.mp.delenv(k, raising=False)
    for k, v in env:
        rig.mp.setenv(k, v)
    rig.mp.setenv('KEEP_AMD_STREAM_GROUPS', '3')
    for rec in (rig.calls, rig.backgrounds, rig.batches, rig.crop_shapes):
        rec.clear()
    rig.helper.frame_index = start                       # (not begin_sequence(): that resets the counter)
    out = rig.proc.process_frames_u8(frames, 1.0, aligned, center, False, max_clip_length=clip)
    out = out.cpu().numpy() if isinstance(out, torch.Tensor) else np.stack([np.asarray(f) for f in out])
    return out, [np.asarray(f) for f in rig.proc.last_restored_faces]


def same(a, b):
    return a[0].shape == b[0].shape and np.array_equal(a[0], b[0]) and len(a[1]) == len(b[1]) and \
        all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))


def glued(a, b):
    return np.concatenate([a[0], b[0]]), a[1] + b[1]


@pytest.mark.parametrize('faces,center', [(1, False), (2, False), (2, True)], ids=['one-face', 'two-faces', 'center-face'])
def test_two_scenes_equal_the_scenes_processed_as_two_videos(net, monkeypatch, faces, center):
    rig = Rig(net, monkeypatch, (512, 512), faces, chunk=4)
    A, B = scenes()
    K = 1 if center else faces
    rig.proc.scene_cuts = True
    ab = run(rig, A + B, center=center)
    assert rig.proc.last_scene_cuts == [NA] and rig.count(SIG) == 2                   # one launch per store chunk
    d = rig.proc.last_scene_distances
    assert d.shape == (NA + NB - 1,) and d[NA - 1] == 1.0 and (np.delete(d, NA - 1) < 0.02).all()
    assert rig.crop_shapes == [('Tensor', (NA + NB) * K)]                             # the store took the sequence
    a = run(rig, A, center=center)
    assert rig.proc.last_scene_cuts == [] and rig.count(SIG) == 2
    b = run(rig, B, start=NA, center=center)
    assert rig.proc.last_scene_cuts == [] and rig.count(SIG) == 1
    assert ab[0].shape == (NA + NB, 512, 512, 3) and len(ab[1]) == (NA + NB) * K
    assert same(ab, glued(a, b))
    assert (ab[0] != np.stack(A + B)).any(axis=(1, 2, 3)).all()                       # (faces were really pasted, on every frame)
    # knob off: the track runs on over the cut, the smoothing blends the two sides and a clip spans the boundary
    rig.proc.scene_cuts = False
    off = run(rig, A + B, center=center)
    assert rig.count(SIG) == 0
    near = [t for t in range(NA + NB) if not np.array_equal(off[0][t], ab[0][t])]
    assert near and NA - 1 in near and NA in near, near                               # THE assertion that fails without the feature
    assert not same(off, ab)


def test_paths_agree_and_only_the_store_path_launches_the_kernel(net, monkeypatch):
    rig = Rig(net, monkeypatch, (512, 512), 2, chunk=4)
    A, B = scenes(52)
    rig.proc.scene_cuts = True
    store = run(rig, A + B)
    assert rig.count(SIG) == 2 and rig.proc.last_scene_cuts == [NA] and rig.crop_shapes == [('Tensor', 16)]
    d_store = rig.proc.last_scene_distances.copy()
    nostore = run(rig, A + B, env=[('KEEP_AMD_FRAME_STORE', '0')])
    assert rig.count(SIG) == 0 and rig.proc.last_scene_cuts == [NA] and rig.crop_shapes == [('list', 16)]
    assert np.array_equal(rig.proc.last_scene_distances, d_store)                    # the host function gives the kernel's integers
    perframe = run(rig, A + B, env=[('KEEP_AMD_STREAM_PASTE', '0')])
    assert rig.count(SIG) == 0 and rig.proc.last_scene_cuts == [NA] and rig.crop_shapes == []
    assert np.array_equal(rig.proc.last_scene_distances, d_store)
    assert same(store, nostore) and same(store, perframe)


def test_a_failing_signature_launch_costs_the_launch_not_the_store(net, monkeypatch):
    """The kernel call raises: one warning, the host function takes the signatures, the sequence stays on the store and the processor
    keeps its store for later calls -- the same frames and faces."""
    from comfyui_keep_amd.engine import hiplib as L
    rig = Rig(net, monkeypatch, (512, 512), 2, chunk=4)
    A, B = scenes(52)
    rig.proc.scene_cuts = True
    want = run(rig, A + B)
    recording = L.call

    def failing(name, *a):
        if name == SIG:
            raise L.KeepHipError('made to fail')
        return recording(name, *a)
    monkeypatch.setattr(L, 'call', failing)
    got = run(rig, A + B)
    monkeypatch.setattr(L, 'call', recording)
    assert rig.count(SIG) == 0 and rig.proc.last_scene_cuts == [NA] and rig.crop_shapes == [('Tensor', 16)]
    assert rig.proc.frame_store is True and same(got, want)
    again = run(rig, A + B)
    assert rig.count(SIG) == 2 and same(again, want)


def test_knob_off_is_an_untouched_processor_and_a_high_threshold_is_track_clips(net, monkeypatch):
    A, B = scenes(53)
    fresh = Rig(net, monkeypatch, (512, 512), 2, chunk=4)
    want = run(fresh, A + B)
    assert fresh.count(SIG) == 0 and not hasattr(fresh.proc, 'last_scene_cuts') and fresh.proc.scene_cuts is False
    rig = Rig(net, monkeypatch, (512, 512), 2, chunk=4)
    rig.proc.scene_cuts = True
    rig.proc.scene_cut_threshold = 1.5                                               # no distance reaches it: no cuts
    high = run(rig, A + B)
    assert rig.proc.last_scene_cuts == [] and rig.count(SIG) == 2
    rig.proc.scene_cuts = False
    off = run(rig, A + B)
    assert rig.count(SIG) == 0 and same(off, want)
    rig.proc.track_clips = True
    clips = run(rig, A + B)
    assert rig.count(SIG) == 0 and same(high, clips) and not same(clips, off)


def test_nothing_is_carried_across_a_cut(net, monkeypatch):
    """With ``track_carry`` on as well: [A;B] equals A and B run separately with carry -- the first clip of B starts from nothing -- and
    differs from carry without the knob, which hands scene A's state to scene B."""
    rig = Rig(net, monkeypatch, (512, 512), 2, chunk=4)
    A, B = scenes(54)
    rig.proc.track_carry = rig.proc.scene_cuts = True
    ab = run(rig, A + B, center=True)
    assert rig.proc.last_scene_cuts == [NA]
    a = run(rig, A, center=True)
    b = run(rig, B, start=NA, center=True)
    assert same(ab, glued(a, b))
    rig.proc.scene_cuts = False
    carried = run(rig, A + B, center=True)
    assert not same(carried, ab)
    assert any(not np.array_equal(x, y) for x, y in zip(carried[1][NA:], ab[1][NA:]))   # scene B's faces


def test_aligned_sequence_is_cut_per_scene(net, monkeypatch):
    """5 + 3 aligned frames with the restored faces returned: the device-resident path (one kernel launch on the uploaded chunk) and
    the per-frame path (the host function) equal the two scenes run separately."""
    rig = Rig(net, monkeypatch, (512, 512), 1, chunk=4)
    rig.proc.return_restored_aligned = True
    A, B = scenes(55)
    rig.proc.scene_cuts = True
    ab = run(rig, A + B, aligned=True)
    assert rig.proc.last_scene_cuts == [NA] and rig.count(SIG) == 1
    a = run(rig, A, aligned=True)
    b = run(rig, B, aligned=True)
    assert same(ab, glued(a, b)) and len(ab[1]) == NA + NB and np.array_equal(ab[0], np.stack(ab[1]))
    perframe = run(rig, A + B, aligned=True, env=[('KEEP_AMD_STREAM_PASTE', '0')])
    assert rig.proc.last_scene_cuts == [NA] and rig.count(SIG) == 0 and same(perframe, ab)
    rig.proc.scene_cuts = False
    off = run(rig, A + B, aligned=True)
    assert rig.count(SIG) == 0 and not same(off, ab)
    assert np.array_equal(off[0][:4], ab[0][:4]) and not np.array_equal(off[0][4:], ab[0][4:])   # [0-4) is a clip either way
