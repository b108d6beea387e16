"""Track lifetimes (KEEP_AMD_TRACK_LIFETIMES), host side (no GPU): the rule in modules/face_tracks.py -- stitching raw tracks over short
gaps, a track alive from its first to its last detection only, the only_center_face split, lifetimes inside scenes --, what the clip
planner makes of such tracks, the fade weights, the processor's knobs over fake nets, the new entry point keep_paste_face_w (header,
binding, library, host refusals) and the restatement tests/paste_fade_ref.py against oracle/paste_oracle.py."""
import ctypes
import logging
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import paste_fade_ref as FR
import paste_oracle as P
from comfyui_keep_amd.modules import face_tracks as FT
from comfyui_keep_amd.modules import scene_cuts as SC
from comfyui_keep_amd.modules.clip_plan import plan_track_chains

NAME = 'keep_paste_face_w'


def _lm(cx, cy, jitter=0.0):
    base = np.array([[-30.0, -20.0], [30.0, -20.0], [0.0, 10.0], [-25.0, 40.0], [25.0, 40.0]])
    return base + np.array([cx, cy]) + jitter


def _one_face(n, seen, rng, x0=300.0, dx=1.0):
    return [[_lm(x0 + dx * t, 300, rng.normal(0, 1.0, (5, 2)))] if t in seen else [] for t in range(n)]


def _presence(tracks, n):
    return [[k for k, seq in tracks.items() if not np.isnan(seq[t]).any()] for t in range(n)]


def _crops(tracks, n):
    return sum(len(p) for p in _presence(tracks, n))


def _live(seq):
    return [t for t in range(len(seq)) if not np.isnan(seq[t]).any()]


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('max_gap', [1, 2, 10])
def test_one_miss_is_one_track_that_lives_on_its_own_frames(max_gap):
    """The issue's example: one face detected on frames 0-4 and 6-9 of 30."""
    n = 30
    raw = _one_face(n, set(range(0, 5)) | set(range(6, 10)), np.random.default_rng(1))
    off = FT.smooth_tracked_faces(raw)
    assert len(off) == 2 and _crops(off, n) == 60                                     # today: two tracks, each on every frame
    report = []
    on = FT.smooth_tracked_faces(raw, lifetimes=max_gap, report=report)
    assert list(on) == [0] and _live(on[0]) == list(range(10)) and _crops(on, n) == 10
    assert report == [(0, 0, 9, 9)]
    # the gap is interpolated and the lifetime is smoothed as a video of its own
    seq = np.full((10, 10), np.nan)
    for t in range(10):
        if raw[t]:
            seq[t] = raw[t][0].reshape(10)
    assert _same(on[0][:10], FT._smooth(seq))
    # max_gap = 0 stitches nothing: two tracks, each alive on its own run
    zero = FT.smooth_tracked_faces(raw, lifetimes=0)
    assert list(zero) == [0, 1] and _live(zero[0]) == list(range(5)) and _live(zero[1]) == list(range(6, 10))


def test_a_gap_longer_than_max_gap_is_two_lifetimes_and_nothing_is_carried_between_them():
    n = 20
    raw = _one_face(n, set(range(2, 7)) | set(range(10, 16)), np.random.default_rng(2))
    report = []
    on = FT.smooth_tracked_faces(raw, lifetimes=2, report=report)                      # the gap is 3 frames
    assert list(on) == [0, 1] and report == [(0, 2, 6, 5), (1, 10, 15, 6)]
    assert _live(on[0]) == list(range(2, 7)) and _live(on[1]) == list(range(10, 16))
    one = FT.smooth_tracked_faces(raw, lifetimes=3)
    assert list(one) == [0] and _live(one[0]) == list(range(2, 16))
    presence = _presence(on, n)
    clips, slot_of, after = plan_track_chains(presence, 4)
    frame_of = [t for t in range(n) for _ in presence[t]]
    starts = [frame_of[m[0]] for m in clips]
    assert starts == [2, 6, 10, 14] and after == [None, 0, None, 2]                  # the first clip of the second lifetime starts from nothing


def test_entrance_and_exit():
    n = 40
    raw = _one_face(n, set(range(12, 21)), np.random.default_rng(3))
    today = FT.smooth_tracked_faces(raw)
    assert not np.isnan(today[0]).any()                                              # np.interp holds the end values: a face on all 40 frames
    for smooth in (FT.smooth_tracked_faces, FT.smooth_center_face):
        on = smooth(raw, lifetimes=10)
        assert list(on) == [0]
        assert np.isnan(on[0][:12]).all() and np.isnan(on[0][21:]).all() and not np.isnan(on[0][12:21]).any()
        assert _same(on[0][12:21], FT._smooth([raw[t][0].reshape(10) for t in range(12, 21)]))
    # a lifetime of one detection is legal
    single = FT.smooth_tracked_faces(_one_face(7, {3}, np.random.default_rng(4)), lifetimes=10)
    assert list(single) == [0] and _live(single[0]) == [3]


def _two_faces(n, rng, drop=(), a=(200.0, 2.0), b=(600.0, -1.5)):
    raw = []
    for t in range(n):
        faces = [_lm(a[0] + a[1] * t, 300, rng.normal(0, 1.0, (5, 2))), _lm(b[0] + b[1] * t, 320, rng.normal(0, 1.0, (5, 2)))]
        raw.append([f for j, f in enumerate(faces) if (t, j) not in drop])
    return raw


def test_stitching_relinks_each_face_to_its_own_chain():
    n = 12
    drop = {(t, j) for t in (5, 6) for j in (0, 1)}                                  # both faces vanish for 2 frames
    raw = _two_faces(n, np.random.default_rng(5), drop)
    assert len(FT.track_faces(raw)) == 4
    report = []
    on = FT.smooth_tracked_faces(raw, lifetimes=2, report=report)
    assert list(on) == [0, 1] and report == [(0, 0, 11, 10), (1, 0, 11, 10)]
    assert abs(on[0][11].mean(axis=0)[0] - (200 + 2.0 * 11)) < 10 and abs(on[1][11].mean(axis=0)[0] - (600 - 1.5 * 11)) < 10
    assert not np.isnan(on[0]).any() and not np.isnan(on[1]).any()
    assert len(FT.smooth_tracked_faces(raw, lifetimes=1)) == 4                       # a 2-frame gap is beyond max_gap = 1
    # the same result out of every run
    again = FT.smooth_tracked_faces(raw, lifetimes=2)
    assert list(again) == list(on) and all(_same(again[k], on[k]) for k in on)
    chains = FT.stitch_tracks(FT.track_faces(raw), 2)
    assert chains == FT.stitch_tracks(FT.track_faces(raw), 2) == [[0, 2], [1, 3]]


def test_a_start_beyond_the_trackers_distance_starts_a_new_chain():
    rng = np.random.default_rng(6)
    n = 10
    raw = [[_lm(300, 300, rng.normal(0, 0.5, (5, 2)))] if t < 4 else [] for t in range(n)]
    for t in range(6, n):
        raw[t] = [_lm(380, 300, rng.normal(0, 0.5, (5, 2)))]                         # 80 px away: not the same person by the tracker's measure
    far = FT.smooth_tracked_faces(raw, lifetimes=5)
    assert list(far) == [0, 1] and _live(far[0]) == [0, 1, 2, 3] and _live(far[1]) == [6, 7, 8, 9]
    for t in range(6, n):
        raw[t] = [_lm(370, 300, rng.normal(0, 0.5, (5, 2)))]                         # 70 px: inside
    near = FT.smooth_tracked_faces(raw, lifetimes=5)
    assert list(near) == [0] and _live(near[0]) == list(range(10))


def test_two_starts_on_one_frame_competing_for_one_chain():
    """One chain ends on frame 2 at x = 300.  On frame 4 two faces start, 40 px (raw track 1) and 20 px (raw track 2) from it.  Raw tracks
    are taken in order of start, ties by track id: track 1 comes first, finds one candidate and joins it; the chain then ends behind frame
    4, so track 2 has no candidate and starts a chain -- whatever its distance.  No chain holds two detections on one frame."""
    raw = [[_lm(300, 300)], [_lm(300, 300)], [_lm(300, 300)], [], [_lm(340, 300), _lm(280, 300)], [_lm(340, 300), _lm(280, 300)]]
    tracks = FT.track_faces(raw)
    assert sorted(tracks) == [0, 1, 2]
    assert FT.stitch_tracks(tracks, 3) == [[0, 1], [2]]
    on = FT.smooth_tracked_faces(raw, lifetimes=3)
    assert list(on) == [0, 1] and _live(on[0]) == [0, 1, 2, 3, 4, 5] and _live(on[1]) == [4, 5]
    # two chains compete for one start: the nearest wins, ties by the lowest chain id
    raw = [[_lm(300, 300), _lm(360, 300)], [], [_lm(340, 300)]]                      # 40 px from chain 0, 20 px from chain 1
    assert FT.stitch_tracks(FT.track_faces(raw), 1) == [[0], [1, 2]]
    raw = [[_lm(300, 300), _lm(360, 300)], [], [_lm(330, 300)]]                      # 30 px from both
    assert FT.stitch_tracks(FT.track_faces(raw), 1) == [[0, 2], [1]]


def test_only_center_face_with_interior_and_edge_gaps():
    n = 24
    seen = {2, 3, 4, 6, 7, 12, 13, 14, 20}                                           # gaps: 2 (edge), 1, 4, 5, 3 (edge)
    raw = _one_face(n, seen, np.random.default_rng(7))
    assert not np.isnan(FT.smooth_center_face(raw)[0]).any()                         # today
    report = []
    on = FT.smooth_center_face(raw, lifetimes=4, report=report)
    assert list(on) == [0, 1] and report == [(0, 2, 14, 8), (1, 20, 20, 1)]
    assert _live(on[0]) == list(range(2, 15)) and _live(on[1]) == [20]
    seq = np.full((13, 10), np.nan)
    for t in range(2, 15):
        if raw[t]:
            seq[t - 2] = raw[t][0].reshape(10)
    assert _same(on[0][2:15], FT._smooth(seq))
    three = FT.smooth_center_face(raw, lifetimes=3)
    assert [_live(three[k]) for k in three] == [list(range(2, 8)), [12, 13, 14], [20]]
    assert [_live(s) for s in FT.smooth_center_face(raw, lifetimes=0).values()] == [[2, 3, 4], [6, 7], [12, 13, 14], [20]]
    assert FT.smooth_center_face([[], [], []], lifetimes=4) == {}


@pytest.mark.parametrize('center', [False, True])
def test_no_lifetime_crosses_a_cut(center):
    n, cuts = 16, [6, 11]
    drop = {(5, 0), (6, 0), (3, 1), (12, 0), (12, 1), (13, 0), (13, 1), (14, 0), (14, 1), (15, 0), (15, 1)}
    raw = _two_faces(n, np.random.default_rng(8), drop)
    smooth = FT.smooth_center_face if center else FT.smooth_tracked_faces
    r = [f[:1] for f in raw] if center else raw
    report = []
    on = smooth(r, cuts, lifetimes=3, report=report)
    assert len(set(on)) == len(on) and [k for k, *_ in report] == list(on)
    segs = SC.segments(n, cuts)
    for (s, key), first, last, count in report:
        a, b = segs[s]
        assert a <= first <= last < b and count >= 1
        assert _live(on[(s, key)]) == list(range(first, last + 1))
    # every scene is the scene alone
    for s, (a, b) in enumerate(segs):
        alone = smooth(r[a:b], lifetimes=3)
        assert [k for (ss, k) in on if ss == s] == list(alone)
        for k, seq in alone.items():
            assert _same(on[(s, k)][a:b], seq)
    again = smooth(r, cuts, lifetimes=3)
    assert list(again) == list(on) and all(_same(again[k], on[k]) for k in on)
    if not center:
        # face 0 is undetected on frames 5 and 6 around the cut at 6: scene 0 ends its lifetime at 4, scene 1 opens it at 7
        by_key = {k: (a, b) for k, a, b, _ in report}
        assert by_key[(0, 0)] == (0, 4) and by_key[(0, 1)] == (0, 5) and by_key[(1, 0)] == (6, 10) and by_key[(1, 1)] == (7, 10)
        assert by_key[(2, 0)] == by_key[(2, 1)] == (11, 11)


def test_every_track_on_every_frame_is_the_knob_off_result():
    n = 11
    raw = _two_faces(n, np.random.default_rng(9))
    for cuts in (None, [4]):
        for smooth, r in ((FT.smooth_tracked_faces, raw), (FT.smooth_center_face, [f[:1] for f in raw])):
            off = smooth(r, cuts)
            for gap in (0, 1, 10):
                on = smooth(r, cuts, lifetimes=gap)
                assert list(on) == list(off) and len(on) == len(off)
                assert all(np.array_equal(on[k], off[k], equal_nan=cuts is not None) for k in off)   # (a scene's tracks are NaN outside it)
    # and the keyword's default is today's call
    assert all(np.array_equal(FT.smooth_tracked_faces(raw, None, None)[k], v) for k, v in FT.smooth_tracked_faces(raw).items())


# ---- the fade weights --------------------------------------------------------------------------------------------------------------------
def test_fade_weights():
    n = 20
    life = [('a', 5, 14, 10)]
    for R in (0,):
        w = FT.fade_weights(n, life, R)['a']
        assert w.dtype == np.float32 and w.shape == (n,) and (w[5:15] == 1.0).all() and not w[:5].any() and not w[15:].any()
    w = FT.fade_weights(n, life, 1)['a']
    assert w[5:15].tolist() == [0.5] + [1.0] * 8 + [0.5]
    w = FT.fade_weights(n, life, 3)['a']
    assert w[5:15].tolist() == [0.25, 0.5, 0.75, 1.0, 1.0, 1.0, 1.0, 0.75, 0.5, 0.25]
    w = FT.fade_weights(n, life, 2)['a']
    third = [np.float32(1 / 3), np.float32(2 / 3)]                                   # float64 quotient, then cast
    assert w[5:7].tolist() == [float(v) for v in third] and w[13:15].tolist() == [float(v) for v in third[::-1]] and (w[7:13] == 1).all()
    # a lifetime shorter than 2 R: the two ramps meet below 1
    w = FT.fade_weights(n, [('s', 8, 10, 3)], 3)['s']
    assert w[8:11].tolist() == [0.25, 0.5, 0.25] and not w[:8].any() and not w[11:].any()
    w = FT.fade_weights(n, [('one', 8, 8, 1)], 3)['one']
    assert w[8] == 0.25
    # ends that are ends of the video: no ramp there
    w = FT.fade_weights(n, [('head', 0, 5, 6), ('tail', 16, 19, 4), ('all', 0, 19, 20)], 1)
    assert w['head'][:6].tolist() == [1, 1, 1, 1, 1, 0.5] and w['tail'][16:].tolist() == [0.5, 1, 1, 1] and (w['all'] == 1).all()
    # ... or of a scene
    w = FT.fade_weights(n, [((0, 0), 3, 9, 7), ((1, 0), 10, 12, 3)], 1, cuts=[10])
    assert w[(0, 0)][3:10].tolist() == [0.5, 1, 1, 1, 1, 1, 1] and w[(1, 0)][10:13].tolist() == [1, 1, 0.5]
    same = FT.fade_weights(n, [((0, 0), 3, 9, 7)], 1)
    assert same[(0, 0)][9] == 0.5


# ---- the processor over fake nets ---------------------------------------------------------------------------------------------------------
def test_processor_knobs_and_the_crop_count(monkeypatch):
    from test_clip_plan_host import _MarkNet, _TrackHelper, _frames, _processor
    for k in ('KEEP_AMD_TRACK_LIFETIMES', 'KEEP_AMD_TRACK_MAX_GAP', 'KEEP_AMD_TRACK_FADE', 'KEEP_AMD_TRACK_CLIPS', 'KEEP_AMD_TRACK_CARRY',
              'KEEP_AMD_SCENE_CUTS'):
        monkeypatch.delenv(k, raising=False)

    class Missing(_TrackHelper):
        """track 0 on frames 0-4 and 6-9 only, track 1 (if any) on every frame"""
        def get_face_landmarks_5(self, only_center_face=False, resize=640, eye_dist_threshold=None):
            n = super().get_face_landmarks_5(only_center_face, resize, eye_dist_threshold)
            t = int(self.input_img[0, 0, 0])
            if t == 5 or t > 9:
                self.all_landmarks_5 = self.all_landmarks_5[1:]
            return len(self.all_landmarks_5)

    def proc_of(net, K):
        p = _processor(net, K, False)
        p.face_helper = Missing(K)
        return p
    frames = _frames(14)
    net = _MarkNet(True)
    off = proc_of(net, 1)
    assert off.track_lifetimes is False and off.track_max_gap == 10 and off.track_fade == 0 and off._per_track is False
    off.process_frames_u8(frames, 1.0, False, False, False, max_clip_length=4)
    assert sum(net.calls) == 28 and not hasattr(off, 'last_track_lifetimes')           # today: two tracks on all 14 frames
    monkeypatch.setenv('KEEP_AMD_TRACK_LIFETIMES', '1')
    monkeypatch.setenv('KEEP_AMD_TRACK_MAX_GAP', '3')
    monkeypatch.setenv('KEEP_AMD_TRACK_FADE', '2')
    net = _MarkNet(True)
    on = proc_of(net, 1)
    assert on.track_lifetimes is True and on.track_max_gap == 3 and on.track_fade == 2 and on._per_track is True and on.track_clips is False
    on.track_fade = 0
    out = on.process_frames_u8(frames, 1.0, False, False, False, max_clip_length=4)
    assert on.last_track_lifetimes == [(0, 0, 9, 9)] and sum(net.calls) == 10
    assert [[t for _, t in c] for c in net.clips] == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9]]
    assert all(np.array_equal(out[t], frames[t]) for t in range(10, 14))               # no live track: the frame as it came
    assert all(np.asarray(out[t]).shape == (1, 6) for t in range(10))
    # two faces: track 1 stays, track 0 has its lifetime; with scene cuts the keys carry the scene
    net = _MarkNet(True)
    two = proc_of(net, 2)
    two.process_frames_u8(frames, 1.0, False, False, False, max_clip_length=4)
    assert sorted(two.last_track_lifetimes) == [(0, 0, 9, 9), (1, 0, 13, 14)] and sum(net.calls) == 24
    # the helper's own paste takes no weight: a fade is ignored with ONE warning
    records = []

    class Catch(logging.Handler):
        def emit(self, record):
            records.append(record.getMessage())
    handler = Catch()
    logging.getLogger('ComfyUI-KEEP').addHandler(handler)
    try:
        on.track_fade = 2
        for _ in range(2):
            faded = on.process_frames_u8(frames[1:], 1.0, False, False, False, max_clip_length=4)   # (the lifetime ends inside the video)
            assert len(faded) == 13
    finally:
        logging.getLogger('ComfyUI-KEEP').removeHandler(handler)
    assert sum('KEEP_AMD_TRACK_FADE' in m for m in records) == 1
    # bad numbers fall back to the defaults; an aligned sequence ignores the knob
    monkeypatch.setenv('KEEP_AMD_TRACK_MAX_GAP', 'many')
    monkeypatch.setenv('KEEP_AMD_TRACK_FADE', '-3')
    p = proc_of(_MarkNet(True), 1)
    assert p.track_max_gap == 10 and p.track_fade == 0


# ---- the entry point ----------------------------------------------------------------------------------------------------------------------
def raw_lib():
    from comfyui_keep_amd.engine import hiplib
    lib = ctypes.CDLL(hiplib.LIB_PATH)
    lib.keep_last_error.restype = ctypes.c_char_p
    return lib


def test_symbol_is_in_the_extension_header_the_binding_and_the_library_only():
    from comfyui_keep_amd.engine import hiplib
    header = open(os.path.join(ROOT, 'include', 'keep_cv_hip.h')).read()
    core = open(os.path.join(ROOT, 'include', 'keep_hip.h')).read()
    assert re.search(r'int32_t ' + NAME + r'\s*\(', header) and NAME not in core
    assert NAME in hiplib.CV_EXPORTED_SYMBOLS and NAME in hiplib._CV_SIGNATURES
    assert NAME not in hiplib.EXPORTED_SYMBOLS and NAME not in hiplib._SIGNATURES
    assert hasattr(raw_lib(), NAME)
    proto = re.search(r'int32_t ' + NAME + r'\s*\(([^;]*)\);', header).group(1)
    assert len(re.sub(r'/\*.*?\*/', '', proto).split(',')) == len(hiplib._CV_SIGNATURES[NAME]) == 15
    # the core entry's argument list with the opacity in front of the stream
    core_sig = hiplib._SIGNATURES['keep_paste_face']
    assert hiplib._CV_SIGNATURES[NAME] == core_sig[:-1] + [ctypes.c_float] + core_sig[-1:]
    bound = hiplib.load(check_device=False)
    assert getattr(bound, NAME).argtypes == hiplib._CV_SIGNATURES[NAME] and getattr(bound, NAME).restype is ctypes.c_int32
    src = open(os.path.join(ROOT, 'comfyui-keep_amd', 'csrc', 'keep_paste.hip')).read()
    assert src.count('paste_face_kernel') == 2                                       # one kernel: its definition and ONE launch


def test_launcher_refusals_are_host_checks_that_name_the_function():
    """A bad opacity -- and every bad argument of the core entry -- is refused with KEEP_EINVAL before anything is launched, on a machine
    without a GPU: the device pointers (placeholders here) are never dereferenced."""
    lib = raw_lib()
    f = getattr(lib, NAME)
    f.restype = ctypes.c_int32
    f.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
                  ctypes.c_void_p] + [ctypes.c_int32] * 5 + [ctypes.c_float, ctypes.c_void_p]
    d2s = (ctypes.c_double * 6)(1, 0, 0, 0, 1, 0)

    def call(frame=0x1000, H=200, W=300, face=0x2000, mask=0x3000, fh=512, fw=512, m=d2s, box=(10, 10, 100, 100), border=10, opacity=0.5):
        return f(frame, H, W, face, mask, fh, fw, m, *box, border, opacity, None)
    refused = [dict(opacity=-0.25), dict(opacity=1.5), dict(opacity=float('nan')), dict(opacity=float('inf')), dict(opacity=-float('inf')),
               dict(opacity=1.0000001), dict(opacity=-1e-30), dict(frame=None), dict(face=None), dict(mask=None), dict(m=None), dict(H=0),
               dict(fw=1), dict(box=(-1, 10, 100, 100)), dict(box=(10, 10, 301, 100)), dict(box=(10, 10, 100, 201))]
    for kw in refused:
        assert call(**kw) == -1, kw
        assert lib.keep_last_error().startswith(NAME.encode() + b':'), (kw, lib.keep_last_error())
    assert call(box=(50, 50, 50, 90)) == 0 and call(box=(50, 50, 40, 90), opacity=0.0) == 0   # an empty box launches nothing
    assert call(box=(50, 50, 50, 90), opacity=2.0) == -1                                      # ... but is judged first


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def case():
    return FR.small_case()


def test_restatement_with_all_weights_one_is_the_oracle(case):
    frame, faces, mats, classes = case
    for cls in (list(classes), None):
        ref = P.paste_faces(frame, list(faces), list(mats), cls)
        assert (ref != frame).any()
        for weights in (None, [1.0, 1.0]):
            got = FR.paste_faces_weighted(frame, list(faces), list(mats), cls, weights=weights)
            assert got.dtype == np.uint8 and np.array_equal(got, ref)
    # the second face is cut by the frame's edge
    only2 = P.paste_faces(frame, [faces[1]], [mats[1]], [classes[1]])
    assert (only2[:, -1] != frame[:, -1]).any() and (only2[-1] != frame[-1]).any()


def test_restatement_with_weight_zero_returns_the_background(case):
    frame, faces, mats, classes = case
    for cls in (list(classes), None):
        assert np.array_equal(FR.paste_faces_weighted(frame, list(faces), list(mats), cls, weights=[0.0, 0.0]), frame)
        assert np.array_equal(FR.composite_f32(frame, list(faces), list(mats), cls, weights=[0.0, 0.0]), frame.astype(np.float32))
        one = FR.paste_faces_weighted(frame, list(faces), list(mats), cls, weights=[1.0, 0.0])
        assert np.array_equal(one, P.paste_faces(frame, [faces[0]], [mats[0]], None if cls is None else [classes[0]]))
        half = FR.paste_faces_weighted(frame, list(faces), list(mats), cls, weights=[0.5, 0.5])
        full = P.paste_faces(frame, list(faces), list(mats), cls)
        assert (half != full).any() and (half != frame).any()
