"""Scene cuts (KEEP_AMD_SCENE_CUTS), host side (no GPU): the signature's host restatement and the cut rule (modules/scene_cuts.py), cuts
in tracking and smoothing (modules/face_tracks.py), what the clip planner makes of tracks that end at a cut, and the new entry point
keep_frame_signature_u8: header, binding, library and the launcher's refusals, which are host checks."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

from comfyui_keep_amd.modules import face_tracks as FT
from comfyui_keep_amd.modules import scene_cuts as SC
from comfyui_keep_amd.modules.clip_plan import plan_track_chains

NAME = 'keep_frame_signature_u8'


def signature_by_loops(frame):
    """The definition, pixel by pixel in Python integers."""
    h, w = frame.shape[:2]
    sig = [0] * 256
    for y in range(h):
        for x in range(w):
            b, g, r = (int(v) for v in frame[y, x])
            lum = (29 * b + 150 * g + 77 * r + 128) >> 8
            sig[(((y * 4) // h) * 4 + (x * 4) // w) * 16 + (lum >> 4)] += 1
    return np.array(sig, np.int32)


# ---- the signature ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hw', [(37, 53), (3, 5), (1, 1), (4, 4), (8, 9)])
def test_signature_is_the_definition_and_sums_to_the_pixel_count(hw):
    h, w = hw
    frame = np.random.default_rng(h * 100 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    sig = SC.frame_signature_host(frame)
    assert sig.dtype == np.int32 and sig.shape == (256,) and int(sig.sum()) == h * w
    assert np.array_equal(sig, signature_by_loops(frame))


def test_cell_boundaries_at_sizes_not_divisible_by_four():
    # 37 x 53: cell rows start at ceil(c * 37 / 4) = 0, 10, 19, 28; columns at ceil(c * 53 / 4) = 0, 14, 27, 40
    sig = SC.frame_signature_host(np.zeros((37, 53, 3), np.uint8)).reshape(16, 16)
    rows, cols = [10, 9, 9, 9], [14, 13, 13, 13]
    assert [[int(sig[cy * 4 + cx, 0]) for cx in range(4)] for cy in range(4)] == [[r * c for c in cols] for r in rows]
    # 3 x 5: (y * 4) // 3 = 0, 1, 2 -- cell row 3 is empty; (x * 4) // 5 = 0, 0, 1, 2, 3
    sig = SC.frame_signature_host(np.zeros((3, 5, 3), np.uint8)).reshape(4, 4, 16)[:, :, 0]
    assert sig.tolist() == [[2, 1, 1, 1], [2, 1, 1, 1], [2, 1, 1, 1], [0, 0, 0, 0]]
    # 1 x 1: the one pixel is cell 0
    sig = SC.frame_signature_host(np.full((1, 1, 3), 255, np.uint8))
    assert int(sig[15]) == 1 and int(sig.sum()) == 1


def test_flat_frames_and_the_bin_boundary():
    for value, b in ((0, 0), (255, 15)):
        sig = SC.frame_signature_host(np.full((16, 24, 3), value, np.uint8)).reshape(16, 16)
        assert (sig[:, b] == 16 * 24 // 16).all() and int(sig.sum()) == 16 * 24 and int(sig[:, b].sum()) == 16 * 24
    # grey g has luma (256 g + 128) >> 8 = g: 15 and 16 are the two sides of the first bin boundary
    s15 = SC.frame_signature_host(np.full((8, 8, 3), 15, np.uint8)).reshape(16, 16)
    s16 = SC.frame_signature_host(np.full((8, 8, 3), 16, np.uint8)).reshape(16, 16)
    assert (s15[:, 0] == 4).all() and (s16[:, 1] == 4).all() and not s15[:, 1].any() and not s16[:, 0].any()
    # the weights: pure blue / green / red 255 -> luma (29 | 150 | 77) * 255 + 128 >> 8 = 29, 149, 77 -> bins 1, 9, 4
    for ch, b in ((0, 1), (1, 9), (2, 4)):
        f = np.zeros((4, 4, 3), np.uint8)
        f[..., ch] = 255
        assert (SC.frame_signature_host(f).reshape(16, 16)[:, b] == 1).all()
    with pytest.raises(ValueError):
        SC.frame_signature_host(np.zeros((4, 4, 3), np.float32))
    with pytest.raises(ValueError):
        SC.frame_signature_host(np.zeros((4, 4), np.uint8))


# ---- the cut rule -------------------------------------------------------------------------------------------------------------------
def test_find_cuts_threshold_is_inclusive_and_the_ends_work():
    hw = 100
    a = np.zeros(256, np.int32); a[0] = 100
    b = np.zeros(256, np.int32); b[0] = 60; b[1] = 40                        # distance to a: (40 + 40) / 200 = 0.4
    assert SC.signature_distance(a, b, hw) == 0.4 and SC.signature_distance(a, a, hw) == 0.0
    c = np.zeros(256, np.int32); c[17] = 100
    assert SC.signature_distance(a, c, hw) == 1.0
    assert SC.find_cuts([a, b], hw, 0.4) == [1]                               # inclusive
    assert SC.find_cuts([a, b], hw, 0.4000001) == []
    assert SC.find_cuts([a, c, c, c], hw, 0.4) == [1]                         # a cut at t = 1
    assert SC.find_cuts([a, a, a, c], hw, 0.4) == [3]                         # ... and at t = n - 1
    assert SC.find_cuts([a, c, a, c], hw, 0.4) == [1, 2, 3]
    assert SC.find_cuts([a], hw, 0.4) == [] and SC.find_cuts([a, c], hw, 1.5) == []
    assert SC.segments(8, [5]) == [(0, 5), (5, 8)] and SC.segments(8, []) == [(0, 8)] and SC.segments(8, None) == [(0, 8)]
    assert SC.segments(4, [1, 3]) == [(0, 1), (1, 3), (3, 4)] and SC.segments(4, [3, 1, 3, 0, 4, 9]) == [(0, 1), (1, 3), (3, 4)]
    assert SC.segments(0, [1]) == []
    d = SC.signature_distances([a, b, c], hw)
    assert d.shape == (2,) and d[0] == 0.4 and d[1] == 1.0


def test_two_noise_scenes_boundary_is_exactly_one_and_inside_is_small():
    """Scene A = integers(0, 128), B = integers(128, 256) at 512 x 512: the lumas of A stay below 128 and those of B at or above it, so
    no counter is shared; inside a scene the histograms of independent noise frames differ by sampling noise only."""
    rng = np.random.default_rng(3)
    A = rng.integers(0, 128, (5, 512, 512, 3), dtype=np.uint8)
    B = rng.integers(128, 256, (3, 512, 512, 3), dtype=np.uint8)
    full = rng.integers(0, 256, (2, 512, 512, 3), dtype=np.uint8)
    sigs = [SC.frame_signature_host(f) for f in np.concatenate([A, B])]
    d = SC.signature_distances(sigs, 512 * 512)
    print('distances', [round(float(v), 4) for v in d])
    assert d[4] == 1.0
    assert all(d[t] < 0.02 for t in range(7) if t != 4)
    assert SC.signature_distance(SC.frame_signature_host(full[0]), SC.frame_signature_host(full[1]), 512 * 512) < 0.02
    assert SC.find_cuts(sigs, 512 * 512, 0.4) == [5]


# ---- cuts in tracking and smoothing ---------------------------------------------------------------------------------------------------
def _lm(cx, cy, jitter=0.0):
    base = np.array([[-30.0, -20.0], [30.0, -20.0], [0.0, 10.0], [-25.0, 40.0], [25.0, 40.0]])
    return base + np.array([cx, cy]) + jitter


def _raw_two_faces(n, rng, drop=()):
    raw = []
    for t in range(n):
        faces = [_lm(200 + 2.0 * t, 300, rng.normal(0, 1.5, (5, 2))), _lm(600 - 1.5 * t, 320, rng.normal(0, 1.5, (5, 2)))]
        raw.append([f for j, f in enumerate(faces) if (t, j) not in drop])
    return raw


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize('cuts', [[5], [1], [11], [3, 4, 9]])
def test_smoothing_with_cuts_equals_the_per_segment_calls_rekeyed(cuts):
    n = 12
    raw = _raw_two_faces(n, np.random.default_rng(8), drop={(2, 1), (7, 0), (8, 0)})
    for smooth, center in ((FT.smooth_tracked_faces, False), (FT.smooth_center_face, True)):
        r = [f[:1] for f in raw] if center else raw
        got = smooth(r, cuts)
        want = {}
        for s, (a, b) in enumerate(SC.segments(n, cuts)):
            for key, seq in smooth(r[a:b]).items():
                full = np.full((n, 5, 2), np.nan)
                full[a:b] = seq
                want[(s, key)] = full
        assert list(got) == list(want) and len(set(got)) == len(got)
        for k in want:
            assert _same(got[k], want[k]), k
        # a track is NaN outside its scene and whole inside it
        for (s, _), seq in got.items():
            a, b = SC.segments(n, cuts)[s]
            assert np.isnan(seq[:a]).all() and np.isnan(seq[b:]).all() and not np.isnan(seq[a:b]).any()


def test_no_cuts_is_todays_output():
    raw = _raw_two_faces(9, np.random.default_rng(9), drop={(4, 1)})
    for smooth, r in ((FT.smooth_tracked_faces, raw), (FT.smooth_center_face, [f[:1] for f in raw])):
        base = smooth(r)
        for cuts in (None, []):
            got = smooth(r, cuts)
            assert list(got) == list(base) and all(_same(got[k], base[k]) for k in base)
        assert all(isinstance(k, int) for k in base)
    # ... and a cut changes the landmarks near it: the whole-video filter blends the two sides
    base, cut = FT.smooth_center_face([f[:1] for f in raw]), FT.smooth_center_face([f[:1] for f in raw], [4])
    assert not np.array_equal(base[0][3], cut[(0, 0)][3]) and not np.array_equal(base[0][4], cut[(1, 0)][4])


def test_a_segment_without_detections_yields_no_track():
    rng = np.random.default_rng(10)
    raw = [[] for _ in range(4)] + [[_lm(300 + t, 300, rng.normal(0, 1, (5, 2)))] for t in range(5)] + [[] for _ in range(3)]
    # today: the face of frames 4 .. 8 is extrapolated over the whole video (np.interp clamps)
    today = FT.smooth_center_face(raw)
    assert not np.isnan(today[0]).any()
    for smooth in (FT.smooth_center_face, FT.smooth_tracked_faces):
        got = smooth(raw, [4, 9])
        assert list(got) == [(1, 0)]
        assert np.isnan(got[(1, 0)][:4]).all() and np.isnan(got[(1, 0)][9:]).all() and not np.isnan(got[(1, 0)][4:9]).any()
        assert _same(got[(1, 0)][4:9], smooth(raw[4:9])[0])
        assert smooth([[], [], []], [1]) == {}
    # only_center_face with a face in scene 2 only: scene 1 stays NaN, i.e. is not restored
    got = FT.smooth_center_face(raw[:9], [4])
    assert list(got) == [(1, 0)] and np.isnan(got[(1, 0)][:4]).all()


def test_framed_alike_across_a_cut_is_two_tracks():
    """Two people at the same place on either side of the cut: one track today, two with the cut."""
    rng = np.random.default_rng(11)
    raw = [[_lm(400, 300, rng.normal(0, 1, (5, 2)))] for _ in range(8)]
    assert list(FT.smooth_tracked_faces(raw)) == [0]
    assert list(FT.smooth_tracked_faces(raw, [5])) == [(0, 0), (1, 0)]


# ---- the planner over cut tracks ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('L', [1, 2, 4, 20])
@pytest.mark.parametrize('center', [False, True])
def test_no_clip_spans_a_cut_and_nothing_is_carried_across_it(L, center):
    n, cuts = 12, [5, 9]
    raw = _raw_two_faces(n, np.random.default_rng(12), drop={(6, 1)})
    tracks = FT.smooth_center_face([f[:1] for f in raw], cuts) if center else FT.smooth_tracked_faces(raw, cuts)
    presence = [[k for k, seq in tracks.items() if not np.isnan(seq[t]).any()] for t in range(n)]
    clips, slot_of, after = plan_track_chains(presence, L)
    frame_of = [t for t in range(n) for _ in presence[t]]
    scene_of = {t: s for s, (a, b) in enumerate(SC.segments(n, cuts)) for t in range(a, b)}
    starts = {a for a, _ in SC.segments(n, cuts)}
    assert sorted(i for m in clips for i in m) == list(range(len(frame_of)))
    for c, m in enumerate(clips):
        frames = [frame_of[i] for i in m]
        assert len({scene_of[t] for t in frames}) == 1 and len(m) <= L, (c, frames)
        assert frames == list(range(frames[0], frames[0] + len(m)))
        if frames[0] in starts:
            assert after[c] is None, (c, frames)                                     # the first clip after a cut starts from nothing
        if after[c] is not None:
            prev = [frame_of[i] for i in clips[after[c]]]
            assert prev[-1] + 1 == frames[0] and scene_of[prev[-1]] == scene_of[frames[0]]
    # every scene's plan is the plan of that scene alone
    if L == 4 and not center:
        a, b = 0, 5
        alone = FT.smooth_tracked_faces(raw[a:b])
        p_alone = [[k for k, seq in alone.items() if not np.isnan(seq[t]).any()] for t in range(b - a)]
        c_alone, _, a_alone = plan_track_chains(p_alone, L)
        assert clips[:len(c_alone)] == c_alone and after[:len(c_alone)] == a_alone


# ---- the processor's host logic over fake nets ------------------------------------------------------------------------------------------
def test_processor_knob_guards_and_the_host_signature_path(monkeypatch):
    """Per-frame path with a fake net (no GPU): the knob finds the cut with the host function, hands per-scene keys to the planner, implies
    track clips, ignores frames it cannot read with ONE warning and leaves a processor without the knob untouched."""
    import logging
    from test_clip_plan_host import _MarkNet, _frames, _processor
    for k in ('KEEP_AMD_SCENE_CUTS', 'KEEP_AMD_SCENE_CUT_THRESHOLD', 'KEEP_AMD_TRACK_CLIPS', 'KEEP_AMD_TRACK_CARRY'):
        monkeypatch.delenv(k, raising=False)
    net = _MarkNet(True)
    proc = _processor(net, 2, False)
    assert proc.scene_cuts is False and proc.scene_cut_threshold == 0.4 and proc._per_track is False
    assert not hasattr(proc, 'last_scene_cuts')
    frames = _frames(6)
    dark = [np.full_like(f, 10) for f in frames[:4]]
    bright = [np.full_like(f, 240) for f in frames[4:]]
    video = dark + bright
    proc.process_frames_u8(video, 1.0, False, False, False, max_clip_length=3)
    assert not hasattr(proc, 'last_scene_cuts')                                      # knob off: nothing is computed or written
    assert [len(c) for c in net.clips] == [3, 3, 3, 3]                                # the flat cut: clip 1 spans the scene boundary
    monkeypatch.setenv('KEEP_AMD_SCENE_CUTS', '1')
    monkeypatch.setenv('KEEP_AMD_SCENE_CUT_THRESHOLD', '0.25')
    net_on = _MarkNet(True)
    on = _processor(net_on, 2, False)
    assert on.scene_cuts is True and on.scene_cut_threshold == 0.25 and on._per_track is True
    on.scene_cut_threshold = 0.4
    on.process_frames_u8(video, 1.0, False, False, False, max_clip_length=3)
    assert on.last_scene_cuts == [4] and on.last_scene_distances.shape == (5,) and on.last_scene_distances[3] == 1.0
    assert sorted(len(c) for c in net_on.clips) == [1, 1, 2, 2, 3, 3]                # per track: scene 1 = [3, 1], scene 2 = [2]
    on.scene_cut_threshold = 1.5
    on.process_frames_u8(video, 1.0, False, False, False, max_clip_length=3)
    assert on.last_scene_cuts == []
    # a single frame has nothing to cut; mixed sizes ignore the knob with one warning
    on.scene_cut_threshold = 0.4
    on.process_frames_u8(video[:1], 1.0, False, False, False, max_clip_length=3)
    assert on.last_scene_cuts == [] and on.last_scene_distances.shape == (0,)
    records = []

    class Catch(logging.Handler):
        def emit(self, record):
            records.append(record.getMessage())
    handler = Catch()
    logging.getLogger('ComfyUI-KEEP').addHandler(handler)
    try:
        odd = [video[0], video[1][:-2], video[5]]
        for _ in range(2):
            on.last_scene_cuts = on.last_scene_distances = 'stale'
            out = on.process_frames_u8(odd, 1.0, False, False, False, max_clip_length=3)   # runs as track clips: the knob implies them
            assert len(out) == 3 and on.last_scene_cuts == [] and on.last_scene_distances.shape == (0,)
        on.last_scene_cuts = 'stale'
        assert on._scene_cuts_apply(odd) is False and on.last_scene_cuts == []
        assert on._scene_cuts_apply([f.astype(np.float32) for f in video]) is False
        assert on._scene_cuts_apply(video) is True
    finally:
        logging.getLogger('ComfyUI-KEEP').removeHandler(handler)
    assert sum('KEEP_AMD_SCENE_CUTS' in m for m in records) == 1


# ---- the entry point ------------------------------------------------------------------------------------------------------------------
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
    assert NAME not in hiplib.EXPORTED_SYMBOLS and NAME not in hiplib._SIGNATURES and len(hiplib.EXPORTED_SYMBOLS) == 63
    assert hasattr(raw_lib(), NAME)
    proto = re.search(r'int32_t ' + NAME + r'\s*\(([^;]*)\);', header).group(1)
    assert len(re.sub(r'/\*.*?\*/', '', proto).split(',')) == len(hiplib._CV_SIGNATURES[NAME]) == 6
    assert int(re.search(r'#define KEEP_CV_ABI_VERSION (\d+)', header).group(1)) == hiplib.CV_ABI_VERSION == 1
    bound = hiplib.load(check_device=False)
    assert getattr(bound, NAME).argtypes == hiplib._CV_SIGNATURES[NAME] and getattr(bound, NAME).restype is ctypes.c_int32
    assert NAME in open(os.path.join(ROOT, 'comfyui-keep_amd', 'csrc', 'Makefile')).read().replace('keep_signature.hip', NAME)


def test_launcher_refusals_are_host_checks_that_name_the_function():
    """Every bad argument is refused with KEEP_EINVAL on a machine without a GPU: the checks run on the host before the first launch, and
    the device pointers (placeholders here) are never dereferenced."""
    lib = raw_lib()
    f = getattr(lib, NAME)
    f.restype = ctypes.c_int32
    f.argtypes = [ctypes.c_void_p] + [ctypes.c_int32] * 3 + [ctypes.c_void_p] * 2

    def call(frames=0x1000, N=3, H=37, W=53, sig=0x2000):
        return f(frames, N, H, W, sig, None)
    refused = [dict(frames=None), dict(sig=None), dict(frames=None, sig=None), dict(N=0), dict(N=-1), dict(H=0), dict(H=-4), dict(W=0),
               dict(W=-1), dict(H=32768), dict(W=32768), dict(H=40000), dict(W=2 ** 31 - 1), dict(H=32768, W=32768)]
    for kw in refused:
        assert call(**kw) == -1, kw
        assert lib.keep_last_error().startswith(NAME.encode() + b':'), (kw, lib.keep_last_error())
