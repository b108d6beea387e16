"""Track clips (KEEP_AMD_TRACK_CLIPS), host side (no GPU): the planner (modules/clip_plan.py) -- runs, pieces, clip order, slots and its
reduction to the cut of the flat list --, the processor's consumers over a fake net that marks every output with clip id and position
(a wrong scatter shows), and the scatter form of the batched crop warp (keep_warp_affine_batch_scatter_u8): header, binding, library
and the launcher's refusals, which are host checks."""
import ctypes
import os
import random
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_host_logic import _Helper, _pack, _U8Net

from comfyui_keep_amd.modules.keep_processor import KEEPFaceProcessor, split_clips

NAME = 'keep_warp_affine_batch_scatter_u8'


def plan(presence, L):
    from comfyui_keep_amd.modules.clip_plan import plan_track_clips
    return plan_track_clips(presence, L)


# ---- the planner ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('L', [1, 20])
@pytest.mark.parametrize('n', [1, 2, 19, 20, 21, 41])
def test_one_track_is_the_cut_of_the_flat_list(n, L):
    clips, slot_of = plan([['a']] * n, L)
    assert clips == [list(range(s, e)) for s, e in split_clips(n, L)]
    assert slot_of == list(range(n))


def test_three_tracks_seven_frames_clips_of_three():
    K, N, L = 3, 7, 3
    clips, slot_of = plan([['A', 'B', 'C']] * N, L)
    first = [K * t for t in range(N)]
    piece = lambda j, a, b: [first[t] + j for t in range(a, b)]                      # noqa: E731  members are first[t] + j
    assert clips == [piece(0, 0, 3), piece(1, 0, 3), piece(2, 0, 3), piece(0, 3, 6), piece(1, 3, 6), piece(2, 3, 6),
                     piece(0, 6, 7), piece(1, 6, 7), piece(2, 6, 7)]                  # A[0-2] B[0-2] C[0-2] A[3-5] ... A[6] B[6] C[6]
    for j in range(K):                                                               # every track: [0-2] [3-5] [6]
        mine = [[(i - j) // K for i in m] for m in clips if m[0] % K == j]
        assert mine == [[0, 1, 2], [3, 4, 5], [6]]
    assert sorted(slot_of) == list(range(K * N))
    assert [slot_of[i] for m in clips for i in m] == list(range(K * N))


def test_a_gap_starts_a_new_run():
    # B is absent on frame 2: crops A0 B0 | A1 B1 | A2 | A3 B3 | A4 B4 = indices 0 1 | 2 3 | 4 | 5 6 | 7 8
    clips, slot_of = plan([['A', 'B'], ['A', 'B'], ['A'], ['A', 'B'], ['A', 'B']], 20)
    assert clips == [[0, 2, 4, 5, 7], [1, 3], [6, 8]]
    assert slot_of == [0, 5, 1, 6, 2, 3, 7, 4, 8]
    # ... and with clips of 2 the second run sorts by ITS first frame (3), behind A's piece that starts at frame 2
    clips, _ = plan([['A', 'B'], ['A', 'B'], ['A'], ['A', 'B'], ['A', 'B']], 2)
    assert clips == [[0, 2], [1, 3], [4, 5], [6, 8], [7]]


def test_a_late_track_sorts_behind_the_clips_that_start_earlier():
    # C appears at frame 3 and takes face position 0 from there on (the face order of a frame is the caller's)
    presence = [['A', 'B']] * 3 + [['C', 'A', 'B']] * 3
    clips, slot_of = plan(presence, 4)
    # crops: frames 0-2 -> 0..5; frame 3: C 6, A 7, B 8; frame 4: 9 10 11; frame 5: 12 13 14
    assert clips == [[0, 2, 4, 7], [1, 3, 5, 8], [6, 9, 12], [10, 13], [11, 14]]
    #                 A[0-3]        B[0-3]        C[3-5]      A[4-5]    B[4-5]: C's first clip starts at 3 < 4, so it runs before them
    assert [slot_of[i] for m in clips for i in m] == list(range(15))
    # at an equal first frame the order is the order of first appearance, not the face order of the frame
    clips, _ = plan([['A', 'B']] * 2 + [['C', 'A', 'B']] * 2, 2)
    assert clips == [[0, 2], [1, 3], [5, 8], [6, 9], [4, 7]]


def test_planner_refuses_nonsense():
    with pytest.raises(ValueError):
        plan([['A']], 0)
    with pytest.raises(ValueError):
        plan([['A', 'A']], 3)
    assert plan([], 5) == ([], [])
    assert plan([[], [], []], 5) == ([], [])


def test_random_presence_tables():
    rng = random.Random(20240607)
    for _ in range(400):
        K, N, L = rng.randint(1, 4), rng.randint(1, 30), rng.randint(1, 7)
        p_on = rng.choice([0.3, 0.7, 0.95])
        presence = []
        for t in range(N):
            keys = [k for k in range(K) if rng.random() < p_on]
            rng.shuffle(keys)                              # (any face order)
            presence.append(keys)
        clips, slot_of = plan(presence, L)
        first, owner = [0], []
        for t, keys in enumerate(presence):
            first.append(first[-1] + len(keys))
            owner += [(k, t) for k in keys]
        n = first[-1]
        assert sorted(i for m in clips for i in m) == list(range(n))                 # every crop in exactly one clip
        assert sorted(slot_of) == list(range(n))                                     # a permutation
        slot = 0
        starts = []
        for m in clips:
            assert 1 <= len(m) <= L
            assert len({owner[i][0] for i in m}) == 1                                # one track
            ts = [owner[i][1] for i in m]
            assert ts == list(range(ts[0], ts[0] + len(m)))                          # consecutive frames
            assert [slot_of[i] for i in m] == list(range(slot, slot + len(m)))       # consecutive, increasing slots, in clip order
            slot += len(m)
            starts.append(ts[0])
        assert starts == sorted(starts)                                              # sorted by first frame
        # runs are maximal and pieces are full first: a clip shorter than L is followed by no clip of its track on the next frame
        ends = {(owner[m[-1]][0], owner[m[-1]][1]): len(m) for m in clips}
        begins = {(owner[m[0]][0], owner[m[0]][1]) for m in clips}
        for (k, t), length in ends.items():
            if length < L:
                assert (k, t + 1) not in begins


# ---- the processor's consumers ----------------------------------------------------------------------------------------------------
class _MarkNet(_U8Net):
    """``_U8Net`` whose output is the input with clip id, position and clip length written into pixel [1, 0] of every crop; records per
    clip the (track, frame) pairs the crops carry in pixel [0, 0]."""

    def __init__(self, single_frame=True):
        super().__init__(single_frame)
        self.clips = []

    def run_clips_u8(self, clips, max_b=4):
        clips = [torch.from_numpy(np.stack(c)) if isinstance(c, list) else c for c in clips]
        outs = []
        for cid, c in enumerate(clips):
            assert c.dtype == torch.uint8 and c.dim() == 4 and c.shape[1:] == (512, 512, 3)
            self.calls.append(c.shape[0])
            self.clips.append([(int(f[0, 0, 0]), int(f[0, 0, 1])) for f in c])
            o = c.clone()
            for k in range(c.shape[0]):
                o[k, 1, 0] = torch.tensor([cid, k, c.shape[0]], dtype=torch.uint8)
            outs.append(o)
        return outs


class _PoolNet(_MarkNet):
    """A net with a worker pool: the clip list it is given is dealt round-robin to two 'workers' and collected by clip index -- what
    engine/pool.py and engine/dist.py do with WHATEVER clip list arrives."""
    pool = object()

    def run_clips_u8(self, clips, max_b=4):
        outs = super().run_clips_u8(clips, max_b)
        self.shards = [list(range(r, len(clips), 2)) for r in range(2)]
        collected = {i: outs[i] for shard in self.shards for i in shard}
        return [collected[i] for i in range(len(clips))]


class _TrackHelper(_Helper):
    """K faces per frame at fixed places (track j: landmarks around x = 200 j); frames carry their index in pixel [0, 0, 0].  The crop of
    (track j, frame t) carries (j, t) in pixel [0, 0]; the 'pasted frame' is the list of marks of the restored faces it was given."""
    use_parse, is_gray, upscale_factor, face_size, pad_blur = True, False, 1, (512, 512), False

    def __init__(self, K):
        self.K = K
        self.clean_all()

    def clean_all(self):
        self.all_landmarks_5, self.affine_matrices, self.cropped_faces, self.restored_faces = [], [], [], []
        self.inverse_affine_matrices = []

    def read_image(self, img):
        self.input_img = img

    def get_face_landmarks_5(self, only_center_face=False, resize=640, eye_dist_threshold=None):
        n = 1 if only_center_face else self.K
        self.all_landmarks_5 = [np.full((5, 2), 200.0 * j) + np.arange(5)[:, None] for j in range(n)]
        return n

    def align_warp_face(self):
        t = int(self.input_img[0, 0, 0])
        for lm in self.all_landmarks_5:
            crop = np.zeros((512, 512, 3), np.uint8)
            crop[0, 0] = (int(round(lm[0, 0] / 200.0)), t, 0)
            self.cropped_faces.append(crop)
            self.affine_matrices.append(np.eye(2, 3))

    def get_inverse_affine(self, _):
        self.inverse_affine_matrices = list(self.affine_matrices)

    def paste_faces_to_input_image(self, upsample_img=None, draw_box=False, face_upsampler=None):
        t = int(self.input_img[0, 0, 0]) if upsample_img is None else int(upsample_img[0, 0, 0])
        return np.array([[t] + list(f[0, 0, :2]) + list(f[1, 0]) for f in self.restored_faces], np.int64)


def _frames(n):
    return [np.full((8, 8, 3), t, np.uint8) for t in range(n)]


def _processor(net, K, knob):
    proc = KEEPFaceProcessor(_pack(net))
    proc.face_helper = _TrackHelper(K)
    proc.gpu_paste = False                       # the helper's own warp and paste
    proc.track_clips = knob
    return proc


def test_knob_is_read_in_the_constructor_and_off_by_default(monkeypatch):
    monkeypatch.delenv('KEEP_AMD_TRACK_CLIPS', raising=False)
    assert KEEPFaceProcessor(_pack(_MarkNet())).track_clips is False
    monkeypatch.setenv('KEEP_AMD_TRACK_CLIPS', '1')
    assert KEEPFaceProcessor(_pack(_MarkNet())).track_clips is True
    monkeypatch.setenv('KEEP_AMD_TRACK_CLIPS', '0')
    assert KEEPFaceProcessor(_pack(_MarkNet())).track_clips is False


@pytest.mark.parametrize('single_frame', [True, False])
def test_sequence_knob_off_hands_over_todays_clips(single_frame, monkeypatch):
    """Knob off: the flat frame-major list cut into clips of L, and the planner is not even imported by the call."""
    from comfyui_keep_amd.modules import clip_plan
    monkeypatch.setattr(clip_plan, 'plan_track_clips', lambda *a, **k: pytest.fail('planned with the knob off'))
    K, N, L = 3, 7, 4
    net = _MarkNet(single_frame)
    proc = _processor(net, K, False)
    out = proc.process_frames_u8(_frames(N), 1.0, False, False, False, max_clip_length=L)
    flat = [(j, t) for t in range(N) for j in range(K)]
    spans = split_clips(K * N, L)                                                    # 21 = 5 x 4 + 1
    lone = [flat[s] for s, e in spans if e - s == 1]
    assert net.clips == [flat[s:e] * (2 if e - s == 1 and not single_frame else 1) for s, e in spans]
    assert lone == [(2, 6)] and net.calls == [4] * 5 + [1 if single_frame else 2]
    for t, fr in enumerate(out):
        for j, (ft, fj, ftt, cid, k, T) in enumerate(fr.tolist()):
            i = K * t + j
            assert (ft, fj, ftt) == (t, j, t) and (cid, k) == (i // L, i % L)


@pytest.mark.parametrize('single_frame', [True, False])
def test_sequence_knob_on_hands_over_per_track_clips_and_scatters_back(single_frame):
    K, N, L = 3, 7, 3
    net = _MarkNet(single_frame)
    proc = _processor(net, K, True)
    out = proc.process_frames_u8(_frames(N), 1.0, False, False, False, max_clip_length=L)
    dup = 1 if single_frame else 2
    expect = []
    for a, b in ((0, 3), (3, 6), (6, 7)):
        for j in range(K):
            expect.append([(j, t) for t in range(a, b)] * (dup if b - a == 1 else 1))
    assert net.clips == expect                                                       # A[0-2] B[0-2] C[0-2] A[3-5] ... one track per clip
    assert len(out) == N
    for t, fr in enumerate(out):                 # every pasted frame got the restored crop of its own frame and face
        assert fr.shape == (K, 6)
        for j, (ft, fj, ftt, cid, k, T) in enumerate(fr.tolist()):
            assert (ft, fj, ftt) == (t, j, t)
            assert (cid, k) == ((t // L) * K + j, t % L)                              # ... from the clip and the position the plan gave it
    faces = proc.last_restored_faces
    assert [tuple(f[0, 0, :2]) for f in faces] == [(j, t) for t in range(N) for j in range(K)]


def test_sequence_with_a_gap_and_a_frame_without_faces(monkeypatch):
    """Track 1 is blanked on frame 2, every track on frame 4 (the smoother would fill gaps: a wrapper blanks them, as
    tests/test_gpu_frame_store.py does): runs never bridge a gap, and the paste still gets every frame's own faces."""
    from comfyui_keep_amd.modules import keep_processor as KP
    real = KP.smooth_tracked_faces

    def blanked(raw):
        tracks = {k: np.array(v, np.float64, copy=True) for k, v in real(raw).items()}
        tracks[1][2] = np.nan
        for k in tracks:
            tracks[k][4] = np.nan
        return tracks
    monkeypatch.setattr(KP, 'smooth_tracked_faces', blanked)
    net = _MarkNet(True)
    proc = _processor(net, 2, True)
    out = proc.process_frames_u8(_frames(7), 1.0, False, False, False, max_clip_length=3)
    assert net.clips == [[(0, 0), (0, 1), (0, 2)], [(1, 0), (1, 1)], [(0, 3)], [(1, 3)], [(0, 5), (0, 6)], [(1, 5), (1, 6)]]
    assert [len(np.atleast_2d(f)) if np.asarray(f).ndim == 2 else 0 for f in out] == [2, 2, 1, 2, 0, 2, 2]
    assert np.array_equal(out[4], _frames(7)[4])                                     # no face: the frame as it came
    for t in (0, 1, 2, 3, 5, 6):
        for row in out[t].tolist():
            assert row[0] == t == row[2]
    assert [r[1] for r in out[2].tolist()] == [0] and [r[1] for r in out[3].tolist()] == [0, 1]


def test_single_face_video_gets_the_same_clips_knob_on_or_off():
    runs = {}
    for knob in (False, True):
        net = _MarkNet(True)
        out = _processor(net, 3, knob).process_frames_u8(_frames(9), 1.0, False, True, False, max_clip_length=4)
        runs[knob] = (net.clips, net.calls, [f.tolist() for f in out])
    assert runs[True] == runs[False] and runs[True][1] == [4, 4, 1]


def test_aligned_sequence_gets_the_same_clips_knob_on_or_off():
    runs = {}
    frames = [np.full((512, 512, 3), t, np.uint8) for t in range(5)]
    for knob in (False, True):
        net = _MarkNet(False)
        proc = _processor(net, 1, knob)
        proc.process_frames_u8(frames, 1.0, True, True, False, max_clip_length=2)
        runs[knob] = (net.calls, [np.asarray(f).tobytes() for f in proc.last_restored_faces])
    assert runs[True] == runs[False] and runs[True][0] == [2, 2, 2]


@pytest.mark.parametrize('single_frame', [True, False])
def test_single_image_with_three_faces(single_frame):
    """Knob off: one 'clip' of T = 3 (reference quirk P3); knob on: every face a clip of its own, restored like a lone face."""
    img = np.full((8, 8, 3), 5, np.uint8)
    net = _MarkNet(single_frame)
    off = _processor(net, 3, False).process_image(img, 1.0, False, False, False)
    assert net.calls == [3] and [r[3:] for r in off.tolist()] == [[0, 0, 3], [0, 1, 3], [0, 2, 3]]
    net = _MarkNet(single_frame)
    proc = _processor(net, 3, True)
    on = proc.process_image(img, 1.0, False, False, False)
    T = 1 if single_frame else 2
    assert net.calls == [T] * 3 and net.clips == [[(j, 5)] * T for j in range(3)]
    assert [r[1] for r in on.tolist()] == [0, 1, 2]                                  # face j is pasted as face j
    assert [r[3:] for r in on.tolist()] == [[j, 0, T] for j in range(3)]             # ... restored as frame 0 of clip j
    # one face: the lone-face rule, knob on or off
    net = _MarkNet(single_frame)
    _processor(net, 1, True).process_image(img, 1.0, False, False, False)
    assert net.calls == [T]


def test_reference_net_without_the_uint8_entry_takes_the_plan_too():
    """A net that is only callable (the reference's): ``_restore_crops_u8(members=...)`` goes through the float path, per-track clips,
    outputs back in crop order (output = input + the 1-based clip number, tests/test_host_logic.py's recording net)."""
    from test_host_logic import _RecordingNet
    net = _RecordingNet()
    proc = KEEPFaceProcessor(_pack(net))
    crops = [np.full((512, 512, 3), 10 * i, np.uint8) for i in range(5)]             # A0 B0 A1 B1 A2
    members = [[0, 2, 4], [1, 3]]
    faces = proc._restore_crops_u8(crops, 3, members=members)
    assert net.calls == [3, 2]
    clip_of = {0: 1, 2: 1, 4: 1, 1: 2, 3: 2}
    from comfyui_keep_amd.modules.utils import crops_to_net_input, net_output_to_bgr_u8
    for i, f in enumerate(faces):
        assert np.array_equal(f, net_output_to_bgr_u8(crops_to_net_input([crops[i]])[0] + float(clip_of[i])))
    net = _RecordingNet()
    KEEPFaceProcessor(_pack(net))._restore_crops_u8(crops[:2], 1, members=[[0], [1]])
    assert net.calls == [2, 2]                                                       # the reference net needs T >= 2


def test_a_net_with_a_pool_shards_whatever_clip_list_it_is_given():
    K, N, L = 2, 5, 2
    ref_net, net = _MarkNet(True), _PoolNet(True)
    ref = _processor(ref_net, K, True).process_frames_u8(_frames(N), 1.0, False, False, False, max_clip_length=L)
    got = _processor(net, K, True).process_frames_u8(_frames(N), 1.0, False, False, False, max_clip_length=L)
    assert net.clips == ref_net.clips and len(net.clips) == 6                        # A[0-1] B[0-1] A[2-3] B[2-3] A[4] B[4]
    assert net.shards == [[0, 2, 4], [1, 3, 5]]
    assert all(np.array_equal(a, b) for a, b in zip(got, ref))

    class NonRoot(_MarkNet):                     # a non-root rank of a torch.distributed run: the root pastes
        def run_clips_u8(self, clips, max_b=4):
            super().run_clips_u8(clips, max_b)
            return None
    assert _processor(NonRoot(True), K, True).process_frames_u8(_frames(N), 1.0, False, False, False, max_clip_length=L) is None
    assert _processor(NonRoot(True), 3, True).process_image(_frames(1)[0], 1.0, False, False, False) is None


# ---- the scatter entry -----------------------------------------------------------------------------------------------------------
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
    assert len(re.sub(r'/\*.*?\*/', '', proto).split(',')) == len(hiplib._CV_SIGNATURES[NAME]) == 16
    assert len(hiplib._CV_SIGNATURES['keep_warp_affine_batch_u8']) == 14             # the existing entry keeps its signature
    proto = re.search(r'int32_t keep_warp_affine_batch_u8\s*\(([^;]*)\);', header).group(1)
    assert len(re.sub(r'/\*.*?\*/', '', proto).split(',')) == 14
    assert int(re.search(r'#define KEEP_CV_ABI_VERSION (\d+)', header).group(1)) == hiplib.CV_ABI_VERSION == 1
    bound = hiplib.load(check_device=False)
    assert getattr(bound, NAME).argtypes == hiplib._CV_SIGNATURES[NAME] and getattr(bound, NAME).restype is ctypes.c_int32


def test_launcher_refusals_are_host_checks_that_name_the_function():
    """Every bad argument is refused with KEEP_EINVAL on a machine without a GPU: the checks run on the host before the first launch, and
    the device pointers (placeholders here) are never dereferenced."""
    lib = raw_lib()
    f = getattr(lib, NAME)
    f.restype = ctypes.c_int32
    f.argtypes = [ctypes.c_void_p] + [ctypes.c_int32] * 3 + [ctypes.c_void_p] + [ctypes.c_int32] * 4 + [ctypes.c_void_p] * 3 + \
                 [ctypes.c_int32] * 3 + [ctypes.c_void_p]
    ident = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]

    def call(N=3, H=37, W=53, n_slots=5, F=2, dh=24, dw=40, frame_of=(0, 2), slot_of=(4, 1), mats=None, null=None):
        idx = (ctypes.c_int32 * max(1, len(frame_of)))(*frame_of)
        slots = (ctypes.c_int32 * max(1, len(slot_of)))(*slot_of)
        m = (ctypes.c_double * (6 * max(1, len(frame_of))))(*(mats if mats is not None else ident * len(frame_of)))
        ptr = [0x1000, 0x2000, ctypes.addressof(idx), ctypes.addressof(slots), ctypes.addressof(m)]   # frames, dst: placeholders
        if null is not None:
            ptr[null] = None
        return f(ptr[0], N, H, W, ptr[1], n_slots, F, dh, dw, ptr[2], ptr[3], ptr[4], 135, 133, 132, None)
    # what the existing entry refuses
    refused = [dict(null=i) for i in range(5)]
    refused += [dict(N=0), dict(N=-1), dict(F=0), dict(F=-2), dict(H=0), dict(W=0), dict(dh=0), dict(dw=0), dict(H=-5), dict(dw=-1),
                dict(H=32768), dict(W=32768), dict(W=40000),
                dict(frame_of=(0, 3)), dict(frame_of=(-2, 0)), dict(frame_of=(3, 0)), dict(N=1, frame_of=(0, 1)),
                dict(mats=ident + [1.0, 0.0, float('nan'), 0.0, 1.0, 0.0]), dict(mats=[float('inf')] + ident[1:] + ident),
                dict(mats=ident + ident[:5] + [float('-inf')]),
                dict(frame_of=(-1, 0), mats=[float('nan')] + ident[1:] + ident)]
    # ... and the slots: fewer slots than faces, a slot outside 0 .. n_slots - 1, a slot named twice
    refused += [dict(n_slots=1), dict(n_slots=0), dict(n_slots=-3), dict(slot_of=(0, 5)), dict(slot_of=(5, 0)), dict(slot_of=(-1, 0)),
                dict(slot_of=(0, -1)), dict(slot_of=(3, 3)), dict(slot_of=(0, 0)), dict(n_slots=2, slot_of=(2, 0)),
                dict(F=3, frame_of=(0, 1, 2), slot_of=(4, 0, 4)), dict(frame_of=(-1, 0), slot_of=(2, 2))]
    for kw in refused:
        assert call(**kw) == -1, kw
        assert lib.keep_last_error().startswith(NAME.encode() + b':'), (kw, lib.keep_last_error())
    # 40 faces (two launches) with one slot named by the first and the last face: refused before anything is launched
    F = 40
    assert call(N=1, F=F, n_slots=64, frame_of=(0,) * F, slot_of=tuple(range(F - 1)) + (0,)) == -1
    assert b'twice' in lib.keep_last_error()
