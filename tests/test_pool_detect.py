"""CPU suite: the detection pre-pass over the worker pool (engine/pool.py ``set_detector`` / ``detect``, modules/keep_processor.py
``_detect_all``) on gloo with the stand-in engine (KEEP_POOL_FAKE_NET=1), and ``RetinaFaceEngine.packed()`` / ``from_packed()``.
The workers' stand-in detector is ``pool_worker.fake_detect_batch``: one row per frame, a function of the frame's bytes, so the order
and the content of what comes back can be compared with a local run over the concatenated frames."""
import time

import numpy as np
import pytest
import torch

from test_dist_gloo import _FakeRootNet, _pool_env

H, W = 8, 12


class _RootDetectorEngine:
    """The root's side of the stand-in detector: what ``GpuPool.set_detector`` packs and what runs the root's own chunks."""
    pool_kind = 'retinaface'

    def __init__(self, max_frames=3):
        self.max_frames = max_frames
        self.calls, self.frames_seen, self.packed_calls = 0, 0, 0

    def packed(self):
        self.packed_calls += 1
        return ('stand-in detector',)

    def detect_batch(self, frames, conf_threshold=0.8):
        from comfyui_keep_amd.engine.pool_worker import fake_detect_batch
        self.calls += 1
        self.frames_seen += len(frames)
        return fake_detect_batch(frames, conf_threshold)


def _chunks(sizes, seed=0):
    g = np.random.default_rng(seed)
    return [g.integers(0, 256, (n, H, W, 3), dtype=np.uint8) for n in sizes]


def _same(got, want):
    return len(got) == len(want) and all(a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b) for a, b in zip(got, want))


def test_fake_detector_tells_frames_and_order_apart():
    """The stand-in must make a swapped or repeated frame visible, or the order checks below check nothing."""
    from comfyui_keep_amd.engine.pool_worker import fake_detect_batch
    fr = _chunks([6])[0]
    rows = fake_detect_batch(fr, 0.97)
    assert len(rows) == 6 and all(r.shape == (1, 15) and r.dtype == np.float32 for r in rows)
    assert len({r.tobytes() for r in rows}) == 6
    assert _same(fake_detect_batch(fr[::-1], 0.97), rows[::-1]) and float(rows[0][0, 4]) == np.float32(0.97)
    swapped = fr[0].copy()
    swapped[0, 0], swapped[0, 1] = fr[0][0, 1], fr[0][0, 0]           # same bytes, another place
    assert not np.array_equal(fake_detect_batch(swapped[None], 0.97)[0], rows[0])


def test_pool_detect_world4_ragged_chunks_order_and_arena_reuse(monkeypatch):
    """World 4, seven chunks of ragged sizes (the last one shorter): chunk k runs on rank k % 4, the per-frame results come back in frame
    order and equal the stand-in run locally over the concatenated frames; a second call reuses the shared-memory arenas; the detector
    travels once per engine object; tensors are taken like arrays; ``detect`` before ``set_detector`` is refused."""
    _pool_env(monkeypatch)
    from comfyui_keep_amd.engine.pool import GpuPool, PoolError
    from comfyui_keep_amd.engine.pool_worker import fake_detect_batch
    net = _FakeRootNet()
    pool = net.pool = GpuPool(net, 4, timeout=120, join_timeout=60)
    try:
        chunks = _chunks([3, 3, 1, 3, 2, 3, 1])
        with pytest.raises(PoolError, match='set_detector'):
            pool.detect(chunks, 0.97)
        assert not pool.closed and not pool._arenas                    # refused on the root: nothing was sent, the pool lives on
        eng = _RootDetectorEngine()
        pool.set_detector(eng)
        pool.set_detector(eng)
        assert eng.packed_calls == 1                                   # sent once per engine object
        want = fake_detect_batch(np.concatenate(chunks), 0.97)
        got = pool.detect(chunks, 0.97)
        assert _same(got, want)
        assert (eng.calls, eng.frames_seen) == (2, 5)                  # the root ran chunks 0 and 4
        assert pool.detector_calls == {1: 2, 2: 2, 3: 1}               # ranks 1, 2: two chunks each, rank 3: chunk 3
        assert sorted(pool.detect_ms) == [0, 1, 2, 3]
        arenas = {r: tuple(m.name for m in pair) for r, pair in pool._arenas.items()}
        assert sorted(arenas) == [1, 2, 3]
        # a second call whose sizes fit: same blocks; other content, other chunking, tensors instead of arrays, another threshold
        chunks2 = [torch.from_numpy(c) for c in _chunks([2, 3, 3, 1, 1], seed=1)]
        got2 = pool.detect(chunks2, 0.5)
        assert _same(got2, fake_detect_batch(torch.cat(chunks2).numpy(), 0.5))
        assert {r: tuple(m.name for m in pair) for r, pair in pool._arenas.items()} == arenas
        assert pool.detector_calls == {1: 3, 2: 3, 3: 2}
        # the clips' path shares the arenas with the detection: still whole after a detect, and the other way round
        clips = [torch.from_numpy(c) for c in _chunks([2, 1, 3, 2, 1], seed=2)]
        assert all(torch.equal(o, 255 - c) for o, c in zip(pool.run(net, clips), clips))
        assert _same(pool.detect(chunks, 0.97), want)
        assert {r: tuple(m.name for m in pair) for r, pair in pool._arenas.items()} == arenas
        # fewer chunks than ranks, and none at all
        assert _same(pool.detect(chunks[:2], 0.97), want[:6]) and pool.detect([], 0.97) == []
        # another engine object travels again
        eng2 = _RootDetectorEngine()
        pool.set_detector(eng2)
        assert eng2.packed_calls == 1 and _same(pool.detect(chunks, 0.97), want) and eng2.calls == 2
        assert sorted(pool.detect_ms_total) == [0, 1, 2, 3] and all(pool.detect_ms_total[r] >= pool.detect_ms[r] for r in range(4))
    finally:
        pool.close()
    with pytest.raises(PoolError, match='closed'):
        pool.detect(chunks, 0.97)


def test_pool_detect_refuses_bad_chunks_whole_and_never_loses_new_arena_names(monkeypatch):
    """A chunk that is not uint8 [n, H, W, 3] is refused before any arena is touched, wherever it stands in the list: the pool stays open
    and the next call is right.  Arenas that grew without a request having carried their names (a call that failed on the root in
    between) are announced by the next request: the worker never reads a block the root has left.  A detector of a kind the workers do
    not rebuild is refused on the root."""
    _pool_env(monkeypatch)
    from comfyui_keep_amd.engine.pool import GpuPool, PoolError
    from comfyui_keep_amd.engine.pool_worker import fake_detect_batch
    net = _FakeRootNet()
    pool = net.pool = GpuPool(net, 3, timeout=120, join_timeout=60)
    try:
        other = _RootDetectorEngine()
        other.pool_kind = 'yolov5face'
        assert not pool.takes_detector(other) and not pool.takes_detector(object())
        with pytest.raises(PoolError, match='kind'):
            pool.set_detector(other)
        assert not pool.closed and other.packed_calls == 0
        pool.set_detector(_RootDetectorEngine())
        chunks = _chunks([2, 2, 1])
        assert _same(pool.detect(chunks, 0.97), fake_detect_batch(np.concatenate(chunks), 0.97))
        arenas = {r: tuple(m.name for m in pair) for r, pair in pool._arenas.items()}
        big = _chunks([2, 4000, 1], seed=4)                             # rank 1's input arena would have to grow for this call ...
        assert big[1].nbytes > pool._arenas[1][0].size
        for bad in (big[2].astype(np.float32), big[2][..., :2], big[2][0]):     # ... but its last chunk is refused first
            with pytest.raises((TypeError, ValueError), match='chunk 2'):
                pool.detect(big[:2] + [bad], 0.97)
            assert not pool.closed and {r: tuple(m.name for m in pair) for r, pair in pool._arenas.items()} == arenas
        assert _same(pool.detect(chunks, 0.97), fake_detect_batch(np.concatenate(chunks), 0.97))
        # rank 1's arena grows and no request follows: the names are still owed, and the next request -- of either kind -- pays
        pool._arena(1, 2 * pool._arenas[1][0].size, 0)
        assert pool._names_unsent == {1} and pool._arenas[1][0].name != arenas[1][0]
        chunks2 = _chunks([1, 3, 2], seed=5)
        assert _same(pool.detect(chunks2, 0.5), fake_detect_batch(np.concatenate(chunks2), 0.5)) and not pool._names_unsent
        pool._arena(2, 2 * pool._arenas[2][0].size, 0)
        clips = [torch.from_numpy(c) for c in _chunks([2, 1, 3], seed=6)]
        assert all(torch.equal(o, 255 - c) for o, c in zip(pool.run(net, clips), clips)) and not pool._names_unsent
        assert _same(pool.detect(big, 0.97), fake_detect_batch(np.concatenate(big), 0.97))
    finally:
        pool.close()


def test_pool_detect_worker_failure_surfaces_and_closes_the_pool(monkeypatch):
    """A worker that raises inside ``detect`` (KEEP_POOL_TEST_FAIL stage 'detect', stand-in engine only): the caller gets the worker's
    traceback well within the join timeout and the pool is closed -- no worker and no arena is left, as after a failing ``run``."""
    _pool_env(monkeypatch, KEEP_POOL_TEST_FAIL='2:detect')
    from comfyui_keep_amd.engine.pool import GpuPool, PoolError
    net = _FakeRootNet()
    join_timeout = 60
    pool = net.pool = GpuPool(net, 3, timeout=120, join_timeout=join_timeout)
    try:
        procs = list(pool._procs)
        eng = _RootDetectorEngine()
        pool.set_detector(eng)
        t0 = time.monotonic()
        with pytest.raises(PoolError) as e:
            pool.detect(_chunks([2, 2, 2, 1]), 0.97)
        assert time.monotonic() - t0 < join_timeout
        assert 'injected failure inside detect' in str(e.value) and 'Traceback' in str(e.value) and 'pool worker 2' in str(e.value)
        assert pool.closed and not pool._procs and not pool._arenas and all(p.poll() is not None for p in procs)
    finally:
        pool.close()


class _Helper:
    """The helper calls ``_detect_all`` makes, with a detector-call counter as tools/synth_facehelper.py keeps one."""
    det_model = 'retinaface_resnet50'

    def __init__(self, det):
        self.face_detector = det
        self.detector_calls = 0

    def clean_all(self):
        self.all_landmarks_5, self.input_img = [], None

    def read_image(self, img):
        self.input_img = img

    def get_face_landmarks_5(self, only_center_face=False, resize=640, eye_dist_threshold=None):
        if hasattr(self.face_detector, 'engine'):
            self.detector_calls += 1                                  # (a per-frame call of the real detector, not a replay)
        b = self.face_detector.detect_faces(self.input_img, 0.97)
        self.all_landmarks_5 = [b[i, 5:].reshape(5, 2) for i in range(b.shape[0])]
        return len(self.all_landmarks_5)


class _Det:
    def __init__(self, max_frames=3):
        self.engine = _RootDetectorEngine(max_frames)

    def detect_batch(self, frames, conf_threshold=0.8):
        return self.engine.detect_batch(frames, conf_threshold)

    def detect_faces(self, image, conf_threshold=0.8):
        return self.engine.detect_batch(np.asarray(image)[None], conf_threshold)[0]


def test_detect_all_over_the_pool_equals_the_root_only_prepass(monkeypatch):
    """``_detect_all`` with a live pool (world 3): 20 frames in chunks of 3 -> 7 chunks -> windows of 3, 3 and 1 chunks.  The landmark
    lists equal the root-only pre-pass (KEEP_AMD_POOL_DETECT=0) bit for bit, with and without the overlap thread; with the knob unset the
    workers' detectors saw their chunks and the root's only its own; a chunk of mixed frame sizes takes the per-frame path on the root; a
    detector whose engine does not travel, a single chunk and a closed pool all stay on the root."""
    _pool_env(monkeypatch)
    import test_host_logic as HL        # installs the ComfyUI stubs
    from comfyui_keep_amd.engine.pool import GpuPool
    from comfyui_keep_amd.modules.keep_model_loader import KEEPModelPack
    from comfyui_keep_amd.modules.keep_processor import KEEPFaceProcessor
    frames = list(_chunks([20], seed=3)[0])
    net = _FakeRootNet()
    pool = net.pool = GpuPool(net, 3, timeout=120, join_timeout=60)
    try:
        def run(frames, det=None):
            det = det or _Det()
            helper = _Helper(det)
            out = KEEPFaceProcessor(KEEPModelPack(net, helper, None, None, 'KEEP'))._detect_all(frames, True)
            assert helper.face_detector is det
            return out, det, helper

        def same(a, b):
            return len(a) == len(b) and all(len(x) == len(y) == 1 and np.array_equal(x[0], y[0]) for x, y in zip(a, b))

        monkeypatch.setenv('KEEP_AMD_POOL_DETECT', '0')
        solo, det0, _ = run(frames)
        assert (det0.engine.calls, det0.engine.frames_seen, det0.engine.packed_calls) == (7, 20, 0) and pool.detector_calls == {}
        assert len(solo) == 20 and len({s[0].tobytes() for s in solo}) == 20
        monkeypatch.delenv('KEEP_AMD_POOL_DETECT')
        for overlap in ('1', '0'):
            monkeypatch.setenv('KEEP_AMD_DETECT_OVERLAP', overlap)
            before = dict(pool.detector_calls)
            pooled, det1, helper = run(frames)
            assert same(pooled, solo)
            # chunks 0, 3, 6 on the root (3 + 3 + 2 frames), 1 and 4 on worker 1, 2 and 5 on worker 2
            assert (det1.engine.calls, det1.engine.frames_seen, det1.engine.packed_calls) == (3, 8, 1)
            assert {r: pool.detector_calls[r] - before.get(r, 0) for r in (1, 2)} == {1: 2, 2: 2}
            assert helper.detector_calls == 0                          # every frame replayed stored detections
        monkeypatch.delenv('KEEP_AMD_DETECT_OVERLAP')
        # frames 3..5 (chunk 1) of mixed sizes: that chunk runs frame by frame on the root, its neighbours on the pool
        mixed = list(frames)
        mixed[4] = np.ascontiguousarray(frames[4][:, :10])
        monkeypatch.setenv('KEEP_AMD_POOL_DETECT', '0')
        solo_m, _, _ = run(mixed)
        monkeypatch.delenv('KEEP_AMD_POOL_DETECT')
        before = dict(pool.detector_calls)
        pooled_m, det_m, helper_m = run(mixed)
        assert same(pooled_m, solo_m) and helper_m.detector_calls == 3
        assert sum(pool.detector_calls[r] - before[r] for r in (1, 2)) == 3       # six batched chunks: 0, 2 | 3, 4, 5 | 6 -> ranks 0,1 | 0,1,2 | 0
        # nothing travels: an engine without packed(), an engine of a kind the workers do not rebuild, a video of one chunk
        before = dict(pool.detector_calls)
        det_k = _Det()
        det_k.engine.pool_kind = 'yolov5face'
        kind, _, _ = run(frames, det_k)
        assert same(kind, solo) and (det_k.engine.calls, det_k.engine.packed_calls) == (7, 0)

        class _Yolo(_Det):
            def __init__(self):
                self.engine = type('E', (), {'max_frames': 3})()
                self.inner = _RootDetectorEngine()

            def detect_batch(self, frames, conf_threshold=0.8):
                return self.inner.detect_batch(frames, conf_threshold)

            def detect_faces(self, image, conf_threshold=0.8):
                return self.inner.detect_batch(np.asarray(image)[None], conf_threshold)[0]
        other, det_y, _ = run(frames, _Yolo())
        assert same(other, solo) and det_y.inner.calls == 7
        one, det_1, _ = run(frames[:3])
        assert same(one, solo[:3]) and (det_1.engine.calls, det_1.engine.packed_calls) == (1, 0)
        assert pool.detector_calls == before
    finally:
        pool.close()
    after, det_c, _ = run(frames)                                      # a closed pool: the root-only pre-pass
    assert same(after, solo) and (det_c.engine.calls, det_c.engine.packed_calls) == (7, 0)


@pytest.mark.parametrize('backbone', ['mobile0.25', 'resnet50'])
def test_retinaface_engine_packed_round_trip_on_the_host(backbone, monkeypatch):
    """``RetinaFaceEngine.from_packed(*engine.packed())``: same index, same blob bytes, same backbone / precision / resolved settings --
    the settings the ORIGINAL read from its environment, not the rebuilding process's -- and it survives pickling (the control
    connection's transport)."""
    import pickle
    from comfyui_keep_amd.engine import retinaface as RF
    monkeypatch.setenv('KEEP_AMD_DETECT_BATCH', '2')
    monkeypatch.setenv('KEEP_AMD_DETECT_SURVIVORS', '1024')
    monkeypatch.setenv('KEEP_AMD_DEVICE_NMS', '0')
    eng = RF.RetinaFaceEngine(RF.synth_retinaface_state_dict(seed=0, backbone=backbone), precision='f16')
    assert eng.settings() == {'max_survivors': 1024, 'max_frames': 2, 'device_nms': False}
    for k in ('KEEP_AMD_DETECT_BATCH', 'KEEP_AMD_DETECT_SURVIVORS', 'KEEP_AMD_DEVICE_NMS'):
        monkeypatch.delenv(k)
    twin = RF.RetinaFaceEngine.from_packed(*pickle.loads(pickle.dumps(eng.packed())))
    assert list(twin._index.items()) == list(eng._index.items())
    assert twin._blob.dtype == eng._blob.dtype and twin._blob.tobytes() == eng._blob.tobytes()
    assert (twin.backbone, twin.precision, twin.cfg, twin._act) == (eng.backbone, 'f16', eng.cfg, eng._act)
    assert twin.settings() == eng.settings()
    assert twin.x3_names() == eng.x3_names() and twin.x1_names() == eng.x1_names()
    assert twin.device == torch.device('cpu') and twin.w is None and twin._priors == {} and twin._priors_dev == {}
    assert set(vars(twin)) == set(vars(eng))                           # nothing the constructor sets is missing in a rebuilt engine
    plain = RF.RetinaFaceEngine.from_packed(eng._blob, eng._index, backbone)
    assert plain.precision == 'x3' and plain.settings() == {'max_survivors': 4096, 'max_frames': 32, 'device_nms': True}
    with pytest.raises(ValueError):
        RF.RetinaFaceEngine.from_packed(eng._blob, eng._index, 'resnet18')
    with pytest.raises(ValueError):
        RF.RetinaFaceEngine.from_packed(eng._blob, eng._index, backbone, precision='bf16')
