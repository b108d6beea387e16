"""GPU suite: the RetinaFace detector on the worker pool (engine/pool.py ``set_detector`` / ``detect``) and the engine's
``packed()`` / ``from_packed()`` round trip on the device.  Two workers on the one device (KEEP_DIST_DEVICE, gloo wire for the one
weight broadcast): three processes with the GPU open."""
import threading

import numpy as np
import pytest
import torch

from comfyui_keep_amd.engine.arch import DEFAULT_ARCH

pytestmark = pytest.mark.gpu


def _within(seconds, pool, fn):
    """``fn()`` under a time limit of its own: past it (a worker that hangs) the workers are killed, the pool is closed and the test
    ends there -- nothing is retried."""
    box = {}

    def run():
        try:
            box['value'] = fn()
        except BaseException as e:
            box['error'] = e
    t = threading.Thread(target=run, daemon=True)
    t.start()
    t.join(seconds)
    if t.is_alive():
        if pool is not None:
            for p in list(pool._procs):
                p.kill()
            pool.close()
        pytest.fail(f"no answer within {seconds} s: the workers were killed")
    if 'error' in box:
        raise box['error']
    return box['value']


def _frames(n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8).numpy()


def _equal(got, want):
    return len(got) == len(want) and all(a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b) for a, b in zip(got, want))


def test_pool_detect_on_two_workers_equals_the_root_engine(synth_weights, monkeypatch):
    """mobile0.25 (synthetic weights, two frames per detector call): five 96 x 128 frames -> chunks of 2, 2 and 1 frames on ranks 0, 1
    and 2.  ``pool.detect`` returns, frame by frame, the arrays the root engine's ``detect_batch`` returns on the same frames, bit for
    bit; then resnet50 on two frames (another engine object: the detector travels again, chunk 1 runs on worker 1)."""
    from comfyui_keep_amd.engine import retinaface as RF
    from comfyui_keep_amd.engine.net import KeepNet
    from comfyui_keep_amd.engine.pool import GpuPool
    monkeypatch.setenv('KEEP_DIST_DEVICE', '0')
    monkeypatch.setenv('KEEP_AMD_DETECT_BATCH', '2')
    net = KeepNet(**DEFAULT_ARCH)
    net.load_state_dict(synth_weights, strict=True)
    net.to('cuda').eval()
    mnet = RF.RetinaFaceEngine(RF.synth_retinaface_state_dict(seed=0, backbone='mobile0.25')).to('cuda')
    assert mnet.max_frames == 2
    frames = _frames(5, 96, 128, seed=21)
    want = mnet.detect_batch(frames, 0.7)
    assert sum(len(w) for w in want) > 0                              # (there is something to compare)
    pool = _within(240, None, lambda: GpuPool(net, 3, timeout=180, join_timeout=60))
    try:
        assert len(pool._procs) == 2 and not torch.distributed.is_initialized()
        _within(120, pool, lambda: pool.set_detector(mnet))
        chunks = [frames[0:2], frames[2:4], frames[4:5]]
        got = _within(120, pool, lambda: pool.detect(chunks, 0.7))
        assert _equal(got, want)
        assert pool.detector_calls == {1: 1, 2: 1}
        print('pool.detect, mobile0.25, 5 frames on 3 ranks of one device: ms inside the detector per rank',
              {r: round(v, 1) for r, v in sorted(pool.detect_ms.items())})
        # device tensors as chunks (what a helper that resizes on the device hands over), and the helper's threshold
        got = _within(120, pool, lambda: pool.detect([torch.from_numpy(c).cuda() for c in chunks], 0.97))
        assert _equal(got, mnet.detect_batch(frames, 0.97))
        r50 = RF.RetinaFaceEngine(RF.synth_retinaface_state_dict(seed=0)).to('cuda')
        two = _frames(2, 96, 128, seed=22)
        want50 = r50.detect_batch(two, 0.6)
        assert sum(len(w) for w in want50) > 0
        _within(180, pool, lambda: pool.set_detector(r50))
        got50 = _within(120, pool, lambda: pool.detect([two[0:1], two[1:2]], 0.6))
        assert _equal(got50, want50)
        assert pool.detector_calls == {1: 3, 2: 2}                    # worker 1: one chunk in each of the three calls; worker 2: none of resnet50's
    finally:
        procs = list(pool._procs)
        pool.close()
    assert all(p.poll() is not None for p in procs)


@pytest.mark.parametrize('precision', ['x3', 'f16'])
@pytest.mark.parametrize('backbone', ['mobile0.25', 'resnet50'])
def test_from_packed_round_trip_on_the_device(backbone, precision):
    """``RetinaFaceEngine.from_packed(*engine.packed()).to('cuda')``: the head outputs and the detections of the rebuilt engine equal the
    original's bit for bit, under the default policy and under 'f16' (whose twins are derived again from the same blob)."""
    from comfyui_keep_amd.engine import retinaface as RF
    eng = RF.RetinaFaceEngine(RF.synth_retinaface_state_dict(seed=0, backbone=backbone), precision=precision).to('cuda')
    twin = RF.RetinaFaceEngine.from_packed(*eng.packed()).to('cuda')
    assert twin is not eng and twin._dev.data_ptr() != eng._dev.data_ptr() and twin.precision == precision
    frames = _frames(3, 96, 128, seed=23)
    x = torch.from_numpy(frames).cuda().float() - torch.tensor(RF.MEAN_BGR, device='cuda')
    assert torch.equal(twin.raw_heads(x), eng.raw_heads(x))
    thr = 0.7 if backbone == 'mobile0.25' else 0.6
    want = eng.detect_batch(frames, thr)
    assert sum(len(w) for w in want) > 0
    assert _equal(twin.detect_batch(frames, thr), want)
