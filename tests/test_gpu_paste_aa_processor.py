"""GPU suite (-m gpu): the alias-free paste-back knob (KEEP_AMD_PASTE_AA; modules/keep_processor.py) through the product's own entry
points over tools/synth_facehelper.py.

The synthetic helper's faces span 0.35 of the frame height: on 576-row frames the crop -> frame scale is r = 0.39, so the rule takes
N = 4; with ``final_upscale_factor`` 3 it is r = 1.18, N = 1, and the knob changes nothing.  The kernel's arithmetic is pinned by
tests/test_gpu_paste_aa.py; here: every path a sequence takes gives the same frames, the network never sees the knob, nothing outside
the face boxes changes, a fade arrives as the entry's opacity, and knob off is an untouched processor."""
import os
import sys

import numpy as np
import pytest
import torch

from test_gpu_frame_store import Rig, net  # noqa: F401  (``net``: the module's fixture)
from test_gpu_track_lifetimes import PATHS, Drops, knobs, outside, same_frames, video

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))

CORE, W, AA = 'keep_paste_face', 'keep_paste_face_w', 'keep_paste_face_aa'
HW = (576, 512)


def run(rig, frames, env=(), factor=1.0, clip=4, start=0):
    """One ``process_frames_u8`` call -> (frames as a list of uint8 arrays, restored faces)."""
    for k in ('KEEP_AMD_FRAME_STORE', 'KEEP_AMD_STREAM_PASTE', 'KEEP_AMD_DETECT_BATCH'):
        rig.mp.delenv(k, raising=False)
    for k, v in env:
        rig.mp.setenv(k, v)
    rig.mp.setenv('KEEP_AMD_STREAM_GROUPS', '3')
    for rec in (rig.calls, rig.backgrounds, rig.batches, rig.crop_shapes):
        rec.clear()
    rig.helper.frame_index = start
    out = rig.proc.process_frames_u8(frames, factor, False, False, False, max_clip_length=clip)
    out = [f for f in out.cpu().numpy()] if isinstance(out, torch.Tensor) else [np.asarray(f) for f in out]
    return out, [np.asarray(f) for f in rig.proc.last_restored_faces]


def boxes_mask(n, faces, hw):
    """Per frame the union of the face boxes, bool [H,W]: ``face_box`` of the helper's own similarity, one pixel wider than the paste's
    (the fitted matrix equals the synthetic one up to rounding)."""
    import synth_facehelper as SF
    from comfyui_keep_amd.engine.paste import face_box
    out = []
    for t in range(n):
        m = np.zeros(hw, bool)
        for i in range(faces):
            x0, y0, x1, y1 = face_box(SF.track_similarity(t, i, hw[0], hw[1], faces), 512, 512, hw[1], hw[0], margin=3)
            m[y0:y1, x0:x1] = True
        out.append(m)
    return out


def test_every_path_gives_the_same_frames_and_the_network_never_sees_the_knob(net, monkeypatch):
    n, faces = 5, 2
    rig = Rig(net, monkeypatch, HW, faces, chunk=4)
    frames = video(n, 81, *HW)
    off, off_faces = run(rig, frames)
    assert rig.count(AA) == 0 and rig.count(CORE) == n * faces and not hasattr(rig.proc, 'last_paste_aa')
    rig.proc.paste_aa = True
    got = {}
    for path, env in PATHS.items():
        got[path] = run(rig, frames, env=env)
        assert rig.count(AA) == n * faces and rig.count(CORE) == 0 and rig.count(W) == 0, path
        assert rig.proc.last_paste_aa == {4: n * faces}, path
        assert rig.crop_shapes == ({'store': [('Tensor', n * faces)], 'streamed': [('list', n * faces)], 'per-frame': []}[path])
    on, on_faces = got['store']
    for path in ('streamed', 'per-frame'):
        assert same_frames(got[path][0], on), path
        assert len(got[path][1]) == n * faces and all(np.array_equal(x, y) for x, y in zip(got[path][1], on_faces)), path
    assert len(on_faces) == len(off_faces) == n * faces and all(np.array_equal(x, y) for x, y in zip(on_faces, off_faces))
    inside = boxes_mask(n, faces, HW)
    for t in range(n):
        changed = (on[t] != off[t]).any(axis=2)
        assert changed.any() and not (changed & ~inside[t]).any(), t
        assert np.array_equal(on[t][~inside[t]], frames[t][~inside[t]]), t


def test_an_enlarging_final_upscale_factor_takes_todays_calls(net, monkeypatch):
    """factor 3: r = 1.18, the face is not shrunk on its way back -- N = 1, the output is the knob-off run's entirely."""
    n = 2
    rig = Rig(net, monkeypatch, HW, 1, chunk=4)
    frames = video(n, 82, *HW)
    off, off_faces = run(rig, frames, factor=3.0)
    names = list(rig.calls)
    rig.proc.paste_aa = True
    on, on_faces = run(rig, frames, factor=3.0)
    assert sorted(rig.calls) == sorted(names) and rig.count(AA) == 0 and rig.count(CORE) == n and rig.proc.last_paste_aa == {1: n}
    assert on[0].shape == (3 * HW[0], 3 * HW[1], 3) and same_frames(on, off)
    assert all(np.array_equal(x, y) for x, y in zip(on_faces, off_faces))


def test_track_fade_reaches_the_entry_as_its_opacity(net, monkeypatch):
    """One face on frames 2-8 of 10, ``track_fade`` 2: the entry is called once per live frame with N = 4 and the weights the rule gives,
    and a faded frame is the by-hand ``GpuPaster.paste(weights=..., aa=True)`` of the same restored face."""
    from comfyui_keep_amd.engine import hiplib as L
    from comfyui_keep_amd.engine.paste import GpuPaster
    n, a, b = 10, 2, 8
    rig = Rig(net, monkeypatch, HW, 1, chunk=4)
    drops = Drops(monkeypatch)
    drops.drop, drops.offset = outside(n, a, b), 0
    seen, recording = [], L.call
    monkeypatch.setattr(L, 'call', lambda name, *args: (seen.append((int(args[-2]), float(args[-1].value))) if name == AA else None,
                                                        recording(name, *args))[1])
    inverse, own = [], rig.helper.get_inverse_affine

    def rec(*args, **kw):
        own(*args, **kw)
        inverse.append([np.array(M) for M in rig.helper.inverse_affine_matrices])
    rig.helper.get_inverse_affine = rec
    frames = video(n, 83, *HW)
    knobs(rig.proc, track_lifetimes=True, fade=2)
    rig.proc.paste_aa = True
    out, faces = run(rig, frames)
    third, two = float(np.float32(1.0 / 3.0)), float(np.float32(2.0 / 3.0))
    assert rig.count(AA) == b - a + 1 and rig.count(W) == 0 and rig.count(CORE) == 0 and rig.proc.last_paste_aa == {4: b - a + 1}
    assert seen == [(4, third), (4, two), (4, 1.0), (4, 1.0), (4, 1.0), (4, two), (4, third)]
    assert all(np.array_equal(out[t], frames[t]) for t in range(n) if t < a or t > b)
    # frame a by hand
    seen.clear()
    fd = torch.from_numpy(faces[0][None]).cuda()
    x = torch.empty(fd.shape, dtype=torch.float32, device='cuda')
    L.call('keep_img2tensor', fd, x, fd.numel() // 3)
    cls = rig.helper.face_parse.engine.classes(x)
    want = GpuPaster('cuda').paste(frames[a], fd, inverse[0], cls, 1.0, False, weights=[third], aa=True).cpu().numpy()
    assert np.array_equal(out[a], want) and not np.array_equal(out[a], frames[a])


def test_knob_off_is_an_untouched_processor_and_the_single_image_node_takes_the_knob(net, monkeypatch):
    n, faces = 3, 1
    frames = video(n, 84, *HW)
    fresh = Rig(net, monkeypatch, HW, faces, chunk=4)
    want = run(fresh, frames)
    assert fresh.proc.paste_aa is False and not hasattr(fresh.proc, 'last_paste_aa') and fresh.count(AA) == 0
    rig = Rig(net, monkeypatch, HW, faces, chunk=4)
    rig.proc.paste_aa = True
    on = run(rig, frames)
    assert rig.count(AA) == n and not same_frames(on[0], want[0])
    rig.proc.paste_aa = False
    off = run(rig, frames)
    assert rig.count(AA) == 0 and rig.count(CORE) == n * faces
    assert same_frames(off[0], want[0]) and all(np.array_equal(x, y) for x, y in zip(off[1], want[1]))
    # the single-image node
    rig.calls.clear()
    rig.helper.frame_index = 0
    plain = np.asarray(rig.proc.process_image(frames[0], 1.0, False, False, False))
    assert rig.count(AA) == 0 and rig.count(CORE) == 1
    rig.proc.paste_aa = True
    rig.calls.clear()
    rig.helper.frame_index = 0
    img = np.asarray(rig.proc.process_image(frames[0], 1.0, False, False, False))
    assert rig.count(AA) == 1 and rig.count(CORE) == 0 and rig.proc.last_paste_aa == {4: 1}
    inside = boxes_mask(1, 1, HW)[0]
    assert img.shape == plain.shape == frames[0].shape and (img != plain).any() and np.array_equal(img[~inside], plain[~inside])
