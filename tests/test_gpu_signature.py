"""GPU suite (-m gpu): keep_frame_signature_u8 (csrc/keep_signature.hip) alone, against its host restatement
(modules/scene_cuts.py:frame_signature_host) -- integers, so EXACTLY -- on the smallest shapes that reach every way the kernel can go
wrong: rows whose byte length is no multiple of 4 or 16 (37 x 53, 3 x 5), cells smaller than a wave and empty cells (3 x 5, 1 x 1),
several rows per block (130 x 258), a row segment longer than one block's threads (9 x 4099: 1025 pixels per cell row) -- all of which
the launcher gives ONE block per cell -- and, in BANDED, cells cut into several blocks, which every real video size is (4 bands per
cell at 720p, 8 at 1080p)."""
import numpy as np
import pytest
import torch

from comfyui_keep_amd.engine import hiplib as L
from comfyui_keep_amd.modules.scene_cuts import frame_signature_host

pytestmark = pytest.mark.gpu

NAME = 'keep_frame_signature_u8'
SHAPES = [(3, 37, 53), (2, 3, 5), (1, 1, 1), (5, 130, 258), (2, 9, 4099)]
# A block takes rpb = 4096 // gpr_max rows of a cell, gpr_max = ceil(ceil(W / 4) / 4) groups of 4 pixels per row, and a cell row has at most
# ceil(H / 4) rows (csrc/keep_signature.hip).  70 x 4099: gpr_max 257, rpb 15, cell rows of 18 / 17 / 18 / 17 rows -> 2 bands, the second
# of 3 or 2 rows.  1100 x 260: gpr_max 17, rpb 240, cell rows of 275 rows -> 2 bands, the second of 35.  543 x 1030: gpr_max 65, rpb 63,
# cell rows of 136 / 136 / 136 / 135 -> 3 bands, the third of 10 or 9 rows.
BANDED = [(2, 70, 4099, 2), (1, 1100, 260, 2), (2, 543, 1030, 3)]
GUARD, PATTERN, GARBAGE = 64, 0x5A5A5A5A, -12345


def bands(H, W):
    """Blocks per cell of the launcher's geometry, restated."""
    gpr_max = ((W + 3) // 4 + 3) // 4
    rpb = 4096 // gpr_max
    return -(-((H + 3) // 4) // rpb)


def contents(N, H, W):
    """name -> uint8 [N,H,W,3]: noise, the flat extremes, lumas on both sides of every bin boundary, a horizontal and a vertical ramp."""
    rng = np.random.default_rng(N * 1000003 + H * 1009 + W)
    out = {'noise': rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8),
           'flat0': np.zeros((N, H, W, 3), np.uint8), 'flat255': np.full((N, H, W, 3), 255, np.uint8)}
    edges = np.array([v for b in range(1, 16) for v in (16 * b - 1, 16 * b)] + [0, 255], np.uint8)      # grey g has luma g
    out['straddle'] = np.repeat(edges[(np.arange(N * H * W) * 7) % len(edges)].reshape(N, H, W, 1), 3, axis=3)
    out['hramp'] = np.broadcast_to(((np.arange(W) * 255) // max(W - 1, 1)).astype(np.uint8)[None, None, :, None], (N, H, W, 3)).copy()
    out['vramp'] = np.broadcast_to(((np.arange(H) * 255) // max(H - 1, 1)).astype(np.uint8)[None, :, None, None], (N, H, W, 3)).copy()
    out['vramp'][..., 0] //= 2                                                                         # (channels that differ: the weights count)
    return out


def host(frames):
    return np.stack([frame_signature_host(f) for f in frames])


def launch(frames_dev, N, H, W):
    """One launch into a guarded, garbage-filled buffer -> int32 [N,256] on the host; the guards are checked."""
    buf = torch.full((GUARD + N * 256 + GUARD,), PATTERN, dtype=torch.int32, device='cuda')
    sig = buf[GUARD:GUARD + N * 256].view(N, 256)
    sig.fill_(GARBAGE)
    L.call(NAME, frames_dev, N, H, W, sig)
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == PATTERN).all()) and bool((buf[GUARD + N * 256:] == PATTERN).all())
    return sig.cpu().numpy()


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_kernel_equals_the_host_restatement_exactly(shape):
    N, H, W = shape
    for name, frames in contents(N, H, W).items():
        want = host(frames)
        assert (want.sum(axis=1) == H * W).all()
        # the frames as a view that starts 1 byte into a larger buffer: no alignment is asked of them
        raw = torch.zeros(N * H * W * 3 + 16, dtype=torch.uint8, device='cuda')
        view = raw[1:1 + N * H * W * 3].view(N, H, W, 3)
        view.copy_(torch.from_numpy(frames))
        assert view.data_ptr() % 2 == 1
        got = launch(view, N, H, W)
        assert got.dtype == np.int32 and np.array_equal(got, want), (name, shape)
        aligned = torch.from_numpy(frames).cuda()
        again = launch(aligned, N, H, W)
        assert np.array_equal(again, want), (name, shape, 'aligned')
        assert np.array_equal(launch(aligned, N, H, W), again)                       # two runs are identical


@pytest.mark.parametrize('shape', BANDED, ids=lambda s: 'x'.join(map(str, s[:3])))
def test_cells_cut_into_several_blocks_equal_the_host_restatement_exactly(shape):
    """Several blocks add to one counter, the last band of a cell is short and a band past a shorter cell's last row is empty: noise, the
    flat extremes, the bin boundaries and both ramps (the vertical one changes from band to band: a misplaced band shows)."""
    N, H, W, parts = shape
    assert bands(H, W) == parts and all(bands(h, w) == 1 for _, h, w in SHAPES) and bands(512, 512) == 1
    for name, frames in contents(N, H, W).items():
        want = host(frames)
        raw = torch.zeros(N * H * W * 3 + 16, dtype=torch.uint8, device='cuda')
        view = raw[3:3 + N * H * W * 3].view(N, H, W, 3)
        view.copy_(torch.from_numpy(frames))
        got = launch(view, N, H, W)
        assert np.array_equal(got, want), (name, shape)
        assert np.array_equal(launch(torch.from_numpy(frames).cuda(), N, H, W), want), (name, shape, 'aligned')
    # a frame whose every row is its own grey level: each band's counts land in their own bins
    rows = np.broadcast_to((np.arange(H) % 256).astype(np.uint8)[None, :, None, None], (N, H, W, 3)).copy()
    assert np.array_equal(launch(torch.from_numpy(rows).cuda(), N, H, W), host(rows))


def test_a_frames_counters_do_not_depend_on_its_batch():
    """Frames 0 .. 4 in one launch equal the launches of frames 0 .. 1 and 2 .. 4, and each frame alone."""
    N, H, W = 5, 130, 258
    frames = contents(N, H, W)['noise']
    dev = torch.from_numpy(frames).cuda()
    whole = launch(dev, N, H, W)
    assert np.array_equal(whole[:2], launch(dev[:2], 2, H, W)) and np.array_equal(whole[2:], launch(dev[2:], 3, H, W))
    for t in range(N):
        assert np.array_equal(whole[t:t + 1], launch(dev[t], 1, H, W)), t
    assert np.array_equal(whole, host(frames))


def test_refused_calls_launch_nothing():
    sig = torch.full((2, 256), GARBAGE, dtype=torch.int32, device='cuda')
    frames = torch.zeros((2, 4, 4, 3), dtype=torch.uint8, device='cuda')
    for args in ((frames, 0, 4, 4, sig), (frames, 2, 0, 4, sig), (frames, 2, 4, 32768, sig), (None, 2, 4, 4, sig), (frames, 2, 4, 4, None)):
        with pytest.raises(L.KeepHipError, match=NAME) as e:
            L.call(NAME, *args)
        assert e.value.code == L.EINVAL
    torch.cuda.synchronize()
    assert bool((sig == GARBAGE).all())
