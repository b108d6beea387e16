"""Scene cuts (``KEEP_AMD_SCENE_CUTS``): where a video changes scene, so that tracking, smoothing and the carried state stop there.

Pure numpy: no torch, no GPU.  A frame's SIGNATURE is a 4 x 4 grid of 16-bin luma histograms in integer arithmetic:

    Y = (29 * B + 150 * G + 77 * R + 128) >> 8        (the weights sum to 256: Y <= 255)
    bin = Y >> 4,   cell = ((y * 4) // H) * 4 + (x * 4) // W,   sig[cell * 16 + bin] counts the pixels

``frame_signature_host`` is that arithmetic on the host; ``keep_frame_signature_u8`` (csrc/keep_signature.hip) is the same on the device
and equals it bit for bit, so where a signature is computed cannot change a result.  Two consecutive frames whose signatures are at
least ``threshold`` apart -- half the L1 distance over the pixel count, a value in [0, 1] -- are a hard cut.  Dissolves, fades and flashes
are not looked for.
"""
import numpy as np

GRID, BINS = 4, 16
SIG_LEN = GRID * GRID * BINS
DEFAULT_THRESHOLD = 0.4     # a setting, not a measured optimum


def _cell_index(n):
    """(i * 4) // n for i in 0 .. n - 1: the cell row (column) of every pixel row (column)."""
    return (np.arange(n, dtype=np.int64) * GRID) // n


def frame_signature_host(frame_bgr):
    """uint8 BGR [H,W,3] -> int32 [256]: the frame's signature; the counters sum to H * W."""
    f = np.asarray(frame_bgr)
    if f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3 or f.shape[0] < 1 or f.shape[1] < 1:
        raise ValueError(f"frame_signature_host: a uint8 [H,W,3] frame, got {f.dtype} {tuple(f.shape)}")
    h, w = f.shape[:2]
    c = f.astype(np.int32)
    y = (29 * c[..., 0] + 150 * c[..., 1] + 77 * c[..., 2] + 128) >> 8
    idx = ((_cell_index(h)[:, None] * GRID + _cell_index(w)[None, :]) * BINS + (y >> 4)).reshape(-1)
    return np.bincount(idx, minlength=SIG_LEN).astype(np.int32)


def signature_distance(a, b, hw):
    """sum |a - b| / (2 * hw): 0 for equal signatures, 1 when no counter is shared."""
    d = np.abs(np.asarray(a, np.int64) - np.asarray(b, np.int64)).sum()
    return float(d) / (2.0 * float(hw))


def signature_distances(sigs, hw):
    """float64 [n - 1]: the distance of every frame t >= 1 to frame t - 1."""
    s = np.asarray(sigs, np.int64).reshape(-1, SIG_LEN)
    if s.shape[0] < 2:
        return np.zeros((0,), np.float64)
    return np.abs(s[1:] - s[:-1]).sum(axis=1).astype(np.float64) / (2.0 * float(hw))


def find_cuts(sigs, hw, threshold=DEFAULT_THRESHOLD):
    """The sorted frames t >= 1 that open a scene: ``signature_distance(sigs[t - 1], sigs[t], hw) >= threshold``."""
    return [int(t) + 1 for t in np.nonzero(signature_distances(sigs, hw) >= threshold)[0]]


def segments(n_frames, cuts):
    """[(a, b)]: the scenes of ``n_frames`` frames as half-open frame spans; ``cuts`` outside 1 .. n_frames - 1 are ignored."""
    n = int(n_frames)
    if n <= 0:
        return []
    edges = [0] + sorted({int(t) for t in (cuts or ()) if 0 < int(t) < n}) + [n]
    return list(zip(edges[:-1], edges[1:]))
