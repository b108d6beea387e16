"""The frame containers of ``keep_processor.py``: the node's IMAGE batch as uint8 BGR frames converted on the device
(``frames_from_comfy``, ``_ConvertedFrames``) and the frames of a detected sequence resident on the device from the detection pre-pass
to the paste-back (``frame_store_plan``, ``_FrameStore``).  Nothing here refers to the processor.
"""
import logging
import os

import numpy as np
import torch

from .utils import comfy_image_to_cv2

log = logging.getLogger('ComfyUI-KEEP')

_PINNED_U8 = {}      # one cached pinned frame buffer per shape (hipHostMalloc of 0.8 GB costs ~0.1 s; frames never outlive the node call)


def cuda_device(device):
    """``torch.device(device)`` with its index named: a bare 'cuda' is the current device."""
    dev = torch.device(device)
    return torch.device('cuda', torch.cuda.current_device()) if dev.index is None else dev


class _ConvertedFrames:
    """The node's IMAGE batch as uint8 BGR frames -- ``comfy_image_to_cv2`` (utils.py:155-160) for the whole sequence, on the device
    (``keep_comfy_to_bgr_u8``: x * 255 in float32, truncating cast, RGB -> BGR) instead of three numpy passes per frame on one host
    core: a worker thread uploads the float frames in chunks (pageable -> device), converts them and downloads the uint8 frames into
    ONE pinned buffer; ``frames[i]`` / ``frames[a:b]`` wait only for the chunks they touch, so the detection pre-pass of the first
    frames runs under the conversion of the rest.  Items are numpy views of the pinned buffer (what the helper and cv2 take)."""

    def __init__(self, seq, device, chunk_bytes=128 << 20):
        import threading
        self.n, self.H, self.W = int(seq.shape[0]), int(seq.shape[1]), int(seq.shape[2])
        self._seq, self._dev = seq, device
        per = self.H * self.W * 3
        self._chunk = max(1, min(self.n, chunk_bytes // (per * 4)))
        self._nchunks = -(-self.n // self._chunk)
        self._done = [threading.Event() for _ in range(self._nchunks)]
        self._ready = threading.Event()          # the pinned buffer exists
        self._err = None
        self._arr = None
        self._thread = threading.Thread(target=self._run, name='keep-comfy-convert', daemon=True)
        self._thread.start()

    def _run(self):
        try:
            from ..engine import hiplib as L
            shape = (self.n, self.H, self.W, 3)
            buf = _PINNED_U8.get(shape)
            if buf is None:
                _PINNED_U8.clear()
                try:
                    buf = torch.empty(shape, dtype=torch.uint8, pin_memory=True)
                    _PINNED_U8[shape] = buf
                except RuntimeError:                                  # more than the host will pin
                    buf = torch.empty(shape, dtype=torch.uint8)
            self._buf, self._arr = buf, buf.numpy()
            self._ready.set()
            with torch.cuda.device(self._dev):
                st = torch.cuda.Stream(device=self._dev)
                pend = None
                with torch.cuda.stream(st):
                    for c in range(self._nchunks):
                        a, b = c * self._chunk, min(self.n, (c + 1) * self._chunk)
                        src = self._seq[a:b]
                        if not src.is_contiguous():
                            src = src.contiguous()
                        d = src.to(self._dev, non_blocking=True)      # (a pageable source: the call returns when the chunk is staged)
                        u = torch.empty((b - a, self.H, self.W, 3), dtype=torch.uint8, device=self._dev)
                        L.call('keep_comfy_to_bgr_u8', d, u, (b - a) * self.H * self.W)
                        buf[a:b].copy_(u, non_blocking=True)
                        ev = torch.cuda.Event()
                        ev.record(st)
                        if pend is not None:                           # chunk c - 1 finished under this chunk's upload
                            pend[1].synchronize()
                            self._done[pend[0]].set()
                        pend = (c, ev)
                    pend[1].synchronize()
                    self._done[pend[0]].set()
        except BaseException as e:                                     # (out of memory, a lost device ...): the host converter, loudly
            log.warning("device-side IMAGE conversion failed (%s); converting on the host", e)
            try:
                self._arr = np.stack([comfy_image_to_cv2(self._seq[i].unsqueeze(0)) for i in range(self.n)])
            except BaseException as e2:                                # surfaced by the first access
                self._err = e2
            self._ready.set()
            for d in self._done:
                d.set()

    def _wait(self, a, b):
        self._ready.wait()
        for c in range(a // self._chunk, min(self._nchunks, -(-b // self._chunk))):
            self._done[c].wait()
        if self._err is not None:
            raise self._err

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        if isinstance(i, slice):
            a, b, step = i.indices(self.n)
            if step != 1:
                return [self[j] for j in range(a, b, step)]
            if b <= a:
                return []
            self._wait(a, b)
            return [self._arr[j] for j in range(a, b)]
        if i < 0:
            i += self.n
        if not 0 <= i < self.n:
            raise IndexError(i)
        self._wait(i, i + 1)
        return self._arr[i]

    def __iter__(self):
        return (self[i] for i in range(self.n))


def frames_from_comfy(seq, device):
    """IMAGE batch [N,H,W,3] float32 (host or device) -> N uint8 BGR frames.  On the device when there is one and the library loads
    (``_ConvertedFrames``); ``KEEP_AMD_DEVICE_CONVERT=0``, another dtype / layout, or no GPU: the per-frame host converter."""
    dev = torch.device(device)
    if (os.environ.get('KEEP_AMD_DEVICE_CONVERT', '1') != '0' and dev.type == 'cuda' and torch.cuda.is_available()
            and isinstance(seq, torch.Tensor) and seq.dtype == torch.float32 and seq.dim() == 4 and seq.shape[-1] == 3
            and seq.shape[0] > 0 and seq.shape[1] > 0 and seq.shape[2] > 0):
        try:
            from ..engine import hiplib as L
            L.load()
            return _ConvertedFrames(seq, cuda_device(dev))
        except Exception:
            pass
    return [comfy_image_to_cv2(seq[i].unsqueeze(0)) for i in range(seq.shape[0])]


def uniform_u8_frames(frames):
    """(h, w) where the frames (at least one) are uint8 [h,w,3] host arrays of ONE size, else None."""
    if isinstance(frames, _ConvertedFrames):            # uint8 [H,W,3] by construction (asking a frame would wait for its conversion)
        return frames.H, frames.W
    shape = tuple(getattr(frames[0], 'shape', ()))
    if len(shape) != 3 or shape[2] != 3:
        return None
    if any(not isinstance(f, np.ndarray) or f.dtype != np.uint8 or tuple(f.shape) != shape for f in frames):
        return None
    return shape[:2]


FRAME_STORE_DEFAULT_GB = 16.0     # KEEP_AMD_FRAME_STORE_GB: a policy (the store must not crowd out the clip batches sized from free HBM), not a measurement


def frame_store_plan(frames, cap_bytes, chunk):
    """The chunk spans [(start, stop)] of a device-resident frame store over ``frames``, or None where there is none: an empty
    sequence, frames that are not uint8 [H,W,3] host arrays of ONE size, or more than ``cap_bytes`` in all (n * H * W * 3; exactly the cap
    still applies).  A sequence over the cap takes the present path entirely: no partial stores.  ``chunk``: frames per chunk (the
    detector's batch axis); the spans cover 0 .. n without overlap.  Pure: needs no device."""
    n = len(frames)
    if n == 0 or chunk < 1:
        return None
    hw = uniform_u8_frames(frames)
    if hw is None or hw[0] <= 0 or hw[1] <= 0 or n * hw[0] * hw[1] * 3 > cap_bytes:
        return None
    return [(s, min(s + chunk, n)) for s in range(0, n, chunk)]


class _FrameStore:
    """The frames of one detected sequence on the device, one uint8 [m,H,W,3] tensor per chunk of the detection pre-pass, from the
    pre-pass (which fills it and detects on it) over the crop warp to the paste-back (which reads the backgrounds from it).  Every
    fill is followed by an event on the filling stream; a stream other than that one waits for it before its first read of the
    chunk (``frame``).  A chunk is let go once its last frame has been emitted (``release``): the caching allocator is told which
    stream read it last, so the memory is not handed out again before that stream has passed the read.

    Small frames (``small = (f, H2, W2)``, set by the pre-pass when ``read_image`` enlarges the first frame): a chunk is kept twice, the
    original frames (``bufs``: the paste-back's backgrounds) and their enlargement (``ebufs``, ``enlarge``: the detector batch and what the
    crop warp reads, let go after that warp)."""

    def __init__(self, spans, h, w, device, cap_bytes=None):
        self.spans, self.h, self.w, self.device = list(spans), int(h), int(w), device
        self.cap_bytes = cap_bytes
        self.small = None
        self.sig = None                   # scene cuts: int32 [n_frames,256] on the device, row t the signature of frame t (``fill`` writes it)
        self.ebufs = [None] * len(self.spans)
        self.chunk = self.spans[0][1] - self.spans[0][0]
        self.bufs = [None] * len(self.spans)
        self.events = [None] * len(self.spans)
        self._waited = [False] * len(self.spans)
        self.dead = False                 # a frame ``read_image`` changed, or a failure: the sequence takes the present path

    def fill(self, k, frames):
        a, b = self.spans[k]
        if len(frames) != b - a:
            raise ValueError(f"frame store: chunk {k} holds frames {a} .. {b - 1}, got {len(frames)}")
        with torch.cuda.device(self.device):
            buf = torch.empty((b - a, self.h, self.w, 3), dtype=torch.uint8, device=self.device)
            for i, fr in enumerate(frames):
                buf[i].copy_(torch.from_numpy(np.ascontiguousarray(fr)), non_blocking=True)
            if self.sig is not None:      # the chunk's signatures: one launch behind its copies, on the frames as they came
                try:
                    from ..engine import hiplib as L
                    L.call('keep_frame_signature_u8', buf, b - a, self.h, self.w, self.sig[a:b])
                except Exception as e:    # the opt-in mode's trouble is not the store's: logged, and the host function takes the signatures
                    log.warning("frame signatures on the device failed (%s): the host function", e)
                    self.sig = None
            ev = torch.cuda.Event()
            ev.record()
        self.bufs[k], self.events[k] = buf, ev
        return buf

    def enlarge(self, k, resizer):
        """Chunk k's frames through ``read_image``'s enlargement: one launch on the current stream, behind the fill."""
        f = self.small[0]
        with torch.cuda.device(self.device):
            ebuf = resizer.enlarge_u8(self.bufs[k], f, f)
            ev = torch.cuda.Event()
            ev.record()
        self.ebufs[k], self.events[k] = ebuf, ev
        return ebuf

    def warp_source(self, k):
        """What the crop warp of chunk k reads: the frames the landmarks live in."""
        return self.bufs[k] if self.small is None else self.ebufs[k]

    def complete(self):
        return all(b is not None for b in self.bufs)

    def frame(self, t, stream):
        """Frame t, uint8 [H,W,3], for work queued on ``stream`` (which waits for the chunk's fill first)."""
        k = t // self.chunk
        if not self._waited[k]:
            stream.wait_event(self.events[k])
            self._waited[k] = True
        return self.bufs[k][t - self.spans[k][0]]

    def release(self, k, stream=None):
        buf = self.bufs[k]
        if buf is not None and stream is not None:
            buf.record_stream(stream)
        self.bufs[k] = self.ebufs[k] = None             # (the enlarged chunk is read on the stream that made it)

    def drop(self, stream=None):
        for k in range(len(self.spans)):
            self.release(k, stream)
