"""Landmark tracking + temporal smoothing that precede the crop step (CPU pre-processing;
restates reference ``modules/keep_processor.py:33-115`` and ``:216-231``).

Semantics kept: a track is a list of one ``[5,2]`` landmark array per frame, missing frames
are NaN; association is Hungarian assignment on landmark-centroid distance with a hard
threshold (75 px); gaps are linearly interpolated per coordinate and the result is smoothed
with ``gaussian_filter1d(sigma=2)`` along time.

Track lifetimes (KEEP_AMD_TRACK_LIFETIMES, off by default; ``lifetimes=max_gap``): the reference's interpolation holds a track's end values
over the whole video, so a face seen on 10 frames is restored on all of them, and a single detector miss ends a track and starts a
duplicate.  With the keyword the raw tracks are stitched over short gaps and a track is NaN outside its first .. last detection.
"""
import numpy as np
from scipy.ndimage import gaussian_filter1d
from scipy.optimize import linear_sum_assignment

_NAN_LM = lambda: np.full((5, 2), np.nan)  # noqa: E731


def interpolate_sequence(seq):
    """Fill NaNs of a 1-D series by linear interpolation over the valid samples (KP:33-40)."""
    out = np.copy(seq)
    missing = np.isnan(seq)
    if missing.any():
        x = np.arange(len(seq))
        out[missing] = np.interp(x[missing], x[~missing], seq[~missing])
    return out


def track_faces(all_frames_landmarks, distance_threshold=75.0):
    """dict track_id -> list (one entry per frame) of [5,2] arrays, NaN where unseen (KP:42-115)."""
    n_frames = len(all_frames_landmarks)
    tracks, next_id = {}, 0
    if all_frames_landmarks and all_frames_landmarks[0]:
        for lm in all_frames_landmarks[0]:
            tracks[next_id] = [lm]
            next_id += 1

    for i in range(1, n_frames):
        for data in tracks.values():                       # pad tracks that skipped frame i-1
            if len(data) < i:
                data.append(_NAN_LM())
        active = [(tid, data[-1]) for tid, data in tracks.items()
                  if len(data) == i and not np.all(np.isnan(data[-1]))]
        current = all_frames_landmarks[i]
        matched = set()
        if active and current:
            cost = np.full((len(active), len(current)), np.inf)
            for r, (_, prev) in enumerate(active):
                for c, cur in enumerate(current):
                    d = np.linalg.norm(prev.mean(axis=0) - cur.mean(axis=0))
                    if d < distance_threshold:
                        cost[r, c] = d
            if not np.all(np.isinf(cost)):
                rows, cols = linear_sum_assignment(cost)
                for r, c in zip(rows, cols):
                    if cost[r, c] != np.inf:
                        tracks[active[r][0]].append(current[c])
                        matched.add(c)
        for tid, _ in active:                              # active but unmatched this frame
            if len(tracks[tid]) == i:
                tracks[tid].append(_NAN_LM())
        for c in set(range(len(current))) - matched:      # new faces start new tracks
            tracks[next_id] = [_NAN_LM()] * i + [current[c]]
            next_id += 1

    for data in tracks.values():
        while len(data) < n_frames:
            data.append(_NAN_LM())
    return tracks


def _smooth(landmark_seq):
    """[N,10] with NaN gaps -> interpolated + gaussian(sigma=2) -> [N,5,2]."""
    arr = np.array(landmark_seq, dtype=np.float64)
    for j in range(arr.shape[1]):
        arr[:, j] = interpolate_sequence(arr[:, j])
    return gaussian_filter1d(arr, sigma=2, axis=0).reshape(arr.shape[0], 5, 2)


def _per_segment(smooth, raw_landmarks_per_frame, cuts, **kw):
    """``smooth`` over every scene of the video on its own, exactly as if the scene were the whole video (scene_cuts.py:segments): the
    tracks of scene s come back under the keys ``(s, key)``, NaN outside the scene.  A scene without any detection yields no track -- its
    frames pass through unrestored; the whole-video interpolation would carry a neighbouring scene's landmarks into it.  ``kw``: what
    ``smooth`` takes besides (``lifetimes``; ``report`` comes back with the scene's keys and the video's frame numbers)."""
    from .scene_cuts import segments
    n = len(raw_landmarks_per_frame)
    report = kw.pop('report', None)
    out = {}
    for s, (a, b) in enumerate(segments(n, cuts)):
        part = raw_landmarks_per_frame[a:b]
        if not any(part):
            continue
        sub = [] if report is not None else None
        if sub is not None:
            kw['report'] = sub
        for key, seq in smooth(part, **kw).items():
            full = np.full((n, 5, 2), np.nan)
            full[a:b] = seq
            out[(s, key)] = full
        if sub is not None:
            report.extend(((s, key), a + first, a + last, count) for key, first, last, count in sub)
    return out


# ---- track lifetimes (KEEP_AMD_TRACK_LIFETIMES): a track exists from its first to its last detection ---------------------------------
def _detected(lm):
    return not np.all(np.isnan(lm))


def stitch_tracks(raw_tracks, max_gap, distance_threshold=75.0):
    """The raw tracks of ``track_faces`` -- each ONE contiguous run of detections [s, e]: a track dies at its first miss -- joined into
    chains over detector dropouts -> list of chains, each the list of its raw track ids in time order; a chain's id is its index.

    The raw tracks are taken in order of s, ties by track id.  Track r continues chain c when 1 <= s_r - e_c - 1 <= ``max_gap`` (e_c: the
    chain's last detection so far) and the centroids of c's last and r's first landmarks are less than ``distance_threshold`` apart (the
    tracker's own measure and threshold).  Among several such chains r joins the nearest, ties by lowest chain id; otherwise r starts a
    chain.  ``max_gap`` = 0 stitches nothing.  A chain's members never overlap in time: r joins only behind the chain's last detection."""
    runs = []
    for tid, lms in raw_tracks.items():
        seen = [t for t, lm in enumerate(lms) if _detected(lm)]
        if seen:
            runs.append((seen[0], tid, seen[-1]))
    chains, ends = [], []                   # ends[c]: (frame of the chain's last detection, centroid of its landmarks there)
    for s, tid, e in sorted(runs, key=lambda r: (r[0], r[1])):
        lms = raw_tracks[tid]
        start = np.asarray(lms[s], np.float64).mean(axis=0)
        best, best_d = None, None
        for c, (e_c, centroid) in enumerate(ends):
            if not 1 <= s - e_c - 1 <= max_gap:
                continue
            d = float(np.linalg.norm(centroid - start))
            if d < distance_threshold and (best is None or d < best_d):
                best, best_d = c, d
        end = (e, np.asarray(lms[e], np.float64).mean(axis=0))
        if best is None:
            chains.append([tid])
            ends.append(end)
        else:
            chains[best].append(tid)
            ends[best] = end
    return chains


def _lifetime(seq, n):
    """[n,10] with NaN rows where nothing was detected -> ([n,5,2]: ``_smooth`` of the rows from the first to the last detection ALONE, as
    if they were the whole video, NaN outside; first frame; last frame; number of detections)."""
    seen = np.flatnonzero(~np.isnan(seq).all(axis=1))
    a, b = int(seen[0]), int(seen[-1])
    full = np.full((n, 5, 2), np.nan)
    full[a:b + 1] = _smooth(seq[a:b + 1])
    return full, a, b, int(seen.size)


def fade_weights(n_frames, lifetimes, fade, cuts=None):
    """The paste weight of every track on every frame (KEEP_AMD_TRACK_FADE = ``fade`` frames): ``lifetimes`` as the smoothers report
    them, (key, first a, last b, n_detections) -> {key: float32 [n_frames]}, 0 outside [a, b] and

        min(1, (t - a + 1) / (fade + 1), (b - t + 1) / (fade + 1))

    inside, in float64, then cast.  The first ramp is dropped when a opens the video or a scene (``cuts``: the frames that open one), the
    second when b closes one: a face that is there from the start does not fade in.  ``fade`` = 0: 1.0 on every live frame."""
    opens = {0} | {int(c) for c in (cuts or ())}
    closes = {n_frames - 1} | {int(c) - 1 for c in (cuts or ())}
    R = max(0, int(fade))
    out = {}
    for key, a, b, _ in lifetimes:
        t = np.arange(a, b + 1, dtype=np.float64)
        w = np.ones(b - a + 1, np.float64)
        if a not in opens:
            w = np.minimum(w, (t - a + 1) / (R + 1))
        if b not in closes:
            w = np.minimum(w, (b - t + 1) / (R + 1))
        full = np.zeros(n_frames, np.float32)
        full[a:b + 1] = w.astype(np.float32)
        out[key] = full
    return out


def smooth_center_face(raw_landmarks_per_frame, cuts=None, lifetimes=None, report=None):
    """only_center_face: at most one face per frame, no association needed (KP:216-222).  ``cuts`` (KEEP_AMD_SCENE_CUTS): the frames
    that open a scene; every scene is smoothed on its own (``_per_segment``).  None / empty: the video is one scene, today's result.

    ``lifetimes`` (KEEP_AMD_TRACK_LIFETIMES: the largest gap in frames, ``max_gap``; None: today's result): the sequence is split where
    more than ``max_gap`` consecutive frames have no detection; every piece is a track of its own (keys 0, 1, ... in time order) that
    lives from its first to its last detection (``_lifetime``) and is NaN elsewhere.  ``report``: a list that receives one
    (key, first_frame, last_frame, n_detections) per lifetime."""
    kw = {} if lifetimes is None else {'lifetimes': lifetimes, 'report': report}
    if cuts:
        return _per_segment(smooth_center_face, raw_landmarks_per_frame, cuts, **kw)
    seq = [(f[0] if f else _NAN_LM()).reshape(10) for f in raw_landmarks_per_frame]
    if lifetimes is None:
        return {0: _smooth(seq)}
    n = len(seq)
    arr = np.array(seq, dtype=np.float64).reshape(n, 10)
    pieces, prev = [], None
    for t in (t for t, f in enumerate(raw_landmarks_per_frame) if f):
        if prev is None or t - prev - 1 > lifetimes:
            pieces.append([t, t])
        pieces[-1][1] = prev = t
    out = {}
    for key, (a, b) in enumerate(pieces):
        part = np.full((n, 10), np.nan)
        part[a:b + 1] = arr[a:b + 1]
        out[key], first, last, count = _lifetime(part, n)
        if report is not None:
            report.append((key, first, last, count))
    return out


def smooth_tracked_faces(raw_landmarks_per_frame, cuts=None, lifetimes=None, report=None):
    """multi-face: Hungarian tracks, each smoothed independently (KP:223-231).  ``cuts``: as in ``smooth_center_face`` -- every scene is
    tracked and smoothed on its own, so no track crosses a cut.

    ``lifetimes`` (``max_gap``; None: today's result): the raw tracks are stitched over gaps of at most ``max_gap`` frames
    (``stitch_tracks``); every chain is one track under its chain id, alive from its first to its last detection (``_lifetime``: interior
    gaps are interpolated as today, the smoothing sees the lifetime alone) and NaN elsewhere.  ``report``: as in ``smooth_center_face``."""
    kw = {} if lifetimes is None else {'lifetimes': lifetimes, 'report': report}
    if cuts:
        return _per_segment(smooth_tracked_faces, raw_landmarks_per_frame, cuts, **kw)
    out = {}
    if not any(raw_landmarks_per_frame):
        return out
    raw_tracks = track_faces(raw_landmarks_per_frame)
    if lifetimes is None:
        for tid, lms in raw_tracks.items():
            seq = [lm.reshape(10) if not np.all(np.isnan(lm)) else np.full(10, np.nan) for lm in lms]
            out[tid] = _smooth(seq)
        return out
    n = len(raw_landmarks_per_frame)
    for cid, members in enumerate(stitch_tracks(raw_tracks, lifetimes)):
        seq = np.full((n, 10), np.nan)
        for tid in members:
            for t, lm in enumerate(raw_tracks[tid]):
                if _detected(lm):
                    seq[t] = np.asarray(lm, np.float64).reshape(10)
        out[cid], first, last, count = _lifetime(seq, n)
        if report is not None:
            report.append((cid, first, last, count))
    return out
