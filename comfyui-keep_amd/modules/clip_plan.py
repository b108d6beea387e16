"""Track clips (``KEEP_AMD_TRACK_CLIPS``): which crops of a multi-face sequence form a clip when every clip holds consecutive frames of ONE
track, instead of the reference's cut of the flat frame-major crop list (keep_processor.py:263-264 of the reference).

Pure: no torch, no GPU.  Crop numbering is the processor's frame-major one -- crop ``first[t] + j`` is face j of frame t -- so everything
that is indexed by crop (restored faces, class maps, affines, the paste order) stays as it is; only the grouping into clips changes.
"""


def plan_track_clips(presence, max_clip_length):
    """``presence[t]``: the keys of the tracks active at frame t, in face order -> ``(clips, slot_of)``.

    * A track's RUN is a maximal stretch of consecutive frames on which it is present: a gap starts a new run, so the net's recurrence
      never bridges frames that are not adjacent.
    * Every run is cut into PIECES of at most ``max_clip_length`` frames, full pieces first (the rule ``split_clips`` applies to the flat
      list).  A piece is a clip.
    * ``clips``: one list of crop indices per clip, in frame order, the clips sorted by their first frame and then by the order in which
      their tracks first appeared.  The engine runs clips in list order and the paste-back emits a frame once all its faces are restored:
      this order makes the early frames complete first (track after track would hold frame 0 back until the last track's first clip).
    * ``slot_of[i]``: a permutation of the crop indices under which the members of every clip occupy consecutive, increasing slots, clip
      after clip: a crop tensor laid out by slot has every clip as a contiguous view.

    One track present on every frame gives the spans of ``split_clips`` and the identity permutation."""
    clips, slot_of, _ = plan_track_chains(presence, max_clip_length)
    return clips, slot_of


def plan_track_chains(presence, max_clip_length):
    """``plan_track_clips`` plus, per clip, the clip it continues (``KEEP_AMD_TRACK_CARRY``) -> ``(clips, slot_of, after)``.

    ``after[c]``: the index in ``clips`` of the previous piece of the same run of the same track -- the clip whose last frame is the frame
    before clip c's first -- or None where clip c starts a run.  A gap in a track starts a new run, so no state is carried across it."""
    L = int(max_clip_length)
    if L < 1:
        raise ValueError(f"plan_track_clips: max_clip_length {max_clip_length} < 1")
    rank, runs, open_run = {}, [], {}        # track key -> order of first appearance; finished runs; key -> the run that reaches frame t - 1
    n_crops = 0
    for t, keys in enumerate(presence):
        keys = list(keys)
        if len(set(keys)) != len(keys):
            raise ValueError(f"plan_track_clips: a track is named twice at frame {t}")
        still = {}
        for j, key in enumerate(keys):
            rank.setdefault(key, len(rank))
            run = open_run.get(key)
            if run is None:
                run = (t, rank[key], [])
                runs.append(run)
            run[2].append(n_crops + j)
            still[key] = run
        open_run = still
        n_crops += len(keys)
    pieces = []
    for n_run, (t0, r, members) in enumerate(runs):
        for s in range(0, len(members), L):
            pieces.append((t0 + s, r, members[s:s + L], (n_run, s // L)))
    pieces.sort(key=lambda p: (p[0], p[1]))
    clips = [m for _, _, m, _ in pieces]
    where = {pid: c for c, (_, _, _, pid) in enumerate(pieces)}
    after = [where.get((n_run, k - 1)) for _, _, _, (n_run, k) in pieces]
    slot_of = [None] * n_crops
    slot = 0
    for m in clips:
        for i in m:
            slot_of[i] = slot
            slot += 1
    return clips, slot_of, after


def clip_slot_spans(clips):
    """[(s0, s1)] of every clip in a tensor laid out by ``slot_of``: clip c is ``tensor[s0:s1]``."""
    spans, s = [], 0
    for m in clips:
        spans.append((s, s + len(m)))
        s += len(m)
    return spans
