"""Host tests of the carried clips (KEEP_AMD_TRACK_CARRY): which clip continues which (modules/clip_plan.py:plan_track_chains), the
order in which clips with predecessors run (engine/net.py:carry_schedule, ``run_clips(after=...)``) and the processor's knob.  No GPU:
the scheduler is driven through a stand-in net that records its calls."""
import numpy as np
import pytest
import torch

from comfyui_keep_amd.engine import net as N
from comfyui_keep_amd.engine.arch import DEFAULT_ARCH
from comfyui_keep_amd.modules.clip_plan import plan_track_chains, plan_track_clips


# ---- the plan -------------------------------------------------------------------------------------------------------------------
def test_one_track_of_five_frames_in_clips_of_two_is_one_chain():
    clips, slot_of, after = plan_track_chains([['A']] * 5, 2)
    assert clips == [[0, 1], [2, 3], [4]] and slot_of == list(range(5))
    assert after == [None, 0, 1]
    assert (clips, slot_of) == plan_track_clips([['A']] * 5, 2)                      # the existing return values stay


def test_a_gap_starts_a_new_run_and_nothing_is_carried_across_it():
    presence = [['A'], ['A'], ['A'], [], ['A'], ['A'], ['A']]
    clips, _, after = plan_track_chains(presence, 2)
    assert clips == [[0, 1], [2], [3, 4], [5]]
    assert after == [None, 0, None, 2]


def test_two_tracks_interleave_and_each_clip_continues_its_own_track():
    presence = [['A', 'B']] * 5
    clips, slot_of, after = plan_track_chains(presence, 2)
    assert clips == [[0, 2], [1, 3], [4, 6], [5, 7], [8], [9]]
    assert after == [None, None, 0, 1, 2, 3]
    assert (clips, slot_of) == plan_track_clips(presence, 2)
    # a track that appears late and one that leaves: runs of their own
    presence = [['A'], ['A', 'B'], ['A', 'B'], ['B'], ['A', 'B']]
    clips, _, after = plan_track_chains(presence, 2)
    for c, p in enumerate(after):
        if p is not None:
            assert p < c and len(clips[p]) == 2                                      # a predecessor is a FULL piece that ran earlier
    track_of = {}
    n = 0
    for t, keys in enumerate(presence):
        for k in keys:
            track_of[n] = (k, t)
            n += 1
    for c, p in enumerate(after):
        k0, t0 = track_of[clips[c][0]]
        if p is None:
            assert (k0, t0 - 1) not in track_of.values()                             # the start of a run: the track is not on the frame before
        else:
            assert track_of[clips[p][-1]] == (k0, t0 - 1)                            # same track, the frame before
    assert after.count(None) == 3                                                    # A's two runs and B's one


# ---- the schedule ----------------------------------------------------------------------------------------------------------------
def test_carry_schedule_orders_groups_by_readiness_and_first_clip():
    keys = [(2, 512, 512)] * 4 + [(1, 512, 512)] * 2
    after = [None, None, 0, 1, 2, 3]
    assert N.carry_schedule(keys, after, lambda k: 8) == [((2, 512, 512), False, [0, 1]), ((2, 512, 512), True, [2, 3]),
                                                          ((1, 512, 512), True, [4, 5])]
    assert N.carry_schedule(keys, after, lambda k: 1) == [
        ((2, 512, 512), False, [0]), ((2, 512, 512), False, [1]), ((2, 512, 512), True, [2]), ((2, 512, 512), True, [3]),
        ((1, 512, 512), True, [4]), ((1, 512, 512), True, [5])]
    with pytest.raises(ValueError):
        N.carry_schedule(keys[:2], [1, 0], lambda k: 8)                              # a cycle
    with pytest.raises(ValueError):
        N.carry_schedule(keys[:3], [None, 0, 0], lambda k: 8)                        # two successors of one clip
    with pytest.raises(ValueError):
        N.carry_schedule(keys[:2], [None, 5], lambda k: 8)


class _Recorder(N.KeepNet):
    """``run_clips`` of the engine over a net call that records (batch, T, carried, return_state) and returns marked tensors: the output
    is the input plus the number of clips in front of it in its chain, the state counts them."""

    def __init__(self, cap):
        super().__init__(**DEFAULT_ARCH)
        self.cap, self.calls = cap, []

    def clips_per_call(self, T, H=512, Wd=512):
        return self.cap

    def __call__(self, x, need_upscale=False, carry=None, return_state=False, **kw):
        B, T = x.shape[:2]
        depth = torch.zeros(B) if carry is None else carry.frame.view(B).clone()
        assert carry is None or carry.batch == B
        self.calls.append({'ids': [int(v) for v in x[:, 0, 0, 0, 0]], 'T': int(T), 'carried': carry is not None, 'state': bool(return_state),
                           'kw': {k: v for k, v in dict(kw, need_upscale=need_upscale).items()}})
        out = x + 1000.0 * depth.view(B, 1, 1, 1, 1)
        if not return_state:
            return out
        nxt = depth + 1
        return out, N.ClipState(nxt.view(B, 1, 1, 1), nxt.view(B, 1, 1, 1), {'16': nxt.view(B, 1, 1, 1)}, {'16': None})


def _clips(lengths):
    return [torch.full((1, T, 3, 2, 2), float(j)) for j, T in enumerate(lengths)]


def test_a_clip_never_runs_before_its_predecessor_and_groups_are_homogeneous():
    # three chains over 9 clips, lengths mixed: 2+2+1, 2+2, 3+1 (sorted the way the plan sorts: by first frame)
    lengths = [2, 2, 3, 2, 2, 1, 1, 1, 2]
    after = [None, None, None, 0, 1, 2, 3, None, 7]
    for cap in (1, 2, 8):
        net = _Recorder(cap)
        outs = net.run_clips(_clips(lengths), after=after)
        ran = []
        for call in net.calls:
            ids = call['ids']
            assert 1 <= len(ids) <= cap
            assert len({lengths[j] for j in ids}) == 1 and call['T'] == lengths[ids[0]]                # one length per call
            assert len({after[j] is not None for j in ids}) == 1 and call['carried'] == (after[ids[0]] is not None)   # carried or not
            assert all(after[j] is None or after[j] in ran for j in ids)                               # predecessors first
            assert call['state'] == any(j in after for j in ids)                                       # a state only where one is consumed
            ran += ids
        assert sorted(ran) == list(range(9))
        depth = {j: 0 for j in range(9)}
        for j in range(9):
            if after[j] is not None:
                depth[j] = depth[after[j]] + 1
        for j, o in enumerate(outs):
            assert o.shape == (1, lengths[j], 3, 2, 2) and float(o.flatten()[0]) == j + 1000.0 * depth[j]     # the RIGHT state reached it
        # of the ready groups the one with the earliest first clip runs first
        firsts = [c['ids'][0] for c in net.calls]
        if cap == 8:
            # (after [3, 4] the carried 1-frame clips 5 and 6 are both ready: one group; clip 7 starts a run: not with them)
            assert [c['ids'] for c in net.calls] == [[0, 1], [2], [3, 4], [5, 6], [7], [8]]
        assert firsts[0] == 0


def test_after_none_reproduces_todays_call_sequence_exactly():
    lengths = [2, 2, 3, 2, 1, 3]
    for after in (None, [None] * 6):
        net = _Recorder(2)
        outs = net.run_clips(_clips(lengths), after=after) if after is not None else net.run_clips(_clips(lengths))
        # today's order: by length in order of first appearance, cut at clips_per_call; no state asked for, no carried call
        assert [c['ids'] for c in net.calls] == [[0, 1], [3], [2, 5], [4]]
        assert all(not c['carried'] and not c['state'] and c['kw'] == {'need_upscale': False} for c in net.calls)
        assert all(float(o.flatten()[0]) == j for j, o in enumerate(outs))


def test_after_is_checked():
    net = _Recorder(2)
    with pytest.raises(ValueError):
        net.run_clips(_clips([2, 2]), after=[None])
    with pytest.raises(ValueError):
        net.run_clips(_clips([2, 2]), after=[None, 1])


def test_chains_do_not_cross_processes_one_warning(caplog):
    """With a worker pool the clips of a call do not all run here: ``after`` is ignored -- today's call sequence -- with ONE warning."""
    import logging
    net = _Recorder(2)
    net.pool = object()
    with caplog.at_level(logging.WARNING, logger='ComfyUI-KEEP'):
        for _ in range(2):
            net.calls.clear()
            outs = net.run_clips(_clips([2, 2, 1]), after=[None, 0, 1])
            assert [c['ids'] for c in net.calls] == [[0, 1], [2]] and not any(c['carried'] or c['state'] for c in net.calls)
            assert all(float(o.flatten()[0]) == j for j, o in enumerate(outs))
    assert len([r for r in caplog.records if 'carried clips' in r.getMessage()]) == 1
    net.pool = None                                                                  # (not a real pool: nothing to close)


def test_chains_do_not_cross_ranks_one_warning(caplog, monkeypatch):
    """Inside a torch.distributed job of more than one rank the clips are sharded over the ranks: ``after`` is ignored, one warning;
    with ``shard_across_ranks`` off every rank restores its own list and the chains hold."""
    import logging
    for fn, val in (('is_available', True), ('is_initialized', True), ('get_world_size', 2)):
        monkeypatch.setattr(torch.distributed, fn, lambda *a, _v=val, **k: _v)
    net = _Recorder(2)
    with caplog.at_level(logging.WARNING, logger='ComfyUI-KEEP'):
        for _ in range(2):
            assert net._chains_apply([None, 0, 1], 3) is None
    assert len([r for r in caplog.records if 'carried clips' in r.getMessage()]) == 1
    net.shard_across_ranks = False
    assert net._chains_apply([None, 0, 1], 3) == [None, 0, 1]
    monkeypatch.setattr(torch.distributed, 'get_world_size', lambda *a, **k: 1)
    net.shard_across_ranks = True
    assert net._chains_apply([None, 0, 1], 3) == [None, 0, 1]


def test_clip_state_select_and_cat_regroup_clips():
    B = 3
    mk = lambda c: torch.arange(B * c, dtype=torch.float32).view(B, c)      # noqa: E731
    st = N.ClipState(mk(2), mk(3), {'16': mk(4), '32': mk(5)}, {'16': torch.arange(B, dtype=torch.float32), '32': None})
    assert st.batch == 3
    parts = [st.select([k]) for k in range(B)]
    assert all(p.batch == 1 and p.cross_amax['32'] is None for p in parts)
    back = N.ClipState.cat([parts[2], parts[0], parts[1]])
    assert torch.equal(back.frame, st.frame[[2, 0, 1]]) and torch.equal(back.prev_out, st.prev_out[[2, 0, 1]])
    assert torch.equal(back.cross_prev['32'], st.cross_prev['32'][[2, 0, 1]]) and torch.equal(back.cross_amax['16'], torch.tensor([2., 0., 1.]))
    assert back.cross_amax['32'] is None
    two = st.select(slice(1, 3))
    assert two.batch == 2 and torch.equal(two.cross_prev['16'], st.cross_prev['16'][1:3])
    two.frame.zero_()
    assert st.frame[1:].abs().sum() > 0                                               # a selection owns its tensors


# ---- the processor's knob --------------------------------------------------------------------------------------------------------
def test_knob_is_off_by_default_implies_track_clips_and_hands_the_chains_to_a_net_that_takes_them(monkeypatch):
    import test_host_logic as H   # installs the ComfyUI stubs
    from comfyui_keep_amd.modules.keep_model_loader import KEEPModelPack
    from comfyui_keep_amd.modules.keep_processor import KEEPFaceProcessor

    class Net:
        supports_single_frame = True

        def __init__(self):
            self.seen = []

        def run_clips_u8(self, clips, max_b=None, after=None):
            self.seen.append(([len(c) for c in clips], after))
            return [torch.from_numpy(np.stack([np.asarray(f) for f in c])) for c in clips]

    class NoT1Net(Net):
        supports_single_frame = False

    class OldNet(Net):
        def run_clips_u8(self, clips, max_b=None):
            return Net.run_clips_u8(self, clips, max_b, 'not asked')

    monkeypatch.delenv('KEEP_AMD_TRACK_CARRY', raising=False)
    crops = [np.full((512, 512, 3), i, np.uint8) for i in range(5)]
    for cls in (Net, OldNet):
        net = cls()
        proc = KEEPFaceProcessor(KEEPModelPack(net, H._Helper(), None, None, 'KEEP'))
        assert proc.track_carry is False and proc._per_track is False
        plan = proc._track_plan([['A']] * 5, 2)
        assert len(plan) == 2
        proc._restore_crops_u8(crops, 2, members=plan[0])
        proc.track_carry = True
        assert proc._per_track is True
        plan = proc._track_plan([['A']] * 5, 2)
        assert plan == ([[0, 1], [2, 3], [4]], list(range(5)), [None, 0, 1])
        got = proc._restore_crops_u8(crops, 2, members=plan[0], after=plan[2])
        assert all(np.array_equal(a, b) for a, b in zip(got, crops))
        if cls is Net:
            assert net.seen == [([2, 2, 1], None), ([2, 2, 1], [None, 0, 1])]
        else:
            assert net.seen == [([2, 2, 1], 'not asked')] * 2                        # a net without the argument: restored, nothing carried
    # a net without the single-frame path: lone clips are doubled on the host, except where it is handed ``after`` -- the duplicate rule
    # is then the net's, so that the state it hands on is the one after frame 0
    net = NoT1Net()
    proc = KEEPFaceProcessor(KEEPModelPack(net, H._Helper(), None, None, 'KEEP'))
    proc._restore_crops_u8(crops, 2, members=[[0, 1], [2, 3], [4]])
    proc.track_carry = True
    proc._restore_crops_u8(crops, 2, members=[[0, 1], [2, 3], [4]], after=[None, 0, 1])
    assert net.seen == [([2, 2, 2], None), ([2, 2, 1], [None, 0, 1])]
    monkeypatch.setenv('KEEP_AMD_TRACK_CARRY', '1')
    assert KEEPFaceProcessor(KEEPModelPack(Net(), H._Helper(), None, None, 'KEEP')).track_carry is True
