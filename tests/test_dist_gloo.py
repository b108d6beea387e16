"""CPU suite: the N>1 path on gloo, world_size 2 -- weight-blob broadcast, clip sharding, host gather by clip index.
(The data path has no collective: clips are independent; the only exchange is the one-off weight broadcast.)"""
import os
import socket
import sys

import numpy as np
import torch
import torch.multiprocessing as mp

from conftest import ROOT


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _worker(rank, world, port, n_clips, out_dir):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR='127.0.0.1',
                      MASTER_PORT=str(port))
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    load_package()
    from comfyui_keep_amd.engine import dist as kdist
    from comfyui_keep_amd.engine.weights import pack_blob, views
    r, w, _ = kdist.init_from_env(backend='gloo')
    assert (r, w) == (rank, world)
    # rank 0 owns the packed blob; everyone else receives index + blob
    if rank == 0:
        tensors = {'a.weight': torch.arange(12, dtype=torch.float32).view(3, 4), 'b.bias': torch.full((5,), 7.0)}
        blob, index = pack_blob(tensors)
        index, blob_t = kdist.broadcast_packed_weights(index, torch.from_numpy(blob), src=0)
    else:
        index, blob_t = kdist.broadcast_packed_weights(None, None, src=0)
    v = views(blob_t, index)
    assert torch.equal(v['a.weight'], torch.arange(12, dtype=torch.float32).view(3, 4)) and float(v['b.bias'][4]) == 7.0
    # independent clips: round-robin shard, "restore" = a function of the clip index only, gather on host by index
    mine = kdist.shard_clips(n_clips, rank, world)
    local = {c: np.full((2, 2), c * 10 + 1, dtype=np.uint8) for c in mine}
    full = kdist.gather_by_clip(local, n_clips, rank, world)
    if rank == 0:
        assert [int(a[0, 0]) for a in full] == [c * 10 + 1 for c in range(n_clips)]
        np.save(os.path.join(out_dir, 'ok.npy'), np.array([len(full)]))
    else:
        assert full is None
    # the product's sharding entry point (what KeepNet.run_clips_u8 runs on): every rank ends up with the full list
    clips = [np.full((2, 4, 4, 3), 3 * c, dtype=np.uint8) for c in range(n_clips)]
    seen = []

    def local_fn(mine_d):
        seen.extend(mine_d)
        return {i: 255 - c for i, c in mine_d.items()}
    allr = kdist.sharded_map(clips, local_fn, gather='all')
    assert sorted(seen) == mine and len(allr) == n_clips
    assert all(np.array_equal(allr[c], 255 - clips[c]) for c in range(n_clips))
    root = kdist.sharded_map(clips, local_fn, gather='root')
    assert (root is None) == (rank != 0)
    # ragged clips (different T per clip, what a 41-crop video gives: 20 + 20 + 1) through the fixed-size tensor gather,
    # with and without the caller providing the shapes
    ragged = [np.full((t, 4, 4, 3), 10 + c, dtype=np.uint8) for c, t in enumerate((20, 20, 1, 7, 3))]
    for shapes in ([r.shape for r in ragged], None):
        got = kdist.sharded_map(ragged, lambda d: {i: (c // 2) for i, c in d.items()}, gather='root', shapes=shapes)
        if rank == 0:
            assert all(g.shape == r.shape and np.array_equal(g, r // 2) for g, r in zip(got, ragged))
        else:
            assert got is None
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def _worker_real_blob(rank, world, port, out_dir):
    """The REAL packed weight blob (896 reference tensors -> fused / permuted kernel layouts, 633 MB) through the same
    broadcast + adopt_packed path bench.py and a multi-GPU deployment use; every named view must arrive bit-identical."""
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR='127.0.0.1',
                      MASTER_PORT=str(port))
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    load_package()
    import hashlib
    from comfyui_keep_amd.engine import dist as kdist, synth
    from comfyui_keep_amd.engine.arch import DEFAULT_ARCH
    from comfyui_keep_amd.engine.net import KeepNet
    kdist.init_from_env(backend='gloo')
    net = KeepNet(**DEFAULT_ARCH)
    if rank == 0:
        net.load_state_dict(synth.synth_state_dict(seed=0), strict=True)
        index, blob = kdist.broadcast_packed_weights(net._index, torch.from_numpy(net._blob), src=0)
    else:
        index, blob = kdist.broadcast_packed_weights(None, None, src=0)
    net.adopt_packed(index, blob)
    h = hashlib.blake2b(digest_size=16)
    for name in sorted(net.w):
        h.update(name.encode())
        h.update(str(tuple(net.w[name].shape)).encode())
        h.update(net.w[name].contiguous().numpy().tobytes())
    with open(os.path.join(out_dir, f'digest{rank}.txt'), 'w') as f:
        f.write(f'{len(net.w)} {blob.numel()} {h.hexdigest()}')
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_world2_real_weight_blob_broadcast(tmp_path):
    mp.spawn(_worker_real_blob, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    d0, d1 = (open(tmp_path / f'digest{r}.txt').read() for r in (0, 1))
    assert d0 == d1 and int(d0.split()[0]) > 600 and int(d0.split()[1]) > 150_000_000


def test_world2_broadcast_shard_gather(tmp_path):
    n_clips = 5
    mp.spawn(_worker, args=(2, _free_port(), n_clips, str(tmp_path)), nprocs=2, join=True)
    assert int(np.load(tmp_path / 'ok.npy')[0]) == n_clips


def test_shard_is_a_partition():
    sys.path.insert(0, ROOT)
    from comfyui_keep_amd.engine.dist import shard_clips
    for world in (1, 2, 4, 8):
        for n in (0, 1, 7, 15, 45):
            parts = [shard_clips(n, r, world) for r in range(world)]
            assert sorted(sum(parts, [])) == list(range(n))
            assert max(len(p) for p in parts) - min(len(p) for p in parts) <= 1


# ---------------------------------------------------------------------------------------------------------------- worker pool
# engine/pool.py driven on a machine without a GPU: KEEP_POOL_FAKE_NET=1 replaces the engine inside the workers by a stand-in
# (restored = 255 - crop under 'x3', 254 - crop otherwise; class map = blue channel mod 19), the root side is the stand-in below.
# Everything else is the product's code: rendezvous, the one broadcast, arenas, sequence numbers, config sync, failure paths.
class _FakeRootNet:
    supports_single_frame = True

    def __init__(self):
        from comfyui_keep_amd.engine.weights import pack_blob
        self.device = torch.device('cpu')
        self.cfg = {'tag': 'fake'}
        self.precision = 'x3'
        self.weights_generation = 0
        self.pool = None
        blob, self._index = pack_blob({'a.weight': torch.arange(4096, dtype=torch.float32).view(64, 64)})
        self._blob_t = torch.from_numpy(blob)
        self.local_calls = []

    def packed_blob(self):
        return self._blob_t

    def pool_config(self):
        return {'precision': self.precision, 'plan_ref_images': 0, 'flags': 0, 'attn_flags': 0, 'graph_mode': 'auto'}

    def _run_clips_u8_local(self, mine, max_b=None, sink=None):
        self.local_calls.append(sorted(mine))
        top = 255 if self.precision == 'x3' else 254
        out = {}
        for i, c in mine.items():
            c = torch.from_numpy(np.stack(c.frames)) if hasattr(c, 'frames') else c
            out[i] = (top - c.numpy().astype(np.int16)).clip(0, 255).astype(np.uint8)
        if sink is not None:
            sink(sorted(out), [torch.from_numpy(out[i]) for i in sorted(out)], None)
            return {}
        return out

    def run_clips_u8(self, clips, max_b=None, sink=None):
        from comfyui_keep_amd.engine.net import _FrameList
        clips = [c if isinstance(c, torch.Tensor) else _FrameList(c) for c in clips]
        return self.pool.run(self, clips, max_b, sink=sink)


def _pool_env(monkeypatch, **extra):
    monkeypatch.setenv('KEEP_POOL_FAKE_NET', '1')
    monkeypatch.delenv('KEEP_DIST_DEVICE', raising=False)
    for k, v in extra.items():
        monkeypatch.setenv(k, v)


def _ragged_clips(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (t, 8, 8, 3), generator=g, dtype=torch.uint8) for t in [20, 20, 1, 7, 3, 20, 2, 5, 20, 11, 4][:n]]


def test_pool_world4_order_config_sync_parse_and_arenas(monkeypatch):
    """GpuPool with three workers (world 4, gloo, no GPU): clip c runs on rank c % 4 and comes back in order; a precision change on
    the root reaches the workers before the next clip does (no clip is restored under a stale policy); ParseNet class
    maps ride back with a worker's crops; the shared-memory arenas of a worker are allocated once and reused; a weight change
    makes the pool refuse to run; close() leaves no worker and no shared memory behind."""
    _pool_env(monkeypatch)
    from comfyui_keep_amd.engine.pool import GpuPool, PoolError
    net = _FakeRootNet()
    pool = net.pool = GpuPool(net, 4, timeout=120, join_timeout=60)
    try:
        assert len(pool._procs) == 3 and pool.broadcast_ms > 0 and not torch.distributed.is_initialized()
        clips = _ragged_clips(11)
        out = pool.run(net, clips)
        assert net.local_calls[-1] == [0, 4, 8]
        assert all(torch.equal(o, 255 - c) for o, c in zip(out, clips))
        arenas = {r: tuple(m.name for m in pair) for r, pair in pool._arenas.items()}
        # the root switches policy after the pool came up: the workers follow before they see a clip
        net.precision = 'fp32'
        out = pool.run(net, clips)
        assert all(torch.equal(o, (254 - c.to(torch.int16)).clamp(0, 255).to(torch.uint8)) for o, c in zip(out, clips))
        assert pool.config['precision'] == 'fp32'
        assert {r: tuple(m.name for m in pair) for r, pair in pool._arenas.items()} == arenas          # same blocks, no re-allocation
        # sink + parse: groups arrive as (ids, crops, classes); the root's own share has no classes (the caller parses it on its GPU)
        net.precision = 'x3'
        pool.set_parser(('fake parser',))
        got = {}
        assert pool.run(net, clips, sink=lambda ids, crops, cls: got.update({i: (c, None if cls is None else cls[k])
                                                                               for k, (i, c) in enumerate(zip(ids, crops))}), parse=True) is None
        assert sorted(got) == list(range(11))
        for i, c in enumerate(clips):
            assert torch.equal(got[i][0], 255 - c)
            if i % 4 == 0:
                assert got[i][1] is None
            else:
                assert torch.equal(got[i][1], (255 - c)[..., 0] % 19)
        # clips given as lists of crops (what the processor holds)
        from comfyui_keep_amd.engine.net import _FrameList
        out = pool.run(net, [_FrameList([f.numpy() for f in c]) for c in clips[:5]])
        assert all(torch.equal(o, 255 - c) for o, c in zip(out, clips[:5]))
        # new weights on the root: the pool is stale
        net.weights_generation += 1
        try:
            pool.run(net, clips)
            raise AssertionError("a stale pool must refuse to run")
        except PoolError as e:
            assert 'other weights' in str(e)
        names = [m.name for pair in pool._arenas.values() for m in pair]
        procs = list(pool._procs)
    finally:
        pool.close()
    assert all(p.poll() is not None for p in procs) and not pool._procs and not pool._arenas
    from multiprocessing import shared_memory
    for n in names:
        try:
            shared_memory.SharedMemory(name=n)
            raise AssertionError(f"arena {n} was not unlinked")
        except FileNotFoundError:
            pass


def test_pool_startup_failures_do_not_hang(monkeypatch):
    """a worker that dies around the rendezvous must not leave the root waiting in the store for the c10d
    default timeout.  Stage 'import': the worker reports 'failed' before anyone joins; stage 'join': the worker dies after the
    handshake -- the root's join times out after `join_timeout` seconds and the error carries the worker's traceback."""
    import time
    from comfyui_keep_amd.engine.pool import GpuPool, PoolError
    for stage, limit in (('import', 60), ('join', 90)):
        _pool_env(monkeypatch, KEEP_POOL_TEST_FAIL=f'2:{stage}')
        net = _FakeRootNet()
        t0 = time.monotonic()
        try:
            GpuPool(net, 3, timeout=120, join_timeout=8)
            raise AssertionError("the pool came up although worker 2 failed")
        except PoolError as e:
            assert 'injected failure' in str(e), str(e)
        assert time.monotonic() - t0 < limit
        assert not torch.distributed.is_initialized()


def test_pool_through_process_image_sequence(monkeypatch):
    """The node's sequence entry point over the pool (world 4): 47 aligned frames -> clips of 20 + 20 + 7 sharded over root + 3
    workers -> restored faces in frame order, equal to the one-process result."""
    _pool_env(monkeypatch)
    import test_host_logic as H        # installs the ComfyUI stubs
    from comfyui_keep_amd.engine.pool import GpuPool
    from comfyui_keep_amd.modules.keep_model_loader import KEEPModelPack
    from comfyui_keep_amd.modules.keep_processor import KEEPFaceProcessor
    net = _FakeRootNet()
    pool = net.pool = GpuPool(net, 4, timeout=120, join_timeout=60)
    try:
        proc = KEEPFaceProcessor(KEEPModelPack(net, H._Helper(), None, None, 'KEEP'))
        proc.return_restored_aligned = True
        frames = torch.rand(47, 512, 512, 3)
        out = proc.process_image_sequence(frames, 1.0, True, True, False, max_clip_length=20)
        u8 = (frames * 255).to(torch.uint8)
        assert out.shape == (47, 512, 512, 3) and torch.equal(out, (255 - u8).float() / 255.0)
        assert net.local_calls[-1] == [0]                      # 3 clips over 4 ranks: the root ran clip 0, workers 1 and 2 the others
        assert len(proc.last_restored_faces) == 47
    finally:
        pool.close()


def test_bench_eight_ranks_line_over_gloo_with_the_stand_in_engine():
    """VERDICT r5 item 7 (first-8-GPU-run checklist, no hardware): `python bench.py --gpus 8` launches itself under torch.distributed.run
    on the loopback address; with KEEP_BENCH_FAKE_NET=1 the forward is a stand-in and the wire is gloo, everything else is the code the
    driver's SCALE run executes: rendezvous of 8 ranks, the weight broadcast in pieces (KEEP_BCAST_CHUNK_MB=1: four pieces of a 3.5 MB
    blob) with the per-rank checksum comparison, barrier + max-over-ranks timing, the per-rank gather, the one-video-per-GPU leg, ONE
    JSON line from rank 0 with the contract's keys."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, KEEP_BENCH_FAKE_NET='1', KEEP_BCAST_CHUNK_MB='1', OMP_NUM_THREADS='1')
    env.pop('KEEP_DIST_DEVICE', None)
    p = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '8', '--steps', '2', '--warmup', '1', '--clips', '2',
                        '--full', '--no-extras', '--no-cpu-baseline'], capture_output=True, text=True, env=env, timeout=600, cwd=root)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, p.stdout[-2000:]
    line = json.loads(lines[0])
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline', 'dtype',
              'data', 'config', 'broadcast_ms', 'broadcast_mb', 'broadcast', 'frames_per_s_per_rank', 'config5_one_video_per_gpu'):
        assert k in line, k
    assert line['fake_engine'] is True and line['roofline'] is None
    assert line['n_gpus'] == 8 and line['steps'] == 2 and line['warmup'] == 1 and line['scaling'] == 'weak'
    assert line['config']['clips_per_gpu'] == 2 and line['config']['parallelism'] == 'dp8 over clips'
    assert len(line['frames_per_s_per_rank']) == 8 and all(v > 0 for v in line['frames_per_s_per_rank'])
    assert abs(line['value'] - 8 * 2 * 20 * 2 / (2 * line['ms_per_step'] * 1e-3)) <= 0.01 * line['value']      # whole job / max-over-ranks time
    assert line['value'] <= sum(line['frames_per_s_per_rank']) * 1.001                                          # the slowest rank sets it
    b = line['broadcast']
    assert b['backend'] == 'gloo' and b['world'] == 8 and b['pieces'] == 4 and b['verified_identical_on_all_ranks'] is True
    assert 3.6 <= line['broadcast_mb'] <= 3.7 and b['largest_piece_mb'] <= 1.05 and line['broadcast_ms'] > 0
    c5 = line['config5_one_video_per_gpu']
    assert c5['crops_per_gpu'] == 300 and c5['clips_per_gpu'] == 15 and c5['value'] > 0
