"""bench.py's own plumbing: the device-side input generator against synth.synth_clip (bit for bit), what a plain run prints and
what --dump-outputs writes -- with the stand-in engine on a machine without a GPU, and on the HIP engine (-m gpu)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

HEADLINE = ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline', 'dtype',
            'data', 'config')
FULL_ONLY = ('roofline', 'whole_net_tflops_executed', 'other_policies', 'b1', 'clips16', 'pcie_inclusive', 'configs', 'paste_back_gpu',
             'facelib', 'end_to_end', 'end_to_end_product', 'cpu_baseline', 'config5_one_video_per_gpu')

# (T, B, seed, phase): a short clip at rank 0, and the bench's full T = 20 at rank 1 (seed 1234 + rank, phase 0.37 * rank)
CLIP_CASES = [(3, 2, 1234, 0.0), (20, 2, 1235, 0.37)]


def _bench(args, env_extra, cwd):
    env = dict(os.environ, **env_extra)
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + args, capture_output=True, text=True, env=env,
                       timeout=900, cwd=cwd)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def _check_plain_line(line, steps, warmup, clips):
    for k in HEADLINE:
        assert k in line, k
    for k in FULL_ONLY:
        assert k not in line, k
    assert line['steps'] == steps and line['warmup'] == warmup and line['config']['clips_per_gpu'] == clips
    assert line['unit'] == 'frames/s' and line['higher_is_better'] is True and line['dtype'] == 'f16x3'
    # value = frames of the timed steps / their wall time; ms_per_step = that wall time / steps
    assert abs(line['value'] - clips * 20 * 1e3 / line['ms_per_step']) <= 0.01 * line['value']


@pytest.mark.parametrize('T,B,seed,phase', CLIP_CASES)
def test_device_clip_generator_is_synth_clip_bit_for_bit(T, B, seed, phase):
    import bench
    from comfyui_keep_amd.engine import synth
    assert torch.equal(bench.synth_clip_device(T, B, seed, phase, 'cpu'), synth.synth_clip(T=T, B=B, seed=seed, phase=phase))


@pytest.mark.gpu
@pytest.mark.parametrize('T,B,seed,phase', CLIP_CASES)
def test_device_clip_generator_on_the_gpu_is_synth_clip_bit_for_bit(T, B, seed, phase):
    import bench
    from comfyui_keep_amd.engine import synth
    got = bench.synth_clip_device(T, B, seed, phase, torch.device('cuda')).cpu()
    assert torch.equal(got, synth.synth_clip(T=T, B=B, seed=seed, phase=phase))


def test_dump_outputs_samples_a_large_output_within_budget(tmp_path):
    """An output larger than DUMP_BYTES is written as a fixed sample: one element from each of equal runs of the flattened array,
    in order, the same positions on every call; under --gpus N every rank writes its own file with 1 / N of the bytes."""
    import bench
    n = bench.DUMP_BYTES // 8
    out = torch.arange(n + n // 2 + 7, dtype=torch.float64).view(-1, 1)       # value = flat position
    bench.dump_outputs(out, str(tmp_path / 'a'), 0, 1)
    bench.dump_outputs(out, str(tmp_path / 'b'), 0, 1)
    bench.dump_outputs(out, str(tmp_path / 'c'), 1, 2)
    a = np.load(tmp_path / 'a' / 'restored_frames.npy')
    assert np.array_equal(a, np.load(tmp_path / 'b' / 'restored_frames.npy'))
    assert a.dtype == np.float64 and a.ndim == 1 and a.nbytes <= bench.DUMP_BYTES and a.size > 0.9 * (n // 2)
    assert (np.diff(a) > 0).all() and ((a // 2) == np.arange(a.size)).all()          # runs of 2: one element from each
    c = np.load(tmp_path / 'c' / 'restored_frames_rank1.npy')
    assert c.nbytes <= bench.DUMP_BYTES // 2 and ((c // 4) == np.arange(c.size)).all()
    small = torch.rand(2, 3, 4, 5)
    bench.dump_outputs(small, str(tmp_path / 'd'), 0, 1)
    assert np.array_equal(np.load(tmp_path / 'd' / 'restored_frames.npy'), small.numpy())     # whole, in its shape


def test_plain_and_full_lines_and_dump_with_the_stand_in_engine(tmp_path):
    """KEEP_BENCH_FAKE_NET=1 (the forward is 1 - x, no GPU): a plain run prints the headline keys and nothing that needs runs of its
    own, and --dump-outputs writes exactly what the last timed step returned; --full adds the roofline key (null for the stand-in)."""
    env = {'KEEP_BENCH_FAKE_NET': '1', 'OMP_NUM_THREADS': '1'}
    line = _bench(['--gpus', '1', '--steps', '3', '--warmup', '1', '--clips', '2', '--dump-outputs', str(tmp_path / 'out')], env, str(tmp_path))
    _check_plain_line(line, 3, 1, 2)
    x = torch.rand((2, 20, 3, 32, 32), generator=torch.Generator().manual_seed(1234))        # bench.py's stand-in input at rank 0
    got = np.load(tmp_path / 'out' / 'restored_frames.npy')
    assert got.dtype == np.float32 and np.array_equal(got, (1.0 - x).numpy())
    full = _bench(['--gpus', '1', '--steps', '2', '--warmup', '1', '--clips', '2', '--full'], env, str(tmp_path))
    assert full['roofline'] is None and full['steps'] == 2 and 'whole_net_tflops_executed' in full


@pytest.mark.gpu
def test_plain_run_on_the_engine_dumps_what_the_forward_returns(tmp_path, synth_weights):
    """`bench.py --gpus 1` without --full on the HIP engine (one clip): the headline line only, and the dumped sample equals the same
    sample of an in-process forward of the same input (bench.py's clip at rank 0) on the same weights."""
    import bench
    from comfyui_keep_amd.engine.arch import DEFAULT_ARCH
    from comfyui_keep_amd.engine.net import KeepNet
    line = _bench(['--gpus', '1', '--steps', '2', '--warmup', '1', '--clips', '1', '--dump-outputs', str(tmp_path / 'bench')], {},
                  str(tmp_path))
    _check_plain_line(line, 2, 1, 1)
    assert line['x3_range_fallbacks'] == 0
    net = KeepNet(**DEFAULT_ARCH)
    net.load_state_dict(synth_weights, strict=True)
    net.to('cuda').eval().set_precision('x3')
    out = net(bench.synth_clip_device(20, 1, 1234, 0.0, torch.device('cuda')))
    bench.dump_outputs(out, str(tmp_path / 'here'), 0, 1)
    got, want = (np.load(tmp_path / d / 'restored_frames.npy') for d in ('bench', 'here'))
    assert got.dtype == np.float32 and got.shape == want.shape and got.nbytes <= bench.DUMP_BYTES
    assert np.isfinite(got).all() and np.abs(got - want).max() <= 1e-5
