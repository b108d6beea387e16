"""What do the footprint-table launches compute?  Every launched case of tests/test_gpu_footprint.py's CONV_CASES / ATTN_CASES --
the strided slices, three images, fused epilogues, split-K, statistics and amax slots the table was built to make awkward -- runs
once with exactly sized buffers (footprint.plain) and is compared with the float64 restatement of the ABI in tests/abi_ref.py:

* ``out`` against ``conv2d_ref`` / ``attention_ref`` under the tolerance class of the kernel family the plan names (abi_ref's
  docstring lists them); an x3 kernel under the suite's yardstick against its exact-f32 twin -- the same case with KEEP_MMA_F32 and
  the x3-only inputs cleared, and for the three features without an f32 kernel the decompositions the kernel tests use (LayerNorm
  epilogue: GEMM + keep_layernorm; in2: GEMM on the concatenation; x2 phases: upsample = 1 with the plain weights); a single-fp16 (x1)
  kernel per output against (2^-10 + 2e-6) sum |x| |w|;
* the amax slots: bit-equal to max |out[n]| of the device output, the other eight slots of the arena still zero;
* the statistics partials, summed over P: the per-(n, c) sum / sum of squares of the reference within what the element tolerance
  allows (HoWo * tol * scale, plus HoWo * 2^-24 * sum |ref| of float32 summation).

One ``[case-values]`` line per case (run with -s): kernel, class, err, scale, the position of the worst element, err_f32 for x3.
tests/test_host_logic.py proves on the CPU that this judge bites and that no optional input of any case can be ignored within
the tolerance.
"""
import pytest
import torch

import abi_ref as A
import footprint as FP
import test_gpu_footprint as T
from comfyui_keep_amd.engine import hiplib as L
from comfyui_keep_amd.engine import ops

pytestmark = pytest.mark.gpu

LAUNCHED_CONV = [n for n, (_, _, kw) in T.CONV_CASES.items() if kw.get('launch', True)]


def payloads(regions):
    """name -> payload tensor of every region that has one (the data the table put into the strided buffers)."""
    return {n: d for r in regions for n, (_, _, d) in r.windows.items() if d is not None}


def with_amax_neighbours(regions, N):
    """The 11-slot amax arena with the slots around the case's own as windows too, so that the plain run hands them back."""
    out = []
    for r in regions:
        if 'amax' in r.windows:
            off, n, data = r.windows['amax']
            assert (off, n, r.ld) == (3, N, 11)
            r = FP.Region(1, 11, {'amax_lo': (0, 3, torch.zeros(1, 3)), 'amax': (3, N, data), 'amax_hi': (3 + N, 8 - N, torch.zeros(1, 8 - N))},
                          torch.float32, 'rw')
        out.append(r)
    return out


def conv_twin_regions(name, t):
    """_conv_regions of the exact-f32 twin of x3 case ``name`` (``t``: the case's payloads)."""
    _, _, kw = T.CONV_CASES[name]
    g = T._Geom(kw)
    x = None
    if g.in2_cin1:
        M = g.N * g.H * g.W
        x = torch.cat([t['x'].reshape(M, g.cin1), t['x2'].reshape(M, g.Cin - g.cin1)], dim=-1).reshape(g.N, g.H, g.W, g.Cin)
    return T._conv_regions(name, A.conv_twin_kw(kw), x=x)


def run_conv(name, g, plan, regions, extra):
    def launch(tt):
        a = T._conv_args(g, {**tt, **extra})
        pl = L.conv2d_plan(a)
        assert (pl.kernel, pl.split_k, pl.stats_P) == (plan.kernel, plan.split_k, plan.stats_P), (name, pl.kernel, pl.split_k, pl.stats_P)
        a.split_k = pl.split_k
        L.conv2d_launch(a)
    return FP.plain(launch, regions, 'cuda')[0]


@pytest.mark.parametrize('name', LAUNCHED_CONV)
def test_conv2d_case_values(name):
    g, plan, regions, extra = T._conv_regions(name)
    kernel = plan.kernel.decode()
    got = run_conv(name, g, plan, with_amax_neighbours(regions, g.N), extra)
    t = payloads(regions)
    ref = A.conv2d_ref(g, t)
    twin = None
    if A.conv_class(kernel) == 'x3':
        g2, plan2, regions2, extra2 = conv_twin_regions(name, t)
        assert A.conv_class(plan2.kernel.decode()) == 'f32', (name, plan2.kernel.decode())
        twin = run_conv(name, g2, plan2, regions2, extra2)['out']
        if g.ln:
            dv = lambda v: v.cuda().reshape(-1).contiguous()  # noqa: E731
            twin = ops.layernorm(twin, dv(t['ln_gamma']), dv(t['ln_beta']), res=t['res'].cuda().contiguous() if g.res_ld else None, eps=A.LN_EPS)
            torch.cuda.synchronize()
    A.judge_conv(name, kernel, g, got, ref, twin, plan.stats_P)


@pytest.mark.parametrize('case', T.ATTN_CASES, ids=[c['name'] for c in T.ATTN_CASES])
def test_attention_case_values(case):
    regions, launch = T.attn_case_launch(case)
    got = FP.plain(launch, regions, 'cuda')[0]['o']
    t = payloads(regions)
    ref = A.attention_ref(case, t['q'], t['k'], t['v'])
    twin = None
    if A.attn_class(case) == 'x3':      # same name -> same data; the range maxima and the kernel-selection flags are x3-only
        regions2, launch2 = T.attn_case_launch(dict(case, mma=L.MMA_F32, flags=0, amax=False))
        twin = FP.plain(launch2, regions2, 'cuda')[0]['o']
    A.judge_attn(case, got, ref, twin)
