"""CPU: the host side of the KEEP network's opt-in single-fp16 precision ('f16': the x3 policy with KEEP_MMA_X1 substituted where the
library's plan admits it) -- the precision knob, the per-call routing of Ops, and the ABI version of header and binding."""
import os
import re

import pytest

from comfyui_keep_amd.engine import hiplib as L
from comfyui_keep_amd.engine import net as N
from comfyui_keep_amd.engine import ops
from comfyui_keep_amd.engine.arch import DEFAULT_ARCH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_f16_is_a_precision_and_not_the_default():
    assert 'f16' in N.PRECISIONS and N.DEFAULT_PRECISION == 'x3'
    assert set(N.PRECISIONS) == {'fp32', 'x3', 'bf16', 'f16'}


def test_environment_selects_f16_and_unknown_values_raise(monkeypatch):
    monkeypatch.setenv('KEEP_AMD_PRECISION', 'f16')
    assert N.KeepNet(**DEFAULT_ARCH).precision == 'f16'
    monkeypatch.delenv('KEEP_AMD_PRECISION')
    net = N.KeepNet(**DEFAULT_ARCH)
    assert net.precision == 'x3'
    assert net.set_precision('f16').precision == 'f16'
    monkeypatch.setenv('KEEP_AMD_PRECISION', 'fp16')
    with pytest.raises(ValueError, match='precision must be one of'):
        N.KeepNet(**DEFAULT_ARCH)
    with pytest.raises(ValueError, match='precision must be one of'):
        net.set_precision('half')


class _Plan:
    def __init__(self, kernel, split_k=1):
        self.kernel, self.split_k = kernel, split_k


def test_routing_picks_x1_where_the_plan_admits_it_and_x3_otherwise():
    """KeepNet's rule (Ops.set_x1_twin(..., base_kernel=X3_STREAM_KERNEL)): route_x1 hands back the call's X1 plan, or None = the base."""
    import torch
    o = ops.Ops()
    o.set_precision(L.MMA_X3, torch.zeros(64), None, torch.zeros(128, dtype=torch.int16))
    o.set_x1_twin(torch.zeros(64, dtype=torch.int16), [(0, 64, 1.0)], flags=0, base_kernel=ops.X3_STREAM_KERNEL)
    asked = []
    x1 = _Plan('conv3x3_halo_x3s_kernel<1, true, true>')

    def admits():
        asked.append('yes')
        return x1

    def refuses():
        asked.append('no')
        raise L.KeepHipError('keep_conv2d_plan failed (code -2): keep_conv2d: KEEP_MMA_X1 has no kernel for this call')

    def broken():
        raise L.KeepHipError('keep_conv2d_plan failed (code -1): keep_conv2d: bad mma 7')
    stream = _Plan(ops.X3_STREAM_KERNEL)
    assert o.route_x1('a', stream, admits) is x1
    assert o.route_x1('b', stream, refuses) is None      # KEEP_EUNSUP: the call stays on the base
    # one plan query per shape: the answers are cached by key
    assert o.route_x1('a', stream, refuses) is x1 and o.route_x1('b', stream, admits) is None and asked == ['yes', 'no']
    # only the un-split streaming 3x3 kernel is substituted: the library is not even asked about anything else
    for k, pl in enumerate((_Plan('gemm_x3l_kernel<4>'), _Plan('conv_x3_kernel<2, 2, 2, 2, true, true>'), _Plan('conv3x3_halo_x3_kernel<32, x2 phases>'),
                            _Plan('conv3x3_halo_x3_kernel<16>'), _Plan(ops.X3_STREAM_KERNEL, split_k=4))):
        assert o.route_x1(('other', k), pl, admits) is None
    assert asked == ['yes', 'no']
    with pytest.raises(L.KeepHipError, match='bad mma'):      # an error is not an answer
        o.route_x1('c', stream, broken)


def test_x1_is_no_base_policy():
    with pytest.raises(ValueError, match='no base policy'):
        ops.Ops().set_precision(L.MMA_X1)


def test_f16_never_hands_x1_to_attention():
    """'f16' rides on the x3 policy: Ops.mma / Ops.attn_mma stay L.MMA_X3 (keep_attention refuses KEEP_MMA_X1), the twin is an extra; a
    policy change drops it, and it cannot be attached to another policy."""
    import torch
    o = ops.Ops()
    blob = torch.zeros(64)
    o.set_precision(L.MMA_X3, blob, None, torch.zeros(128, dtype=torch.int16), 1.0, x3_scales=[(0, 64, 1.0)])
    o.set_x1_twin(torch.zeros(64, dtype=torch.int16), [(0, 32, 1.0)])
    assert o.mma == L.MMA_X3 and o.attn_mma == L.MMA_X3 and o.blobx1 is not None
    assert o.x1_twin(blob[:32]).numel() == 32 and o.x1_twin(blob[32:]) is None      # a tensor without a twin stays x3
    o.set_precision(L.MMA_F32, blob, None)
    assert o.blobx1 is None and o.x1_twin(blob[:32]) is None
    with pytest.raises(ValueError, match='x3 policy'):
        o.set_x1_twin(torch.zeros(64, dtype=torch.int16), [(0, 32, 1.0)])


def test_header_and_binding_agree_on_abi_v23():
    header = open(os.path.join(ROOT, 'include', 'keep_hip.h')).read()
    assert int(re.search(r'#define KEEP_ABI_VERSION (\d+)', header).group(1)) == L.ABI_VERSION == 23
    assert 'v23' in header
