"""CPU: the host side of the KEEP network's opt-in single-fp16 precision ('f16': the x3 policy with KEEP_MMA_X1 substituted where the
library's plan admits it) -- the precision knob and the ABI version of header and binding."""
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
