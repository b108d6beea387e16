"""The CPU restatement of a carried clip (tests/carry_ref.py) against the oracle it is composed from and against its committed result
(tests/golden/carry_T4.npz, tests/make_carry_golden.py).  The GPU side reads the fixture in tests/test_gpu_track_carry.py."""
import os

import numpy as np
import pytest

from comfyui_keep_amd.engine import synth
from conftest import GOLDEN

PATH = os.path.join(GOLDEN, 'carry_T4.npz')


def test_fixture_holds_what_the_gpu_test_reads():
    g = np.load(PATH)
    a, b, c, d = (int(v) for v in g['crop'])
    assert int(g['seed']) == 4321 and int(g['cut']) == 2 and (b - a, d - c) == (128, 128)
    assert g['indices'].shape == (4, 256) and g['indices'].dtype == np.int16 and g['margins'].shape == (4, 256)
    assert g['gains0_second'].shape == (256,) and 0.0 < g['gains0_second'].min() and g['gains0_second'].max() < 1.0
    assert g['out_crop'].shape == (4, 3, 128, 128) and g['out_grid'].shape == (4, 3, 32, 32)
    assert np.isfinite(g['out_crop']).all() and os.path.getsize(PATH) < (1 << 20)


@pytest.mark.slow
def test_restatement_is_the_oracle_and_reproduces_the_fixture(synth_weights):
    """(a) The pin: cut in two at frame 2 and given the uncut clip's gains, ``carry_ref`` reproduces ``oracle.keep_forward`` on the uncut
    clip to 0.0, indices included -- the state in / out changes nothing else.  (b) With each half's own gains it reproduces the
    committed fixture (bounds of tests/test_oracle_vs_golden.py: indices wherever the margin exceeds 1e-3, gains 1e-4, pixels 3e-4)."""
    import make_carry_golden as M
    g = np.load(PATH)
    x = synth.synth_clip(T=M.T, B=1, seed=int(g['seed']))
    err, same = M.pin_error(x, synth_weights)
    print('max |carry_ref(forced gains) - keep_forward| =', err, '; indices equal:', same)
    assert err == 0.0 and same
    out, aux_a, aux_b = M.split_run(x, synth_weights)
    idx = np.concatenate([aux_a['indices'][0].numpy(), aux_b['indices'][0].numpy()]).astype(np.int16)
    safe = g['margins'] > 1e-3
    assert np.array_equal(idx[safe], g['indices'][safe])
    assert np.abs(aux_b['gains'][0, 0].reshape(-1).numpy() - g['gains0_second']).max() <= 1e-4
    a, b, c, d = (int(v) for v in g['crop'])
    # the frames in front of the first frame with a differing (low-margin) token; frame 0 is always compared
    first = next((t for t in range(M.T) if not np.array_equal(idx[t], g['indices'][t])), M.T)
    print('first frame with a differing index:', first, 'of', M.T)
    assert first >= 1
    assert np.abs(out[0][:first, :, a:b, c:d].numpy() - g['out_crop'][:first]).max() <= 3e-4
    assert np.abs(M.digest(out[0]).numpy()[:first] - g['out_grid'][:first]).max() <= 3e-4
