"""What do the flat footprint-table launches compute?  Every (entry point, case) of tests/test_gpu_footprint.py's FLAT_CASES -- C = 6
with ld = 9, M = 35, F = 20, 5 x 7 maps, one-pixel outputs, channel slices of wider rows -- runs once with exactly sized buffers
(footprint.plain) and is judged against the plain restatement of include/keep_hip.h in tests/flat_ref.py: bit for bit where the ABI
promises bits, against float64 under the tolerance the operation's own reference test uses otherwise (flat_ref's docstring holds the
table).  The amax arenas carry a marker in the slots around the case's own, which must come back untouched.

One ``[flat-values]`` line per output (run with -s): entry point, case, output, class, err, scale, tol, the position of the worst
element.  tests/test_host_logic.py proves on the CPU that this judge bites on every case, the last element included, and that no
optional input of any case can be ignored within the tolerance.
"""
import pytest

import flat_ref as R
import footprint as FP
import test_gpu_footprint as T

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('fn,case', [(fn, cid) for fn, cases in T.FLAT_CASES.items() for cid, _, _ in cases])
def test_flat_op_values(fn, case):
    regions, launch, _, params = T.flat_case(fn, case)
    specs = R.reference(fn, params, R.payloads(regions, fn, params))
    got = FP.plain(launch, R.with_amax_neighbours(regions), 'cuda')[0]
    R.judge(fn, case, specs, got)
