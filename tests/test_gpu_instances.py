"""Every compiled kernel is launched by a case that checks its output (tests/instance_manifest.py, one case per kernel,
found by tools/instance_search.py).  For each case: (1) the kernels that really ran -- the profiler's device-side records,
normalised -- EQUAL the case's list, so a dispatch line that launches another twin, or an extra pass the manifest does not
know, fails; (2) the output equals a plain reference of the same operation (tests/instance_runner.py: the C oracle on the
physical cells, Piola maps written out in NumPy, long-double 1-D bases, NumPy statements of the auxiliary operations) at
the standing tolerances, 1e-12 for value tables and 1e-10 for derivative tables relative to max(1, max |ref|) of the table;
(3) cases whose kernel leaves its tables through store.hpp flush_block or an 8-byte flush twin also run into guarded views
at 0, 1, 7 and 8 doubles past a 128-byte line: guards untouched, every entry written, no NaN, tables bit-equal."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import edge_reference as R  # noqa: E402
import instance_manifest as M  # noqa: E402


@pytest.mark.parametrize("case", M.CASES, ids=[c["id"] for c in M.CASES])
def test_instance(case, kernel_policy):
    import torch
    import instance_runner as IR
    p = IR.prepare(case)
    kernel_policy(*case["policy"])
    p.run()                                                     # lazy set-up of the element (stacked matrices ...) happens here
    ran = {n for n in M.normalise_all(sorted(R.launched(p.run))) if n.startswith(M.NAMESPACE)}
    assert ran == set(case["kernels"]), (sorted(ran - set(case["kernels"])), sorted(set(case["kernels"]) - ran))
    got = p.run()
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    ref = p.reference()
    rows = IR.compare_tables(got.reshape(np.shape(ref)), ref, p.table_axis, p.tol)
    print(case["id"], " ".join(f"t{t}:{err:.1e}" for err, _, t in rows))
    for err, bound, t in rows:
        assert err <= bound, (case["id"], "table", t, err, bound)
    if M.guarded(case):
        assert p.shape is not None
        fresh = R.compare(lambda o: p.run(out=o), tuple(p.shape), torch.device("cuda", torch.cuda.current_device()))
        assert np.array_equal(fresh.cpu().numpy().reshape(got.shape), got)
