"""The planner's routes AND plans on a reduced grid, against tests/golden/routes_mi355x.txt.

plan_launch (csrc/api.hip) picks a kernel family, a registry row and a launch geometry per request shape; the fixture was
recorded from the library of the commit BEFORE the planner was split into choose / fill stages, through
fx_plan_kernel's digest (family, row, grid, LDS bytes, every integer the launcher reads, the device table chosen, a hash of
the floating-point arguments).  A change that is meant to keep every route and every plan must leave the lines identical; a
change that moves one on purpose re-records the fixture (python tests/test_gpu_routes.py) and says so.

The lines are built by tools/route_sweep.py's own sweep_lines, --digest-hash form: per (policy, element, order) one SHA-256
prefix over the --digest lines of its modes and batches, names and digests of all 130 point counts -- the full reports of
this grid are ~100 MB, a committed file holds at most 1 MiB and is read by people.  To see WHAT differs in a failing line:
tools/route_sweep.py --digest --only "<start of the line>" OUT with either library.  Grid: every point count 1-130; orders
0-2; own cell / cells / cells + Piola map where the element has one; batches of 1 and 100000; policies default, wg_small, stacked_small, no_stacked_mix, no_small; the elements the windows
of plan_launch name -- Lagrange 3-6 on triangles and tetrahedra, Nedelec / Raviart-Thomas 2 and 3 and Brezzi-Douglas-Marini
1 and 3 on tetrahedra, Nedelec 3 on triangles, the sweep's random set of 75 rows.  Nothing of that grid was dropped.  The
grids and LDS sizes depend on the device's CU count and LDS per CU, hence the fixture's name."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "routes_mi355x.txt")
POLICIES = [(), ("wg_small",), ("stacked_small",), ("no_stacked_mix",), ("no_small",)]
ELEMENTS = ([("Lagrange", 2, d) for d in (3, 4, 5, 6)] + [("Lagrange", 3, d) for d in (3, 4, 5, 6)] +
            [("Nedelec", 3, 2), ("Nedelec", 3, 3), ("RaviartThomas", 3, 2), ("RaviartThomas", 3, 3),
             ("BrezziDouglasMarini", 3, 1), ("BrezziDouglasMarini", 3, 3), ("Nedelec", 2, 3)])


def route_lines():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import route_sweep
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    from fiat_amd import runtime
    ctx = runtime.Context.get()
    els = [route_sweep.family_element(*spec) for spec in ELEMENTS] + [route_sweep.random_element()]
    try:
        return [line for line, _ in route_sweep.sweep_lines(ctx, els, POLICIES, digest="hash")]
    finally:
        ctx.set_policy()


@pytest.mark.gpu
def test_routes_and_plans_match_the_recorded_ones():
    with open(FIXTURE) as f:
        want = f.read().splitlines()
    got = route_lines()
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"line {i + 1} differs:\n  planned : {g}\n  recorded: {w}"
    assert len(got) == len(want), f"{len(got)} lines planned, {len(want)} recorded"


if __name__ == "__main__":  # record the fixture (on the MI355X)
    with open(sys.argv[1] if len(sys.argv) > 1 else FIXTURE, "w") as f:
        f.write("\n".join(route_lines()) + "\n")
