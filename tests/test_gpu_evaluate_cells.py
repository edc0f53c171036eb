"""``evaluate_batch`` with per-request cells on the GPU: every family and every instance of the fused kernel on many cells of
both orientations, the item shapes, right-hand sides, elements built on their own non-UFC cell, output alignment and empty
calls.  The oracle is closed form (tests/evaluate_cells_reference.py): the reference's own tables on its reference cell pushed
through the chain rule and the Piola formulas, independent of the kernel's recurrence, cell map and Piola code.  Every request
of every call is compared, at the project's standing 1e-12 on values and 1e-10 on derivatives in the norm
max|x - ref| / max(1, max|ref|).  Every fused call writes into a guarded output, is asserted to have launched exactly the named
instance, and ``evaluate_kernel`` is asserted to report that instance with the (P, chunks) of ``expected_plan``."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import edge_reference as E  # noqa: E402
import evaluate_cells_reference as C  # noqa: E402
import make_golden_evaluate as M  # noqa: E402
from evaluate_gpu_common import G, assert_launched, check, element, expected_plan, facts, fused, instance, restated  # noqa: E402


def ids(cases):
    return ["-".join(str(x) for x in c) for c in cases]


def report(el, order, npts, nrhs, pushforward):
    """``evaluate_kernel`` names the instance and the item scheme that the launcher's arithmetic predicts."""
    sd, n, _, vdim, ndof = facts(el)
    P, chunks = expected_plan(sd, n, order, vdim, ndof, npts)
    assert (P, chunks) == C.R.plan(sd, n, order, vdim, ndof, npts)
    assert el.evaluate_kernel(order, npts, nrhs=nrhs, has_verts=True, pushforward=pushforward) == \
        f"fused: fxk::{instance(el, order)} degree={n} P={P} chunks={chunks}"
    return P, chunks


def pushes(name):
    return C.meta(name)["mapping"] != 0


def fused_cells(el, name, order, b, dofs=None, offset=1):
    """The fused route on the batch ``b`` with its cells (the Piola families pushed forward), under ``fused``'s discipline."""
    dofs = b["dofs"] if dofs is None else dofs
    report(el, order, b["pts"].shape[1], dofs.shape[1] if dofs.ndim == 3 else 1, pushes(name))
    return fused(el, order, b["pts"], dofs, verts=b["verts"], pushforward=pushes(name), offset=offset)


def flat(dofs):
    """(nreq, 1, ndof) -> (nreq, ndof)."""
    return np.ascontiguousarray(dofs[:, 0])


def test_case_lists_reach_every_instance_with_cells():
    """All 15 compile-time instances run with ``verts`` in this file: every call below asserts that it launched exactly the
    instance of its case, and the cases cover the set."""
    assert C.instances_with_cells() == {(sd, o, v) for sd in (1, 2, 3) for o in range(3) for v in {1, sd}}
    assert {C.instance_of(c[0], c[1]) for c in C.FAMILY_CASES + C.INSTANCE_CASES} == C.instances_with_cells()
    both = {(C.meta(n)["sd"], C.meta(n)["mapping"], o) for n, o, *_ in C.FAMILY_CASES + C.INSTANCE_CASES if pushes(n)}
    assert both == {(sd, mp, o) for sd in (2, 3) for mp in (1, 2) for o in range(3)}       # both Piola kinds at every order


@pytest.mark.parametrize("case", C.FAMILY_CASES, ids=ids(C.FAMILY_CASES))
def test_every_family_on_many_cells(case):
    """All fused fixture cases at order 2: the fixture's points permuted per request, three whole items and a partial one,
    cells of both orientations, Piola families pushed forward; the fused route and, on the same batch, the general route
    (``tabulate_batch(verts=, pushforward=)`` on many cells) against the closed-form oracle."""
    name, order, npts, nreq, nrhs = case
    el = element(name)
    b = C.batch(*case)
    P, chunks = report(el, order, npts, nrhs, pushes(name))
    assert chunks == 1 and nreq == 3 * P + 2
    out = fused_cells(el, name, order, b, dofs=flat(b["dofs"])).cpu().numpy()
    check(out[:, :, None], b["ref"], (name, "fused"))
    general = el.evaluate_batch(order, b["pts"], flat(b["dofs"]), verts=b["verts"], pushforward=pushes(name), route="general")
    check(general.cpu().numpy()[:, :, None], b["ref"], (name, "general"))


@pytest.mark.parametrize("case", C.INSTANCE_CASES, ids=ids(C.INSTANCE_CASES))
def test_every_instance_with_cells(case):
    """Orders 0 and 1 of one element per (sd, vdim) and of one contravariant element per dimension: with the order-2 cases
    above, all 15 instances run the ``verts`` branch, and both Piola kinds run at every order in 2-D and 3-D."""
    name, order, npts, nreq, nrhs = case
    el = element(name)
    assert (facts(el)[0], order, facts(el)[3]) == C.instance_of(name, order)
    b = C.batch(*case)
    out = fused_cells(el, name, order, b, dofs=flat(b["dofs"])).cpu().numpy()
    check(out[:, :, None], b["ref"], case)


@pytest.mark.parametrize("npts", C.SHAPE_POINTS)
@pytest.mark.parametrize("name", C.SHAPE_ELEMENTS)
def test_item_shapes_with_cells(name, npts):
    """One lane per request (the LDS budget sets P), the wave boundary, and point-chunked requests with a partial last chunk
    and the Piola map applied before the stores from registers; one request, an item less one, an item, one more, and three
    items and two requests."""
    el = element(name)
    cases = [c for c in C.SHAPE_CASES if c[0] == name and c[2] == npts]
    order = cases[0][1]
    P, chunks = report(el, order, npts, 1, pushes(name))
    assert (chunks > 1) == (npts > 64)
    if npts == 1:
        assert 1 < P < 64                   # fewer requests than lanes: the LDS budget sets P
    assert [c[3] for c in cases] == E.nreq_list(P if chunks == 1 else 1)
    for case in cases:
        b = C.batch(*case)
        out = fused_cells(el, name, order, b, dofs=flat(b["dofs"])).cpu().numpy()
        check(out[:, :, None], b["ref"], case)


@pytest.mark.parametrize("case", C.RHS_CASES, ids=ids(C.RHS_CASES))
def test_right_hand_sides_with_cells(case):
    """nrhs 1 (2-D and 3-D dofs), 3 and 8 with cells: every right-hand side against the oracle, and bit for bit the single-rhs
    call on that slice."""
    import torch
    name, order, npts, nreq, nrhs = case
    assert nrhs == 8
    el = element(name)
    b = C.batch(*case)
    single = [fused_cells(el, name, order, b, dofs=np.ascontiguousarray(b["dofs"][:, j])) for j in range(nrhs)]
    for j in range(nrhs):
        check(single[j].cpu().numpy(), b["ref"][:, :, j], (name, "single", j))
    one = fused_cells(el, name, order, b, dofs=np.ascontiguousarray(b["dofs"][:, :1]))
    assert one.shape[2] == 1 and torch.equal(one[:, :, 0], single[0])
    for k in (3, 8):
        many = fused_cells(el, name, order, b, dofs=np.ascontiguousarray(b["dofs"][:, :k]))
        assert many.shape[2] == k
        check(many.cpu().numpy(), b["ref"][:, :, :k], (name, "nrhs", k))
        for j in range(k):
            assert torch.equal(many[:, :, j], single[j]), (k, j)


@pytest.mark.parametrize("name", C.OWN_ELEMENTS)
def test_element_on_its_own_cell(name):
    """The element built on the fixture's skewed cell (``EvalArgs::A0``, ``b0``).  Without ``verts`` the fused route equals the
    reference's element built on that cell (``{name}_pref``) at all three orders; with per-request cells on top it equals
    those tables chained through the map of the own cell onto the request's cell, and the restatement in extended precision.
    The values of the oracle carry the reference's own rounding on a cell with edges of 0.05 (1.9e-13 for Lagrange 4 on the
    tetrahedron, the same against the restatement in float64 and in extended precision), not that of the requests' cells."""
    el = element(name, own=True)
    sd = facts(el)[0]
    ntabs = [len(E.jet(sd, o)) for o in range(3)]
    pts, dofs, pref = G[f"{name}_ppts"][None], G[f"{name}_dofs"][None], G[f"{name}_pref"][None]
    for order in range(3):
        assert el.evaluate_kernel(order, pts.shape[1], nrhs=M.NRHS).startswith(f"fused: fxk::{instance(el, order)} ")
        out = fused(el, order, pts, dofs).cpu().numpy()
        check(out, pref[:, :ntabs[order]], (name, "own cell", order))
        names = E.launched(lambda: el.evaluate_batch(order, pts, dofs))           # route=None takes the fused kernel
        assert_launched(names, el, order)
    for case in [c for c in C.OWN_CASES if c[0] == name]:
        order = case[1]
        b = C.batch(*case, own=True)
        out = fused_cells(el, name, order, b, dofs=flat(b["dofs"])).cpu().numpy()
        check(out[:, :, None], b["ref"], (case, "own cell and cells"))
        check(out[:, :, None], restated(el, order, b["pts"], b["dofs"], verts=b["verts"], cell=G[f"{name}_verts"], longdouble=True),
              (case, "restatement"))


@pytest.mark.parametrize("name", ["ned_tri3", "rt_tet2"])
def test_piola_element_on_its_own_cell(name):
    """A Piola family built on the skewed cell, with per-request cells and the push-forward: J = E_req G with G = A0 / 2 of
    the own cell.  Against the restatement in extended precision, and the general route against the same."""
    el = element(name, own=True)
    cell = G[f"{name}_verts"]
    for order in range(3):
        b = C.batch(name, order, 7, 13, seed=order)
        out = fused_cells(el, name, order, b, dofs=flat(b["dofs"])).cpu().numpy()
        ref = restated(el, order, b["pts"], b["dofs"], verts=b["verts"], pushforward=True, cell=cell, longdouble=True)
        check(out[:, :, None], ref, (name, order, "fused"))
        general = el.evaluate_batch(order, b["pts"], flat(b["dofs"]), verts=b["verts"], pushforward=True, route="general")
        check(general.cpu().numpy()[:, :, None], ref, (name, order, "general"))


@pytest.mark.parametrize("case", C.ALIGN_CASES, ids=ids(C.ALIGN_CASES))
def test_output_alignment_with_cells(case):
    """``out`` 0, 1, 7 and 8 doubles past a 128-byte line.  Whole requests of 7 doubles, 9 an item: the items have 63, 63 and
    14 doubles and their starts alternate in parity: the odd items leave by the scalar loop and the even last item by
    ``flush_block`` where it starts on 16 bytes (the even offsets: both branches inside one launch) and by the scalar loop too
    at the odd offsets; and a chunked shape.  Bit-identical across the offsets and equal to the oracle."""
    from fiat_amd import runtime
    name, order, npts, nreq, nrhs = case
    el = element(name)
    b = C.batch(*case)
    P, chunks = report(el, order, npts, 1, False)
    reqsize = b["ref"][0].size
    if chunks == 1:
        assert (P, reqsize % 2, P % 2) == (9, 1, 1) and [min(P, nreq - i) * reqsize for i in range(0, nreq, P)] == [63, 63, 14]
    else:
        assert (P, chunks) == (1, 2)
    dofs = flat(b["dofs"])

    def call(out):
        names = E.launched(lambda: el.evaluate_batch(order, b["pts"], dofs, verts=b["verts"], out=out, route="fused"))
        assert_launched(names, el, order)

    shape = b["ref"][:, :, 0].shape
    fresh = E.compare(call, shape, runtime.Context.get().device)
    check(fresh.cpu().numpy()[:, :, None], b["ref"], case)


@pytest.mark.parametrize("route", ["fused", "general"])
@pytest.mark.parametrize("name", ["lag_tet3", "ned_tri3"])
def test_empty_calls(name, route):
    """No requests or no points, with and without cells and ``out``: the documented shape, ``out`` returned where one was
    given, and no evaluation kernel launched."""
    import torch
    from fiat_amd import runtime
    el = element(name)
    sd, _, vs, _, ndof = facts(el)
    device = runtime.Context.get().device
    for nreq, npts in ((0, 5), (3, 0), (0, 0)):
        for nrhs in (None, 2):
            for with_verts in (False, True):
                for with_out in (False, True):
                    pts = np.zeros((nreq, npts, sd))
                    dofs = np.ones((nreq, ndof) if nrhs is None else (nreq, nrhs, ndof))
                    verts = np.broadcast_to(E.ufc_simplex(sd), (nreq, sd + 1, sd)).copy() if with_verts else None
                    shape = (nreq, len(E.jet(sd, 1))) + (() if nrhs is None else (nrhs,)) + vs + (npts,)
                    out = torch.empty(shape, dtype=torch.float64, device=device) if with_out else None
                    res = []
                    names = E.launched(lambda: res.append(el.evaluate_batch(1, pts, dofs, verts=verts, out=out,
                                                                            pushforward=with_verts and pushes(name), route=route)))
                    assert not [n for n in names if "eval_kernel" in n], names
                    assert tuple(res[0].shape) == shape and res[0].dtype == torch.float64 and res[0].device == device
                    assert res[0].numel() == 0
                    if with_out:
                        assert res[0] is out
