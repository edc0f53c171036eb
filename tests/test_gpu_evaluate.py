"""``evaluate_batch`` on the GPU: every instance of the fused evaluation kernel against the NumPy restatement
(tests/evaluate_reference.py), every case of the reference's fixture (tests/golden/evaluate.npz) on both routes and both cells,
the tiling edges, right-hand sides, special inputs and the refusals.  Tolerances, in the norm max|x - ref| / max(1, max|ref|):
the project's standing 1e-12 on values and 1e-10 on derivatives, everywhere.  Every fused call is asserted to have launched
exactly the named instance and writes into a guarded output."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import edge_reference as E  # noqa: E402  (guarded outputs, request samples, profiler records)
import evaluate_reference as R  # noqa: E402
import make_golden_evaluate as M  # noqa: E402
from evaluate_gpu_common import (G, STANDING, as3, assert_launched, check, element, expected_plan, facts, fused,  # noqa: E402
                                 inputs, instance, restated)


# ---- parity --------------------------------------------------------------------------------------------------------------

# one element per (sd, vdim): the instance is (sd, order, vdim)
INSTANCE_ELEMENTS = {(1, 1): "leg_int3", (2, 1): "lag_tri3", (2, 2): "ned_tri3", (3, 1): "lag_tet3", (3, 3): "ned_tet2"}


@pytest.mark.parametrize("order", [0, 1, 2])
@pytest.mark.parametrize("sd,vdim", sorted(INSTANCE_ELEMENTS))
def test_compile_time_instances(sd, vdim, order):
    """Every compile-time instance once: 7 points (9 requests per item) and 13 requests leave a partial last item and an odd
    total; all requests against the restatement."""
    el = element(INSTANCE_ELEMENTS[(sd, vdim)])
    assert facts(el)[0] == sd and facts(el)[3] == vdim
    pts, dofs = inputs(el, 7, 13, np.random.default_rng(100 * sd + 10 * vdim + order))
    assert el.evaluate_kernel(order, 7).startswith(f"fused: fxk::{instance(el, order)} ")
    out = fused(el, order, pts, dofs).cpu().numpy()
    check(out[:, :, None], restated(el, order, pts, as3(dofs)), (sd, vdim, order))


@pytest.mark.parametrize("physical", [False, True], ids=["own", "physical"])
@pytest.mark.parametrize("name", sorted(M.CASES))
def test_fixture_cases(name, physical):
    """Every fixture case on both routes, on the element's own cell and on the skewed physical cell (the Piola families pushed
    forward), against the reference's own contraction; the two routes against each other, all at the standing tolerances."""
    import torch
    el = element(name)
    sd = facts(el)[0]
    order = M.ORDER
    pts = G[f"{name}_ppts" if physical else f"{name}_pts"][None]
    verts = G[f"{name}_verts"][None] if physical else None
    dofs = G[f"{name}_dofs"][None]
    ref = G[f"{name}_pref" if physical else f"{name}_ref"][None]
    assert [el.degree(), el.space_dimension(), sd] == list(G[f"{name}_meta"][:3])
    assert R.error(el.get_coeffs(), G[f"{name}_coeffs"]) <= STANDING[1]
    kw = dict(verts=verts, pushforward=physical)
    general = el.evaluate_batch(order, pts, dofs, route="general", **kw)
    names = E.launched(lambda: el.evaluate_batch(order, pts, dofs, route="general", **kw))
    assert names and not [n for n in names if "eval_kernel" in n], names
    check(general.cpu().numpy(), ref, (name, "general"))
    report = el.evaluate_kernel(order, pts.shape[1], nrhs=M.NRHS, has_verts=physical, pushforward=physical)
    if name in M.GENERAL_ONLY:
        assert report.startswith("general: "), report
        names = E.launched(lambda: el.evaluate_batch(order, pts, dofs, **kw))
        assert names and not [n for n in names if "eval_kernel" in n], names
        assert torch.equal(el.evaluate_batch(order, pts, dofs, **kw), general)
        with pytest.raises(NotImplementedError):
            el.evaluate_batch(order, pts, dofs, route="fused", **kw)
        return
    assert report.startswith(f"fused: fxk::{instance(el, order)} "), report
    out = fused(el, order, pts, dofs, **kw)
    check(out.cpu().numpy(), ref, (name, "fused"))
    check(out.cpu().numpy(), general.cpu().numpy(), (name, "fused against general"))
    names = E.launched(lambda: el.evaluate_batch(order, pts, dofs, **kw))      # route=None picks the fused kernel
    assert_launched(names, el, order)


# ---- tiling edges --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("npts", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("name", ["lag_tri2", "lag_tet3"])
def test_tiling_edges(name, npts):
    """One lane per request, the wave boundary and point-chunked requests; one request, exactly one item, one request more
    than a workgroup takes in its first item, and enough for every workgroup of the grid to take a second item."""
    import torch
    el = element(name)
    sd, n, _, vdim, ndof = facts(el)
    order = 1
    P, chunks = expected_plan(sd, n, order, vdim, ndof, npts)
    assert (P, chunks) == {("lag_tri2", 1): (64, 1), ("lag_tet3", 1): (45, 1)}.get((name, npts), (1, -(-npts // 64)))
    assert el.evaluate_kernel(order, npts) == f"fused: fxk::{instance(el, order)} degree={n} P={P} chunks={chunks}"
    grid = torch.cuda.get_device_properties(0).multi_processor_count * 32        # workgroups at most
    per_item = P if chunks == 1 else 1
    second_trip = -(-(2 * grid) // chunks) * per_item + 1                       # items >= 2 * grid, and an odd total
    for nreq in sorted({1, per_item, per_item + 1, second_trip}):
        pts, dofs = inputs(el, npts, nreq, np.random.default_rng(npts * 7 + nreq))
        out = fused(el, order, pts, dofs)
        assert bool(torch.isfinite(out).all())
        sample = E.sample_requests(nreq, per_item, nitems_per_trip=grid if chunks == 1 else max(1, grid // chunks), k=6, seed=npts)
        got = out[torch.as_tensor(sample, device=out.device)].cpu().numpy()
        check(got[:, :, None], restated(el, order, pts[sample], as3(dofs[sample])), (name, npts, nreq))


# ---- right-hand sides ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,order,npts,nreq,physical", [("lag_tet3", 1, 23, 5, False), ("ned_tri3", 2, 9, 8, True),
                                                         ("lag_tri2", 1, 70, 3, False)])
def test_right_hand_sides(name, order, npts, nreq, physical):
    """nrhs 1 (2-D and 3-D dofs), 3 and 8: every right-hand side is the single-rhs call on that slice bit for bit, and two
    identical calls are bitwise equal."""
    import torch
    el = element(name)
    rng = np.random.default_rng(npts)
    pts, dofs = inputs(el, npts, nreq, rng, nrhs=8, lo=0.0, hi=0.5)
    kw = {}
    if physical:
        verts = E.random_cells(rng, nreq, facts(el)[0])
        B = np.swapaxes(verts[:, 1:] - verts[:, :1], 1, 2)
        pts = np.einsum("rde,rpe->rpd", B, pts) + verts[:, :1]
        kw = dict(verts=verts, pushforward=True)
    single = [fused(el, order, pts, np.ascontiguousarray(dofs[:, j]), **kw) for j in range(8)]
    check(single[0].cpu().numpy()[:, :, None], restated(el, order, pts, dofs[:, :1], **kw), (name, "nrhs 1"))
    flat = fused(el, order, pts, np.ascontiguousarray(dofs[:, :1]), **kw)
    assert flat.shape[2] == 1 and torch.equal(flat[:, :, 0], single[0])
    for nrhs in (3, 8):
        many = fused(el, order, pts, np.ascontiguousarray(dofs[:, :nrhs]), **kw)
        assert many.shape[2] == nrhs
        for j in range(nrhs):
            assert torch.equal(many[:, :, j], single[j]), (nrhs, j)
        again = fused(el, order, pts, np.ascontiguousarray(dofs[:, :nrhs]), offset=0, **kw)
        assert torch.equal(again, many)


# ---- special inputs ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,order", [("lag_tet3", 1), ("rt_tri3", 2)])
def test_unit_vectors_reproduce_rows_of_the_table(name, order):
    el = element(name)
    ndof = facts(el)[4]
    rng = np.random.default_rng(order)
    pts, _ = inputs(el, 11, 4, rng, lo=0.0, hi=0.4)
    rows = [0, 1, ndof // 2, ndof - 1]
    dofs = np.broadcast_to(np.eye(ndof)[rows], (4, len(rows), ndof)).copy()
    out = fused(el, order, pts, dofs).cpu().numpy()
    tables = el.tabulate_batch(order, pts).cpu().numpy()
    check(out, tables[:, :, rows], (name, "unit vectors"))


def test_zero_dofs_give_exact_zeros():
    import torch
    for name, order in (("lag_tet3", 2), ("ned_tet2", 1)):
        el = element(name)
        pts, dofs = inputs(el, 9, 6, np.random.default_rng(3), nrhs=2)
        out = fused(el, order, pts, np.zeros_like(dofs))
        assert int(torch.count_nonzero(out)) == 0


def test_out_is_honoured_and_inputs_may_live_on_the_device():
    import torch
    el = element("lag_tri3")
    pts, dofs = inputs(el, 6, 21, np.random.default_rng(8))
    host = fused(el, 1, pts, dofs)
    dev = fused(el, 1, torch.as_tensor(pts).cuda(), torch.as_tensor(dofs).cuda(), offset=0)
    assert torch.equal(host, dev)
    fresh = el.evaluate_batch(1, pts, dofs)
    assert fresh.is_contiguous() and torch.equal(fresh, host)
    check(host.cpu().numpy()[:, :, None], restated(el, 1, pts, as3(dofs)), "out=")


def test_non_default_stream():
    """The call is ordered on its stream: the inputs are filled on that stream immediately before it."""
    import torch
    el = element("lag_tet3")
    pts, dofs = inputs(el, 23, 40, np.random.default_rng(5))
    src_p, src_d = torch.as_tensor(pts).cuda(), torch.as_tensor(dofs).cuda()
    dev_p = torch.full_like(src_p, float("nan"))
    dev_d = torch.full_like(src_d, float("nan"))
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        dev_p.copy_(src_p, non_blocking=True)
        dev_d.copy_(src_d, non_blocking=True)
        out = el.evaluate_batch(1, dev_p, dev_d, stream=s, route="fused")
    s.synchronize()
    check(out.cpu().numpy()[:, :, None], restated(el, 1, pts, as3(dofs)), "stream")


# ---- refusals ------------------------------------------------------------------------------------------------------------

def refused(exc, call, match=None):
    """``call`` raises ``exc`` and launches nothing."""
    def attempt():
        with pytest.raises(exc, match=match):
            call()
    assert not E.launched(attempt)


def test_refusals_launch_nothing():
    import fiat_amd
    from fiat_amd import finite_element
    el = element("lag_tet3")
    pts, dofs = inputs(el, 5, 4, np.random.default_rng(1))
    ndof = facts(el)[4]
    verts = E.random_cells(np.random.default_rng(2), 4, 3)
    refused(ValueError, lambda: el.evaluate_batch(1, pts, dofs[:, :-1]), "dofs must have shape")
    refused(ValueError, lambda: el.evaluate_batch(1, pts, dofs[:3]), "dofs must have shape")
    refused(ValueError, lambda: el.evaluate_batch(1, pts, dofs.reshape(4, 1, 1, ndof)), "dofs must have shape")
    refused(ValueError, lambda: el.evaluate_batch(1, pts, dofs.astype(np.float32)), "float64")
    refused(ValueError, lambda: el.evaluate_batch(1, pts, np.zeros((4, 9, ndof))), "right-hand sides")
    refused(ValueError, lambda: el.evaluate_batch(1, pts, dofs, pushforward=True), "push-forward")
    refused(ValueError, lambda: el.evaluate_batch(1, pts[..., :2], dofs), "points must have shape")
    refused(ValueError, lambda: el.evaluate_batch(1, pts, dofs, verts=verts[:, :3]), "verts must have shape")
    refused(ValueError, lambda: el.evaluate_batch(1, pts, dofs, route="fast"), "unknown route")
    refused(ValueError, lambda: el.evaluate_batch(-1, pts, dofs), "negative")
    refused(NotImplementedError, lambda: el.evaluate_batch(3, pts, dofs, route="fused"), "order 3")
    p7 = element("lag_tri7")
    p2, d7 = inputs(p7, 5, 4, np.random.default_rng(3))
    refused(NotImplementedError, lambda: p7.evaluate_batch(1, p2, d7, route="fused"), "degree 7")
    regge = element("regge_tri1")
    _, dr = inputs(regge, 5, 4, np.random.default_rng(4))
    refused(NotImplementedError, lambda: regge.evaluate_batch(1, p2, dr, route="fused"), "value shape")
    line = fiat_amd.Lagrange(fiat_amd.ufc_simplex(1), 2)
    quad = fiat_amd.TensorProductElement(line, line)
    dq = np.zeros((4, quad.space_dimension()))
    refused(NotImplementedError, lambda: finite_element.evaluate_batch(quad, 1, p2, dq, route="fused"), "TensorProductElement")
    _, dl = inputs(line, 5, 4, np.random.default_rng(5))
    refused(NotImplementedError, lambda: line.evaluate_batch(1, p2[..., :1], dl, route="fused"), "1-D primal")


def test_wrong_out_is_refused():
    import torch
    el = element("lag_tet3")
    pts, dofs = inputs(el, 5, 4, np.random.default_rng(1))
    good = el.evaluate_batch(1, pts, dofs)
    bad = [torch.empty(good.shape[:-1] + (6,), dtype=torch.float64, device=good.device),
           torch.empty(good.shape, dtype=torch.float32, device=good.device),
           torch.empty(good.shape[:-1] + (10,), dtype=torch.float64, device=good.device)[..., ::2],
           torch.empty(good.shape, dtype=torch.float64)]
    for out in bad:
        for route in ("fused", "general"):
            refused(ValueError, lambda: el.evaluate_batch(1, pts, dofs, out=out, route=route), "out must be")


def test_general_route_of_other_elements():
    """The general route serves what has ``tabulate_batch``: the 1-D Lagrange element and a tensor-product element."""
    import fiat_amd
    from fiat_amd import finite_element
    line = fiat_amd.Lagrange(fiat_amd.ufc_simplex(1), 2)
    quad = fiat_amd.TensorProductElement(line, line)
    rng = np.random.default_rng(6)
    for el, sd in ((line, 1), (quad, 2)):
        pts = rng.uniform(size=(3, 5, sd))
        dofs = rng.uniform(-1, 1, size=(3, 2, el.space_dimension()))
        got = finite_element.evaluate_batch(el, 1, pts, dofs).cpu().numpy()
        tab = el.tabulate_batch(1, pts).cpu().numpy()
        ref = np.einsum("rji,rtip->rtjp", dofs, tab)
        check(got, ref, type(el).__name__)
