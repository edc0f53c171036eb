"""Bernstein kernels (csrc/bernstein.hpp, launcher bernstein.hip) at their tiling edges, against the long-double definition
of tests/edge_reference.py: every compile-time instance; the generic instance at high degrees and orders, with per-request
cells and on the shared route; point counts around 64 (P = 64 / npts whole requests per item, one request in chunks of 64
points beyond); items at the LDS image limit and above; odd item sizes (the scalar copy loop); grids that the items
exceed (the grid-stride loop); and exact properties.  Norm max|x - ref| / max(1, max|ref|): 1e-12 values, 1e-10
derivatives.  The shape lists are those of tests/edge_reference.py; tests/test_edge_reference_host.py runs them through
the launcher mirror and checks that together they reach every route category."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edge_reference as R  # noqa: E402

TOL_VAL, TOL_DER = 1e-12, 1e-10

# the shape lists live in edge_reference.py, where the host test runs them through the launcher mirror
CENSUS, GENERIC_OWN, GENERIC_CELLS = R.BERN_CENSUS, R.BERN_GENERIC_OWN, R.BERN_GENERIC_CELLS
POINT_COUNTS, POINT_SHAPES = R.POINT_COUNTS, R.BERN_POINT_SHAPES
IMAGE_EDGE, ODD_SHAPES = R.BERN_IMAGE_EDGE, R.BERN_ODD_SHAPES
nreq_list, grid_stride_cases, inside, cells = R.nreq_list, R.bern_grid_stride_cases, R.simplex_points, R.random_cells


# ---------------------------------------------------------------------------------------------------------------------

def rel_check(got, ref, what=""):
    """got, ref (nreq, ntab, ndof, npts): the suite's norm per request, values and derivatives apart."""
    got, ref = np.asarray(got, dtype=float), np.asarray(ref, dtype=float)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    for r in range(len(ref)):
        e0 = np.abs(got[r, 0] - ref[r, 0]).max() / max(1.0, np.abs(ref[r, 0]).max())
        assert e0 <= TOL_VAL, (what, r, "values", e0)
        if ref.shape[1] > 1:
            e1 = np.abs(got[r, 1:] - ref[r, 1:]).max() / max(1.0, np.abs(ref[r, 1:]).max())
            assert e1 <= TOL_DER, (what, r, "derivatives", e1)


_ELS = {}


def element(sd, n):
    from fiat_amd import Bernstein, ufc_simplex
    if (sd, n) not in _ELS:
        _ELS[(sd, n)] = Bernstein(ufc_simplex(sd), n)
    return _ELS[(sd, n)]


def run(sd, n, order, npts, nreq, mode, rng, sample=None, lo=-0.05):
    """Tabulate on the device in ``mode`` ("own", "cells", "shared"), compare ``sample`` requests with the reference."""
    import torch
    el = element(sd, n)
    if mode == "own":
        pts = inside(rng, (nreq, npts), sd, lo)
        out = el.tabulate_batch(order, pts)
        verts = None
    elif mode == "cells":
        verts = cells(rng, nreq, sd)
        pts = np.einsum("rpv,rvd->rpd", np.concatenate([1 - (x := inside(rng, (nreq, npts), sd, lo)).sum(-1, keepdims=True), x], -1), verts)
        out = el.tabulate_batch(order, pts, verts=verts)
    else:
        verts = cells(rng, nreq, sd)
        pts = inside(rng, (npts,), sd, lo)
        out = el.tabulate_cells(order, pts, verts)
    torch.cuda.synchronize()
    idx = np.arange(nreq) if sample is None else sample
    got = out[torch.as_tensor(idx, device=out.device)].cpu().numpy()
    if mode == "shared":
        ref = R.bernstein_reference(sd, n, order, pts, verts=verts[idx], shared=True)
    else:
        ref = R.bernstein_reference(sd, n, order, pts[idx], verts=None if verts is None else verts[idx])
    rel_check(got, ref, (sd, n, order, npts, nreq, mode))
    return out


@pytest.mark.parametrize("sd,n,order,npts,nreq", CENSUS, ids=[f"s{c[0]}n{c[1]}o{c[2]}" for c in CENSUS])
def test_instance_census(sd, n, order, npts, nreq):
    r = R.bern_route(sd, n, order, npts, False, nreq, R.MI355X_CU)
    assert r["spec"] and r["last_partial"] and r["P"] * npts < 64
    run(sd, n, order, npts, nreq, "own", np.random.default_rng(sd * 100 + n * 10 + order))


@pytest.mark.parametrize("sd,n,order,npts,nreq", GENERIC_OWN, ids=[f"s{c[0]}n{c[1]}o{c[2]}" for c in GENERIC_OWN])
def test_generic_own_cell(sd, n, order, npts, nreq):
    r = R.bern_route(sd, n, order, npts, False, nreq, R.MI355X_CU)
    assert not r["spec"]
    sample = R.sample_requests(nreq, r["P"], k=4, seed=n)
    run(sd, n, order, npts, nreq, "own", np.random.default_rng(n * 10 + order + sd), sample=sample)


@pytest.mark.parametrize("sd,n,order,npts,mode", GENERIC_CELLS, ids=[f"s{c[0]}n{c[1]}o{c[2]}p{c[3]}{c[4]}" for c in GENERIC_CELLS])
def test_generic_cells_and_shared(sd, n, order, npts, mode):
    r = R.bern_route(sd, n, order, npts, True, 1, R.MI355X_CU)
    assert not r["spec"]
    nreq = 3 * r["P"] + 2
    run(sd, n, order, npts, nreq, mode, np.random.default_rng(7 * npts + order + sd))


@pytest.mark.parametrize("mode", ["own", "cells", "shared"])
@pytest.mark.parametrize("npts", POINT_COUNTS)
@pytest.mark.parametrize("sd,n,order", POINT_SHAPES, ids=["spec", "generic"])
def test_point_counts(sd, n, order, npts, mode):
    P = R.bern_route(sd, n, order, npts, mode != "own", 1, R.MI355X_CU)["P"]
    for nreq in nreq_list(P):
        run(sd, n, order, npts, nreq, mode, np.random.default_rng(npts * 31 + nreq))


@pytest.mark.parametrize("sd,n,order,npts", IMAGE_EDGE + ODD_SHAPES)
def test_image_boundary_and_odd_items(sd, n, order, npts):
    r = R.bern_route(sd, n, order, npts, False, 1, R.MI355X_CU)
    assert r["spec"] and r["image"] == (r["item_bytes"] <= R.C["BERN_IMAGE_BYTES"])
    for nreq in (r["P"], 3 * r["P"] + 1):
        run(sd, n, order, npts, nreq, "own", np.random.default_rng(npts + nreq))


def test_grid_stride():
    import torch
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    for sd, n, order, npts, mode, nreq in grid_stride_cases(num_cu):
        r = R.bern_route(sd, n, order, npts, mode != "own", nreq, num_cu)
        assert r["nitems"] >= 2 * r["gridcap"]
        sample = R.sample_requests(nreq, r["P"], nitems_per_trip=r["grid"], k=16, seed=npts)
        out = run(sd, n, order, npts, nreq, mode, np.random.default_rng(nreq), sample=sample)
        assert not bool(torch.isnan(out).any())
        if order == 0 and mode == "own":
            assert float((out[:, 0].sum(1) - 1).abs().max()) < 1e-13          # every request: partition of unity
        del out


# ---------------------------------------------------------------------------------------------------------------------
# exact properties

@pytest.mark.parametrize("sd,n", [(1, 4), (2, 3), (3, 6), (2, 9), (3, 12)])
def test_vertices_are_kronecker(sd, n):
    import torch
    el = element(sd, n)
    V = R.ufc_simplex(sd)
    out = el.tabulate_batch(1, np.repeat(V[None], 3, 0))[:, 0]            # (3, ndof, sd+1)
    want = torch.zeros_like(out)
    ks = R.multi_indices(sd + 1, n)
    for v in range(sd + 1):
        want[:, ks.index(tuple(n if i == v else 0 for i in range(sd + 1))), v] = 1.0
    assert torch.equal(out, want)


@pytest.mark.parametrize("sd,n,order", [(1, 1, 2), (2, 0, 2), (3, 1, 2), (2, 2, 5), (3, 3, 8), (1, 5, 8)])
def test_order_above_degree_is_exactly_zero(sd, n, order):
    el = element(sd, n)
    out = el.tabulate_batch(order, inside(np.random.default_rng(n), (5, 9), sd, -0.2))
    assert bool((out[:, R.ntables(sd, n):] == 0).all())
    assert bool((out[:, :R.ntables(sd, n)] != 0).any())


@pytest.mark.parametrize("sd,n", [(1, 2), (2, 2), (3, 2), (1, 8), (2, 5), (3, 4)])
def test_order_equal_degree_is_the_exact_constant(sd, n):
    """On the UFC cell G holds 0 / +-1: the order-n tables are integers (sums of products of +-1 and n!), exact in fp64."""
    import torch
    el = element(sd, n)
    x = inside(np.random.default_rng(n + sd), (1, 1), sd)[0, 0]
    ex = R.bernstein_exact(sd, n, n, x)
    t0 = R.ntables(sd, n - 1)
    want = np.array([[float(v) for v in row] for row in ex[t0:]])
    assert all(v.denominator == 1 and abs(v) < 2 ** 53 for row in ex[t0:] for v in row)
    out = el.tabulate_batch(n, inside(np.random.default_rng(sd), (4, 6), sd, -0.3))[:, t0:]
    assert torch.equal(out, torch.as_tensor(want, device=out.device)[None, :, :, None].expand_as(out).contiguous())


@pytest.mark.parametrize("mode", ["own", "cells", "shared"])
@pytest.mark.parametrize("sd,n,order", [(2, 4, 2), (3, 9, 3)])
def test_points_outside_the_cell(sd, n, order, mode):
    run(sd, n, order, 13, 11, mode, np.random.default_rng(sd + n + order), lo=-0.5)
