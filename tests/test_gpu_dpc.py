"""DPC elements on the GPU: every instance of the closed-form kernel against the NumPy restatement
(tests/dpc_reference.py) and the reference's fixtures (tests/golden/dpc.npz), the tiling edges of the kernel, the general
route, and the facade.  Tolerances, in the norm max|x - ref| / max(1, max|ref|): against the restatement the project's
standing 1e-12 on values and 1e-10 on derivatives; against the fixtures dpc_reference.fixture_tol (the reference loses
digits in its Vandermonde solve from degree 6 on, see tests/test_dpc_host.py); between the two routes 1e-10, because the
general route inherits the Vandermonde's conditioning."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import dpc_reference as R  # noqa: E402
import edge_reference as E  # noqa: E402  (guarded outputs, request samples)
import make_golden_dpc as M  # noqa: E402

G = np.load(os.path.join(HERE, "golden", "dpc.npz"))
SD = {"quad": 2, "hex": 3, "prod": 2}
TABLES = sorted(n for n, c in M.CASES.items() if c[2] is not None)
ROUTE_TOL = 1e-10
_ELS = {}


def element(name):
    import fiat_amd
    if name not in _ELS:
        _ELS[name] = M.build(fiat_amd, name)
    return _ELS[name]


def unit(sd, k):
    """DPC_k on the UFC quadrilateral / hexahedron."""
    import fiat_amd
    from fiat_amd import reference_element
    key = ("unit", sd, k)
    if key not in _ELS:
        _ELS[key] = fiat_amd.DPC(reference_element.ufc_hypercube(sd), k)
    return _ELS[key]


def rel_check(got, ref, what="", tol=R.STANDING):
    """Per request: (ntab, ndof, npts) tables, values and derivatives apart."""
    got, ref = np.asarray(got, dtype=float), np.asarray(ref, dtype=float)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    for r in range(len(ref)):
        e0 = R.rel_err(got[r, :1], ref[r, :1])
        e1 = R.rel_err(got[r, 1:], ref[r, 1:]) if ref.shape[1] > 1 else 0.0
        assert e0 <= tol[0], (what, r, "values", e0)
        assert e1 <= tol[1], (what, r, "derivatives", e1)


def stack(tab, sd, order):
    from fiat_amd import mis
    return np.stack([tab[a] for k in range(order + 1) for a in mis(sd, k)])


def instance(sd, k, order):
    return f"fxk::dpc_kernel<{sd},{k},{order}>"


def run(sd, k, order, npts, nreq, rng, sample=None, route=None, lo=-0.1, hi=1.1, **kw):
    """``nreq`` requests with points in [lo, hi]^sd on the unit cube, ``sample`` (default: all) against the restatement;
    ``route``: "image" / "stream", asserted with the instance's name."""
    import torch
    el = unit(sd, k)
    name = el.kernel(order, npts)
    assert name.startswith(instance(sd, k, order) + " "), name
    if route is not None:
        assert f" {route} " in name, name
    pts = rng.uniform(lo, hi, size=(nreq, npts, sd))
    out = el.tabulate_batch(order, pts, **kw)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (nreq, len(R.mis(sd, order)), R.ndof(sd, k), npts) == el.out_shape(order, nreq, npts)
    idx = np.arange(nreq) if sample is None else sample
    got = out[torch.as_tensor(idx, device=out.device)].cpu().numpy()
    rel_check(got, R.tabulate(sd, k, order, pts[idx]), (sd, k, order, npts, nreq))
    assert bool(torch.isfinite(out).all())
    return out


def requests_per_item(sd, k, order, npts):
    """P of the route report."""
    return int(unit(sd, k).kernel(order, npts).rsplit("P=", 1)[1])


def route_of(sd, k, order, npts):
    return unit(sd, k).kernel(order, npts).split()[1]


# ---- parity --------------------------------------------------------------------------------------------------------------

SPEC = [(sd, k, order) for sd in (2, 3) for k in range(1, 7) for order in range(3)]


@pytest.mark.parametrize("sd,k,order", SPEC)
def test_compile_time_instances(sd, k, order):
    """Every compile-time instance on its image route (3 points: the largest request is 20 KB) with a partial last item, and
    streaming (64 points) where that exceeds the image."""
    P = requests_per_item(sd, k, order, 3)
    run(sd, k, order, 3, 2 * P + 1, np.random.default_rng(sd * 100 + k * 10 + order), route="image")
    if route_of(sd, k, order, 64) == "stream":
        run(sd, k, order, 64, 3, np.random.default_rng(k), route="stream")


@pytest.mark.parametrize("name", TABLES)
def test_tabulate_against_fixture(name):
    kind, k, order = M.CASES[name]
    el = element(name)
    sd = SD[kind]
    direct = 1 <= k <= 6 and order <= 2
    assert ("dpc_kernel" in el.kernel(order, len(G[f"{name}_pts"]))) == direct
    pts, ref = G[f"{name}_pts"], G[f"{name}_tab"]
    tab = el.tabulate(order, pts)
    from fiat_amd import mis
    assert list(tab) == [a for o in range(order + 1) for a in mis(sd, o)]
    rel_check(stack(tab, sd, order)[None], ref[None], name, R.fixture_tol(k))
    # the batch form: request 0 = the fixture's points, request 1 = the same points reversed
    dev = el.tabulate_batch(order, np.stack([pts, pts[::-1]])).cpu().numpy()
    rel_check(dev, np.stack([ref, ref[..., ::-1]]), name, R.fixture_tol(k))
    if direct:
        # and the restatement at the same points, at the standing tolerances
        rel_check(dev[:1], R.tabulate(sd, k, order, pts)[None], name)


# ---- tiling edges ------------------------------------------------------------------------------------------------------

POINT_COUNTS = [1, 9, 27, 63, 64, 65, 130]              # P = 64, 7, 2, 1, 1, then chunks of 64 with a partial last one
POINT_ELEMENTS = [(2, 2, 1), (3, 3, 1), (2, 5, 2), (3, 6, 2)]     # image and streaming by size


@pytest.mark.parametrize("npts", POINT_COUNTS)
@pytest.mark.parametrize("sd,k,order", POINT_ELEMENTS)
def test_point_counts(sd, k, order, npts):
    """Every point count with a whole, a partial and several items: nreq in {1, P, P + 1, 3 P + 2}."""
    P = requests_per_item(sd, k, order, npts)
    for nreq in sorted({1, P, P + 1, 3 * P + 2}):
        run(sd, k, order, npts, nreq, np.random.default_rng(npts * 13 + nreq))


def test_requests_per_item_of_the_point_counts():
    """DPC_1 quadrilateral values, 24 bytes per point: P = 64 // npts, one request in chunks beyond 64 points."""
    assert [requests_per_item(2, 1, 0, n) for n in POINT_COUNTS] == [64, 7, 2, 1, 1, 1, 1]
    assert route_of(2, 1, 0, 130) == "image" and route_of(3, 6, 2, 130) == "stream"


@pytest.mark.parametrize("sd,k,order", [(3, 6, 2), (3, 3, 1), (2, 6, 2), (2, 3, 0)])
def test_image_boundary(sd, k, order):
    """The last point count whose request leaves through the image and the first one that streams, as fx_dpc_kernel
    reports them."""
    routes = [route_of(sd, k, order, n) for n in range(1, 2000)]
    first_stream = routes.index("stream") + 1
    assert first_stream > 1 and set(routes[:first_stream - 1]) == {"image"} and set(routes[first_stream - 1:]) == {"stream"}
    below, above = first_stream - 1, first_stream
    for npts, route in ((below, "image"), (above, "stream")):
        P = requests_per_item(sd, k, order, npts)
        run(sd, k, order, npts, 2 * P + 1, np.random.default_rng(npts), route=route)


def test_shrunk_items():
    """Requests of which 64 // npts do not fit the image together: the item shrinks to those that do."""
    for sd, k, order, npts in [(3, 3, 2, 8), (3, 2, 2, 8), (2, 5, 2, 9), (3, 4, 1, 8)]:
        P = requests_per_item(sd, k, order, npts)
        assert 1 <= P < 64 // npts
        for nreq in sorted({1, P, P + 1, 3 * P + 2}):
            run(sd, k, order, npts, nreq, np.random.default_rng(nreq), route="image")


@pytest.mark.parametrize("sd,k,order,npts,nreq", [(2, 4, 0, 3, 5), (2, 5, 1, 7, 12), (3, 4, 0, 1, 49), (2, 4, 1, 5, 7)])
def test_odd_totals(sd, k, order, npts, nreq):
    """Items of an odd number of doubles: the 8-byte copy loop instead of the 16-byte flush."""
    P = requests_per_item(sd, k, order, npts)
    reqsize = len(R.mis(sd, order)) * R.ndof(sd, k) * npts
    assert (min(P, nreq) * reqsize) % 2 == 1 or (nreq % P) * reqsize % 2 == 1
    run(sd, k, order, npts, nreq, np.random.default_rng(nreq), route="image")


OFFSET_SHAPES = [(2, 2, 1, 9, 1), (3, 3, 1, 27, 1), (2, 4, 0, 3, 1), (3, 6, 2, 64, 1), (2, 2, 1, 9, 16), (3, 2, 2, 8, 7)]


@pytest.mark.parametrize("sd,k,order,npts,offset", OFFSET_SHAPES)
def test_offset_out_with_guard_bands(sd, k, order, npts, offset):
    """An out= view at an 8-byte offset (and one on a line boundary, one 56 bytes into a line): guards untouched, every entry
    written, equal to a fresh out and to the restatement."""
    import torch
    el = unit(sd, k)
    P = requests_per_item(sd, k, order, npts)
    for nreq in (P, 3 * P + 1):
        pts = np.random.default_rng(npts + nreq).uniform(-0.1, 1.1, size=(nreq, npts, sd))
        fresh = el.tabulate_batch(order, pts)
        buf, out = E.guarded_out(tuple(fresh.shape), offset, fresh.device)
        assert el.tabulate_batch(order, pts, out=out) is out
        torch.cuda.synchronize()
        E.check_guarded(buf, out)
        assert torch.equal(out, fresh)
        rel_check(out.cpu().numpy(), R.tabulate(sd, k, order, pts), (sd, k, nreq))


def test_non_default_stream():
    import torch
    s = torch.cuda.Stream()
    for sd, k, order, npts, nreq in [(2, 3, 2, 9, 30), (3, 6, 2, 64, 3)]:
        el = unit(sd, k)
        pts = np.random.default_rng(npts).uniform(size=(nreq, npts, sd))
        dev = torch.as_tensor(pts).cuda()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            out = el.tabulate_batch(order, dev, stream=s)
        s.synchronize()
        rel_check(out.cpu().numpy(), R.tabulate(sd, k, order, pts), (sd, k, "stream"))


@pytest.mark.parametrize("sd,k", [(2, 6), (3, 6), (3, 2)])
def test_points_outside_the_cell(sd, k):
    """Up to 0.2 outside the cell on every side (the hexahedron's mapped simplex does not cover the cell either)."""
    run(sd, k, 2, 13, 11, np.random.default_rng(k), lo=-0.2, hi=1.2)


def test_grid_stride():
    """More items than the grid holds: every workgroup takes several."""
    import torch
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    P = requests_per_item(2, 1, 0, 4)
    nreq = 2 * num_cu * 64 * P + P + 3
    sample = E.sample_requests(nreq, P, nitems_per_trip=num_cu * 64, k=16, seed=4)
    run(2, 1, 0, 4, nreq, np.random.default_rng(nreq), sample=sample)


# ---- the two routes --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sd", [2, 3])
@pytest.mark.parametrize("k", range(1, 7))
def test_routes_agree(sd, k):
    el = unit(sd, k)
    pts = np.random.default_rng(sd * 10 + k).uniform(size=(5, 11, sd))
    direct = el.tabulate_batch(2, pts).cpu().numpy()
    general = el.tabulate_batch(2, pts, route="general").cpu().numpy()
    for r in range(len(pts)):
        e = R.rel_err(general[r], direct[r])
        assert e <= ROUTE_TOL, (sd, k, r, e)
    with pytest.raises(ValueError):
        el.tabulate_batch(2, pts, route="fast")


@pytest.mark.parametrize("name", ["q0", "h0", "q7", "h3o3"])
def test_general_route_against_fixture(name):
    """Degree 0, degree 7 at order 1 and degree 3 at order 3: beyond the direct kernel's instances."""
    kind, k, order = M.CASES[name]
    el = element(name)
    sd = SD[kind]
    pts, ref = G[f"{name}_pts"], G[f"{name}_tab"]
    assert "dpc_kernel" not in el.kernel(order, len(pts))
    names = E.launched(lambda: el.tabulate_batch(order, pts[None]))
    assert names and not [n for n in names if "dpc_kernel" in n], names
    dev = el.tabulate_batch(order, np.stack([pts, pts[::-1]])).cpu().numpy()
    rel_check(dev, np.stack([ref, ref[..., ::-1]]), name, R.fixture_tol(k))
    if k >= 1:
        forced = el.tabulate_batch(order, pts[None], route="general").cpu().numpy()
        assert np.array_equal(forced[0], dev[0])


def test_direct_route_launches_the_instance():
    el = unit(3, 4)
    pts = np.random.default_rng(1).uniform(size=(3, 5, 3))
    names = E.launched(lambda: el.tabulate_batch(1, pts))
    assert [n for n in names if "dpc_kernel<3, 4, 1>" in n.replace(",", ", ").replace(",  ", ", ")], names
    names = E.launched(lambda: el.tabulate_batch(1, pts, route="general"))
    assert names and not [n for n in names if "dpc_kernel" in n], names


# ---- the facade --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(M.CASES))
def test_metadata_nodes_and_coefficients(name):
    kind, k, order = M.CASES[name]
    el = element(name)
    sd = SD[kind]
    ndof = R.ndof(sd, k)
    assert list(M.metadata(el)) == list(G[f"{name}_meta"]) == [k, ndof, sd, k]
    assert el.value_shape() == () and el.mapping() == ["affine"] * ndof and el.space_dimension() == ndof
    assert np.array_equal(M.eids_rows(el.entity_dofs()), G[f"{name}_eids"])
    assert np.array_equal(M.eids_rows(el.entity_closure_dofs()), G[f"{name}_cids"])
    assert set(el.entity_dofs()) == set(el.get_reference_element().get_topology())
    np.testing.assert_allclose(M.node_points(el), G[f"{name}_nodes"], rtol=0, atol=1e-15)
    ref = G[f"{name}_coeffs"]
    assert el.get_coeffs().shape == ref.shape
    assert R.rel_err(el.get_coeffs(), ref) <= ROUTE_TOL         # two LU solves of the same Vandermonde matrix
    assert el.get_nodal_basis().get_coeffs() is el.get_coeffs()
    assert el.get_nodal_basis().get_reference_element().is_simplex()
    assert el.get_reference_element() is el.get_reference_complex() and not el.is_macroelement()
    with pytest.raises(NotImplementedError):
        el.entity_permutations()


# cond_2 of the reference's own Vandermonde matrix (numpy.linalg.cond of FIAT's ``el.V``) where the general route serves the
# element: DPC_7 on the quadrilateral.  (For comparison: 3.2e5 at q6, 1.1e7 at h6.)
GENERAL_ROUTE_COND = {"q7": 4.9e6}


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_nodality(name):
    """Q phi = I at the dual nodes, atol 1e-11, for every element the closed-form kernel (degrees 1-6) or DPC0 serves.
    Degree 7 takes the general route, whose tables come from an LU solve of the Vandermonde matrix: a backward-stable solve
    promises unit roundoff times cond(V) = 1.1e-16 * 4.9e6 = 5.4e-10 there and no more (the reference itself, same matrix, is
    3.5e-12 from the identity at q7 and 3.1e-11 at h6, measured on the CPU), so that is the bound of q7; the device's general
    route measured 7.6e-11."""
    kind, k, _ = M.CASES[name]
    el = element(name)
    nodes = M.node_points(el)
    phi = el.tabulate(0, nodes)[(0,) * SD[kind]]
    atol = 1e-11 if name not in GENERAL_ROUTE_COND else 0.5 * np.finfo(float).eps * GENERAL_ROUTE_COND[name]
    err = np.abs(phi - np.eye(len(nodes))).max()
    print(f"{name}: |Q phi - I| = {err:.2e} (atol {atol:.1e})")
    np.testing.assert_allclose(phi, np.eye(len(nodes)), rtol=0, atol=atol)


@pytest.mark.parametrize("name,dim,ent,order", M.ENTITIES)
def test_entity_tabulation(name, dim, ent, order):
    el = element(name)
    kind, k, _ = M.CASES[name]
    sd = SD[kind]
    p, ref = G[f"ent_{name}_{dim}_{ent}_pts"], G[f"ent_{name}_{dim}_{ent}_tab"]
    rel_check(stack(el.tabulate(order, p, entity=(dim, ent)), sd, order)[None], ref[None], (name, dim, ent), R.fixture_tol(k))
    dev = el.tabulate_batch(order, np.stack([p, p[::-1]]), entity=(dim, ent)).cpu().numpy()
    rel_check(dev, np.stack([ref, ref[..., ::-1]]), (name, dim, ent), R.fixture_tol(k))
    general = el.tabulate_batch(order, p[None], entity=(dim, ent), route="general").cpu().numpy()
    assert R.rel_err(general[0], dev[0]) <= ROUTE_TOL
    # the cell itself as the entity: the points as they are
    q = G[f"{name}_pts"]
    assert np.array_equal(stack(el.tabulate(order, q, entity=(sd, 0)), sd, order), stack(el.tabulate(order, q), sd, order))


def test_product_cell():
    """Interval x interval, not flattened: nodes and metadata are the reference's (test_metadata_nodes_and_coefficients),
    entity ids are keyed by the product cell's dimension tuples; the reference's tabulate raises a TypeError there, so the
    tables are checked against the restatement on the flattened cell."""
    el = element("p3")
    assert set(el.entity_dofs()) == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert el.entity_dofs()[(1, 1)] == {0: list(range(10))} and el.entity_closure_dofs()[(1, 1)] == {0: list(range(10))}
    assert all(dofs == [] for dim in [(0, 0), (0, 1), (1, 0)] for dofs in el.entity_dofs()[dim].values())
    pts = np.random.default_rng(7).uniform(-0.1, 1.1, size=(3, 10, 2))
    assert el.kernel(2, 10).startswith("fxk::dpc_kernel<2,3,2> ")
    rel_check(el.tabulate_batch(2, pts).cpu().numpy(), R.tabulate(2, 3, 2, pts), "p3")
    rel_check(stack(el.tabulate(1, pts[0]), 2, 1)[None], R.tabulate(2, 3, 1, pts[:1]), "p3")
    # an edge of the product cell: x = 1
    xi = np.random.default_rng(8).uniform(size=(1, 6, 1))
    on_edge = np.concatenate([np.ones_like(xi), xi], axis=-1)
    rel_check(el.tabulate_batch(1, xi, entity=((0, 1), 1)).cpu().numpy(), R.tabulate(2, 3, 1, on_edge), "p3 edge")


def test_constructor_as_the_reference():
    import fiat_amd
    from fiat_amd import discontinuous_pc, reference_element
    assert fiat_amd.supported_elements["DPC"] is fiat_amd.DPC is discontinuous_pc.DPC
    assert isinstance(unit(2, 0), discontinuous_pc.DPC0) and isinstance(unit(3, 2), discontinuous_pc.HigherOrderDPC)
    assert isinstance(unit(2, 3).get_dual_set(), discontinuous_pc.DPCDualSet)
    assert discontinuous_pc.hypercube_simplex_map[reference_element.UFCHexahedron()] == reference_element.UFCTetrahedron()
    for cell in (fiat_amd.UFCInterval(), reference_element.Point(), fiat_amd.ufc_simplex(2), fiat_amd.ufc_simplex(3)):
        for k in (0, 2):
            with pytest.raises(NotImplementedError):
                fiat_amd.DPC(cell, k)
    # a product that does not flatten to a UFC cell: the reference's KeyError (recorded in the fixture)
    assert list(G["b2_keyerror"]) == [1]
    with pytest.raises(KeyError):
        M.build(fiat_amd, "b2")


def test_no_per_request_cells():
    el = unit(2, 2)
    pts = np.random.default_rng(0).uniform(size=(3, 4, 2))
    with pytest.raises(NotImplementedError):
        el.tabulate_batch(1, pts, verts=np.zeros((3, 3, 2)))
    with pytest.raises(NotImplementedError):
        el.tabulate_cells(1, pts[0], np.zeros((3, 3, 2)))
    with pytest.raises(ValueError):
        el.tabulate_batch(1, np.zeros((3, 4, 3)))
    # pushforward changes nothing
    import torch
    assert torch.equal(el.tabulate_batch(1, pts, pushforward=True), el.tabulate_batch(1, pts))


def test_finat_adapter_accepts_the_element():
    from fiat_amd import finat_adapter as ad
    el = unit(3, 3)
    fe = ad.FiatElement(el)
    pts = np.random.default_rng(5).uniform(size=(2, 6, 3))
    ref = R.tabulate(3, 3, 2, pts)
    res = fe.basis_evaluation(2, ad.PointSet(pts[0]))
    bres = fe.basis_evaluation_batch(2, pts)
    for t, alpha in enumerate(R.mis(3, 2)):
        tol = R.STANDING[0] if t == 0 else R.STANDING[1]
        assert R.rel_err(res[alpha].array.reshape(20, 6), ref[0, t]) <= tol
        assert R.rel_err(bres[alpha].array.cpu().numpy(), ref[:, t]) <= tol
    assert fe.space_dimension() == 20 and fe.formdegree == 3 and fe.degree == 3
    # every basis function is supported on every facet's closure or none: the cell owns all dofs
    assert fe.entity_dofs()[3][0] == list(range(20))
