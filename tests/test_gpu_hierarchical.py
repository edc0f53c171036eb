"""IntegratedLegendre on the GPU: every instance of the direct C0-hierarchy kernel against the NumPy restatement
(tests/hierarchical_reference.py) and the reference's fixtures (tests/golden/hierarchical.npz), the tiling edges of the
kernel, the general route, and the facade.  Tolerances, in the norm max|x - ref| / max(1, max|ref|): the project's standing
1e-12 on values and 1e-10 on derivatives against the restatement and against the fixtures; between the two routes 1e-10,
because the general route goes through the Vandermonde solve."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import edge_reference as E  # noqa: E402  (guarded outputs, request samples, profiler records)
import hierarchical_reference as R  # noqa: E402
import make_golden_hierarchical as M  # noqa: E402

G = np.load(os.path.join(HERE, "golden", "hierarchical.npz"))
SD = {"int": 1, "tri": 2, "tet": 3}
STANDING = (1e-12, 1e-10)
ROUTE_TOL = 1e-10
_ELS = {}


def element(name):
    import fiat_amd
    if name not in _ELS:
        _ELS[name] = M.build(fiat_amd, name)
    return _ELS[name]


def unit(sd, k):
    """IntegratedLegendre(k) on the UFC simplex of dimension sd (the fixture's element of that degree)."""
    return element(("int", "tri", "tet")[sd - 1] + str(k))


def ndof(sd, k):
    return len(R.dof_table(sd, k))


def reference(sd, k, order, pts):
    pts = np.asarray(pts)
    return np.stack([R.tabulate(sd, k, order, p) for p in pts])


def rel_check(got, ref, what="", tol=STANDING):
    """Per request: (ntab, ndof, npts) tables, values and derivatives apart."""
    got, ref = np.asarray(got, dtype=float), np.asarray(ref, dtype=float)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    for r in range(len(ref)):
        e0 = R.table_error(got[r, :1], ref[r, :1])
        e1 = R.table_error(got[r, 1:], ref[r, 1:]) if ref.shape[1] > 1 else 0.0
        print(f"{what} request {r}: values {e0:.2e} derivatives {e1:.2e}")
        assert e0 <= tol[0], (what, r, "values", e0)
        assert e1 <= tol[1], (what, r, "derivatives", e1)


def instance(sd, k, order):
    return f"fxk::hier_kernel<{sd},{k},{order}>"


def run(sd, k, order, npts, nreq, rng, sample=None, route=None, lo=-0.1, hi=1.1, **kw):
    """``nreq`` requests with points in [lo, hi]^sd, ``sample`` (default: all) against the restatement; ``route``:
    "image" / "stream", asserted with the instance's name."""
    import torch
    el = unit(sd, k)
    name = el.kernel(order, npts)
    assert name.startswith(instance(sd, k, order) + " "), name
    if route is not None:
        assert f" {route} " in name, name
    pts = rng.uniform(lo, hi, size=(nreq, npts, sd))
    out = el.tabulate_batch(order, pts, **kw)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (nreq, len(E.jet(sd, order)), ndof(sd, k), npts)
    idx = np.arange(nreq) if sample is None else np.asarray(sample)
    got = out[torch.as_tensor(idx, device=out.device)].cpu().numpy()
    rel_check(got, reference(sd, k, order, pts[idx]), (sd, k, order, npts, nreq))
    assert bool(torch.isfinite(out).all())
    return out


def requests_per_item(sd, k, order, npts):
    return int(unit(sd, k).kernel(order, npts).rsplit("P=", 1)[1])


def route_of(sd, k, order, npts):
    return unit(sd, k).kernel(order, npts).split()[1]


# ---- parity --------------------------------------------------------------------------------------------------------------

SPEC = [(sd, k, order) for sd in (1, 2, 3) for k in range(1, 7) for order in range(3)]


@pytest.mark.parametrize("sd,k,order", SPEC)
def test_compile_time_instances(sd, k, order):
    """Every compile-time instance once: 7 points (P = 9 where the image holds that many) and 13 requests leave a partial
    last item and an odd total."""
    run(sd, k, order, 7, 13, np.random.default_rng(sd * 100 + k * 10 + order))


def hierarchy_points():
    """Vertices, edge midpoints, the barycentre of face 0 and the barycentre of the UFC tetrahedron."""
    v = np.vstack([np.zeros(3), np.eye(3)])
    pts = [v[i] for i in range(4)]
    pts += [0.5 * (v[i] + v[j]) for i in range(4) for j in range(i + 1, 4)]
    pts += [v[[1, 2, 3]].mean(axis=0), v.mean(axis=0)]
    return np.array(pts)


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_hierarchy_vanishes_where_it_should(k):
    """The first degrees with each kind of correction.  A dof of entity e vanishes on every sub-entity of the cell that does
    not contain e: vertex functions at the other vertices, edge functions on the other edges, face functions on the other
    faces, interior bubbles on the whole boundary -- to 1e-13 -- and vertex functions are 1 at their vertex."""
    import fiat_amd
    el = unit(3, k)
    pts = hierarchy_points()
    tab = el.tabulate_batch(0, pts[None]).cpu().numpy()[0, 0]             # (ndof, npts)
    rel_check(tab[None, None], reference(3, k, 0, pts[None]), ("hierarchy", k))
    top = fiat_amd.ufc_simplex(3).get_topology()
    ids = el.entity_dofs()
    bary = np.concatenate([1 - pts.sum(-1, keepdims=True), pts], axis=-1)   # (npts, 4)
    checked = 0
    for dim in ids:
        for ent, dofs in ids[dim].items():
            mine = set(top[dim][ent])
            for j in range(len(pts)):
                support = {i for i in range(4) if bary[j, i] > 1e-14}     # the smallest entity the point lies in
                if not mine <= support:
                    for dof in dofs:
                        assert abs(tab[dof, j]) <= 1e-13, (k, dim, ent, dof, j, tab[dof, j])
                        checked += 1
    assert checked > 0
    np.testing.assert_allclose(tab[:4, :4], np.eye(4), rtol=0, atol=1e-13)


POINT_COUNTS = [1, 2, 31, 32, 33, 63, 64, 65, 129]


@pytest.mark.parametrize("npts", POINT_COUNTS)
@pytest.mark.parametrize("sd,k,order", [(2, 3, 1), (3, 2, 2)])
def test_point_counts(sd, k, order, npts):
    P = requests_per_item(sd, k, order, npts)
    for nreq in sorted({1, P + 1, 2 * P + 1}):
        run(sd, k, order, npts, nreq, np.random.default_rng(npts * 13 + nreq))


@pytest.mark.parametrize("sd,k,order", [(3, 4, 2), (3, 6, 2)])
def test_image_boundary(sd, k, order):
    """The last point count whose request leaves through the image and the first one that streams, as fx_hier_kernel
    reports them."""
    routes = [route_of(sd, k, order, n) for n in range(1, 200)]
    first_stream = routes.index("stream") + 1
    assert first_stream > 1 and set(routes[:first_stream - 1]) == {"image"} and set(routes[first_stream - 1:]) == {"stream"}
    for npts, route in ((first_stream - 1, "image"), (first_stream, "stream")):
        P = requests_per_item(sd, k, order, npts)
        run(sd, k, order, npts, 2 * P + 1, np.random.default_rng(npts), route=route)


def test_shrunk_items():
    """Requests of which 64 // npts do not fit the image together: the item shrinks to those that do."""
    for sd, k, order, npts in [(3, 3, 2, 8), (2, 5, 2, 9), (3, 4, 1, 8)]:
        P = requests_per_item(sd, k, order, npts)
        assert 1 <= P < 64 // npts
        for nreq in sorted({1, P + 1, 3 * P + 2}):
            run(sd, k, order, npts, nreq, np.random.default_rng(nreq), route="image")


@pytest.mark.parametrize("sd,k,order,npts,offset", [(2, 2, 1, 9, 0), (2, 2, 1, 9, 1), (3, 3, 1, 7, 2), (3, 6, 2, 23, 1),
                                                    (1, 4, 2, 5, 1), (3, 2, 2, 8, 2)])
def test_offset_out_with_guard_bands(sd, k, order, npts, offset):
    """An out= view 0, 1 and 2 doubles into a line (16-byte aligned or not): guards untouched, every entry written, equal to a
    fresh out and to the restatement."""
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
        rel_check(out.cpu().numpy(), reference(sd, k, order, pts), (sd, k, nreq))


def test_non_default_stream():
    import torch
    s = torch.cuda.Stream()
    for sd, k, order, npts, nreq in [(2, 3, 2, 9, 30), (3, 6, 2, 23, 3)]:
        el = unit(sd, k)
        pts = np.random.default_rng(npts).uniform(size=(nreq, npts, sd))
        dev = torch.as_tensor(pts).cuda()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            out = el.tabulate_batch(order, dev, stream=s)
        s.synchronize()
        rel_check(out.cpu().numpy(), reference(sd, k, order, pts), (sd, k, "stream"))


def test_grid_stride():
    """More items than the grid holds: every workgroup takes several."""
    import torch
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    P = requests_per_item(1, 1, 0, 4)
    nreq = 2 * num_cu * 64 * P + P + 3
    sample = E.sample_requests(nreq, P, nitems_per_trip=num_cu * 64, k=16, seed=4)
    run(1, 1, 0, 4, nreq, np.random.default_rng(nreq), sample=sample)


# ---- the two routes, the fixtures ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("sd", [1, 2, 3])
@pytest.mark.parametrize("k", range(1, 7))
def test_routes_agree(sd, k):
    el = unit(sd, k)
    pts = np.random.default_rng(sd * 10 + k).uniform(size=(5, 11, sd))
    direct = el.tabulate_batch(2, pts).cpu().numpy()
    general = el.tabulate_batch(2, pts, route="general").cpu().numpy()
    for r in range(len(pts)):
        e = R.table_error(general[r], direct[r])
        print(f"sd {sd} degree {k} request {r}: routes differ by {e:.2e}")
        assert e <= ROUTE_TOL, (sd, k, r, e)
    with pytest.raises(ValueError):
        el.tabulate_batch(2, pts, route="fast")


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_tabulate_against_fixture(name):
    """``tabulate`` and ``tabulate_batch`` against the reference's tables, the general-route cases (degree 7, order 3) and
    "integral(2)" included; the direct route also against the restatement at the same points."""
    from fiat_amd import mis
    c, k, variant, order = M.CASES[name]
    sd = SD[c]
    el = element(name)
    pts, ref = G[f"{name}_pts"], G[f"{name}_tab"]
    assert int(G[f"{name}_order"][0]) == order
    direct = k <= 6 and order <= 2
    assert ("hier_kernel" in el.kernel(order, len(pts))) == direct
    assert list(M.ids_rows(el.entity_dofs()).ravel()) == list(G[f"{name}_eids"].ravel())
    assert list(M.ids_rows(el.entity_closure_dofs()).ravel()) == list(G[f"{name}_cids"].ravel())
    assert [el.degree(), el.space_dimension(), el.get_formdegree(), sd] == list(G[f"{name}_meta"])
    assert R.table_error(el.get_coeffs(), G[f"{name}_coeffs"]) <= ROUTE_TOL
    tab = el.tabulate(order, pts)
    assert list(tab) == [a for o in range(order + 1) for a in mis(sd, o)]
    rel_check(np.stack([tab[a] for a in tab])[None], ref[None], name)
    dev = el.tabulate_batch(order, np.stack([pts, pts[::-1]])).cpu().numpy()
    rel_check(dev, np.stack([ref, ref[..., ::-1]]), name)
    if direct:
        rel_check(dev[:1], reference(sd, k, order, pts[None]), name)
    else:
        names = E.launched(lambda: el.tabulate_batch(order, pts[None]))
        assert names and not [n for n in names if "hier_kernel" in n], names


@pytest.mark.parametrize("name", sorted(M.ENTITY))
def test_entity_tabulation(name):
    c, k, _, _ = M.CASES[name]
    sd = SD[c]
    el = element(name)
    dim, number = (int(v) for v in G[f"{name}_e_ent"])
    p, ref = G[f"{name}_e_pts"], G[f"{name}_e_tab"]
    tab = el.tabulate(1, p, entity=(dim, number))
    rel_check(np.stack([tab[a] for a in tab])[None], ref[None], (name, dim, number))
    dev = el.tabulate_batch(1, np.stack([p, p[::-1]]), entity=(dim, number)).cpu().numpy()
    rel_check(dev, np.stack([ref, ref[..., ::-1]]), (name, dim, number))
    general = el.tabulate_batch(1, p[None], entity=(dim, number), route="general").cpu().numpy()
    assert R.table_error(general[0], dev[0]) <= ROUTE_TOL
    names = E.launched(lambda: el.tabulate_batch(1, p[None], entity=(dim, number)))
    assert [n for n in names if "hier_kernel" in n], names


def test_per_request_cells_take_the_general_route():
    """``verts=``: equal to the element the facade builds on a physical triangle, and to the chain rule applied to the
    reference-cell tables."""
    import fiat_amd
    from fiat_amd import reference_element
    el = unit(2, 3)
    rng = np.random.default_rng(3)
    verts = np.array([[0.2, 0.1], [1.3, 0.4], [0.5, 1.6]])
    ref_pts = E.simplex_points(rng, (7,), 2)
    B = (verts[1:] - verts[0]).T                                           # x = B xi + v0
    phys = ref_pts @ B.T + verts[0]
    names = E.launched(lambda: el.tabulate_batch(1, phys[None], verts=verts[None]))
    assert names and not [n for n in names if "hier_kernel" in n], names
    got = el.tabulate_batch(1, phys[None], verts=verts[None], pushforward=True).cpu().numpy()[0]
    # chain rule: grad_x = B^-T grad_xi
    ref = R.tabulate(2, 3, 1, ref_pts)
    Binv = np.linalg.inv(B)
    chain = np.concatenate([ref[:1], np.einsum("id,ijp->djp", Binv, ref[1:])])
    rel_check(got[None], chain[None], "verts / chain rule")
    cell = reference_element.UFCSimplex(reference_element.TRIANGLE, tuple(map(tuple, verts)),
                                        fiat_amd.ufc_simplex(2).get_topology())
    other = fiat_amd.IntegratedLegendre(cell, 3)
    assert "hier_kernel" not in other.kernel(1, 7)
    tab = other.tabulate(1, phys)
    err = R.table_error(np.stack([tab[a] for a in tab]), got)
    print(f"element on the physical triangle: {err:.2e}")
    assert err <= ROUTE_TOL


def test_direct_route_launches_the_instance():
    el = unit(3, 4)
    pts = np.random.default_rng(1).uniform(size=(3, 5, 3))
    names = E.launched(lambda: el.tabulate_batch(1, pts))
    assert [n for n in names if "hier_kernel<3, 4, 1>" in n.replace(",", ", ").replace(",  ", ", ")], names
    names = E.launched(lambda: el.tabulate_batch(1, pts, route="general"))
    assert names and not [n for n in names if "hier_kernel" in n], names
    import torch
    assert torch.equal(el.tabulate_batch(1, pts, pushforward=True), el.tabulate_batch(1, pts))


# ---- the reference's own unit tests of the family, restated against the facade ----------------------------------------------

def apply_node(node, fn):
    """A scalar functional applied to a function: the facade's functionals are data, sum of weight * fn(point)."""
    assert not node.deriv_dict
    return sum(w * fn(pt) for pt, wcs in node.get_point_dict().items() for w, comp in wcs)


@pytest.mark.parametrize("dim", [1, 2, 3])
@pytest.mark.parametrize("degree", range(1, 7))
def test_monomial_integrals_through_the_dual_nodes(dim, degree):
    """sum_i n_i(v) int phi_i = int v for v = (x_1 + ... + x_d)^m, m <= degree: the nodal basis reproduces P_degree."""
    import fiat_amd
    s = fiat_amd.ufc_simplex(dim)
    q = fiat_amd.make_quadrature(s, degree + 1)
    fe = unit(dim, degree)
    tab = fe.tabulate(0, np.asarray(q.get_points()))[(0,) * dim]
    for m in range(degree + 1):
        v = lambda x: sum(x) ** m     # noqa: E731
        coefs = [apply_node(n, v) for n in fe.dual_basis()]
        assert np.allclose(np.dot(coefs, np.dot(tab, q.get_weights())), q.integrate(v), rtol=1e-14)


@pytest.mark.parametrize("degree", range(1, 7))
def test_sparsity_on_the_interval(degree):
    """Non-zeros of the mass and stiffness matrices of the hierarchy on the interval."""
    import fiat_amd
    q = fiat_amd.make_quadrature(fiat_amd.ufc_simplex(1), degree + 1)
    fe = unit(1, degree)
    expected = [5 * min(degree, 3) + 3 * max(0, degree - 3) - 1, degree + 3]
    tab = fe.tabulate(1, np.asarray(q.get_points()))
    for k, ennz in enumerate(expected):
        A = sum((tab[a] * q.get_weights()) @ tab[a].T for a in tab if sum(a) == k)
        assert A.size - np.sum(np.isclose(A, 0.0, rtol=1e-14)) == ennz


def test_constructor_and_registry():
    import fiat_amd
    from fiat_amd import hierarchical
    assert fiat_amd.supported_elements["Integrated Legendre"] is fiat_amd.IntegratedLegendre is hierarchical.IntegratedLegendre
    assert isinstance(unit(2, 3).get_dual_set(), hierarchical.IntegratedLegendreDual)
    assert list(G["raises_degree0"]) == [1]
    with pytest.raises(ValueError, match=bytes(G["raises_text"]).decode()):
        fiat_amd.IntegratedLegendre(fiat_amd.ufc_simplex(2), 0)
    rule, tests = hierarchical.make_dual_bubbles(fiat_amd.reference_element.symmetric_simplex(1), 3)
    assert tests.shape == (2, len(rule.get_points()))


def test_finat_adapter_accepts_the_element():
    from fiat_amd import finat_adapter as ad
    el = unit(3, 3)
    fe = ad.FiatElement(el)
    pts = np.random.default_rng(5).uniform(size=(2, 6, 3))
    ref = reference(3, 3, 2, pts)
    res = fe.basis_evaluation(2, ad.PointSet(pts[0]))
    bres = fe.basis_evaluation_batch(2, pts)
    for t, alpha in enumerate(E.jet(3, 2)):
        tol = STANDING[0] if t == 0 else STANDING[1]
        assert R.table_error(res[alpha].array.reshape(20, 6), ref[0, t]) <= tol
        assert R.table_error(bres[alpha].array.cpu().numpy(), ref[:, t]) <= tol
    assert fe.space_dimension() == 20 and fe.formdegree == 0 and fe.degree == 3
