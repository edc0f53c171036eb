"""Bernstein elements on the HIP path (fiat_amd/csrc/bernstein.hpp): the reference's tabulations (tests/golden/bernstein.npz,
FIAT/bernstein.py) at 1e-12 for values and 1e-10 for derivatives -- with the exact n! where the derivative order equals
the degree (>= 2), which the reference returns as 1 -- on the element's cell, on sub-entities, on per-request physical
cells and on the shared-point route; the pointwise dual; error paths; and two full-size batches checked against the
definition and against the independent Dubiner-coefficient kernels."""
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "bernstein.npz"))
TOL_VAL, TOL_DER = 1e-12, 1e-10


def keys(sd, order):
    from fiat_amd.polynomial_set import mis
    return [a for o in range(order + 1) for a in mis(sd, o)]


def corrected(tab, sd, n, order):
    """The reference's tables with its order == degree entries (1) scaled to the exact n!."""
    tab = np.array(tab, dtype=float)
    t = 0
    for o in range(order + 1):
        for _ in keys(sd, o)[len(keys(sd, o - 1)) if o else 0:]:
            if o == n and n >= 2:
                tab[t] *= math.factorial(n)
            t += 1
    return tab


def check_tables(got, ref, sd):
    ref = np.asarray(ref)
    got = np.asarray(got)
    assert got.shape == ref.shape
    scale = max(1.0, np.abs(ref[0]).max())
    assert np.abs(got[0] - ref[0]).max() <= TOL_VAL * scale
    if len(ref) > 1:
        scale = max(1.0, np.abs(ref[1:]).max())
        assert np.abs(got[1:] - ref[1:]).max() <= TOL_DER * scale


def as_stack(tab, sd, order):
    return np.stack([tab[a] for a in keys(sd, order)])


def numpy_tables(lam, Gm, n, order):
    """Definition of the basis, written independently of the kernel: lam (npts, sd+1) barycentric coordinates, Gm
    (sd+1, sd) = d lambda / dx -> (ntab, ndof, npts)."""
    from fiat_amd.polynomial_set import mis
    sd = Gm.shape[1]
    ks = np.array(mis(sd + 1, n))
    out = []
    for o in range(order + 1):
        for alpha in mis(sd, o):
            dirs = [d for d, a in enumerate(alpha) for _ in range(a)]
            tab = np.zeros((len(ks), lam.shape[0]))
            for seq in np.ndindex(*(sd + 1,) * o):
                beta = np.bincount(np.array(seq, dtype=int), minlength=sd + 1)
                w = np.prod([Gm[s, d] for s, d in zip(seq, dirs)]) if o else 1.0
                e = ks - beta
                ok = (e >= 0).all(1)
                c = np.array([math.factorial(n) / np.prod([math.factorial(int(x)) for x in row]) if good else 0.0
                              for row, good in zip(e, ok)])
                tab += w * c[:, None] * np.prod(lam[None] ** np.maximum(e, 0)[:, None, :], axis=2) * ok[:, None]
            out.append(tab)
    return np.stack(out)


def bary(verts, pts):
    """lam (npts, sd+1) and Gm (sd+1, sd) of points in the simplex verts (sd+1, sd)."""
    sd = verts.shape[1]
    E = np.linalg.inv((verts[1:] - verts[0]).T)
    lam_r = (pts - verts[0]) @ E.T
    lam = np.concatenate([1.0 - lam_r.sum(1, keepdims=True), lam_r], axis=1)
    Gm = np.concatenate([-E.sum(0, keepdims=True), E])
    assert Gm.shape == (sd + 1, sd)
    return lam, Gm


@pytest.fixture(scope="module")
def elements():
    from fiat_amd import Bernstein, ufc_simplex
    cache = {}

    def get(sd, n):
        if (sd, n) not in cache:
            cache[(sd, n)] = Bernstein(ufc_simplex(sd), n)
        return cache[(sd, n)]
    return get


@pytest.mark.parametrize("sd", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6])
def test_fixture_orders_0_to_3(elements, sd, n):
    """Orders 0..2 run on the compile-time instances, order 3 on the generic one: both against the reference."""
    el = elements(sd, n)
    pts = G[f"pts_s{sd}"]
    ref = corrected(G[f"tab_s{sd}_n{n}"], sd, n, 3)
    check_tables(as_stack(el.tabulate(3, pts), sd, 3), ref, sd)
    for order in (0, 1, 2):
        ntab = len(keys(sd, order))
        check_tables(as_stack(el.tabulate(order, pts), sd, order), ref[:ntab], sd)


@pytest.mark.parametrize("name,sd,n", [("tet10", 3, 10), ("tri16", 2, 16)])
def test_high_degree(elements, name, sd, n):
    el = elements(sd, n)
    check_tables(as_stack(el.tabulate(1, G[f"hi_{name}_pts"]), sd, 1), G[f"hi_{name}"], sd)


def test_degree_zero(elements):
    el = elements(2, 0)
    tab = el.tabulate(2, G["pts_s2"])
    assert np.array_equal(tab[(0, 0)], np.ones((1, len(G["pts_s2"]))))
    assert all(not np.any(tab[a]) for a in keys(2, 2)[1:])


def test_order_above_degree_is_zero(elements):
    tab = elements(3, 2).tabulate(4, G["pts_s3"])
    assert all(not np.any(tab[a]) for a in keys(3, 4)[len(keys(3, 2)):])


def test_second_derivatives_of_the_reference_test(elements):
    """The reference's test_bernstein_2nd_derivatives, restated on its recorded inputs and outputs."""
    check_tables(as_stack(elements(2, 3).tabulate(2, G["d2_pts"]), 2, 2), G["d2_tab"], 2)


@pytest.mark.parametrize("sd", [1, 2])
def test_single_point(elements, sd):
    el = elements(sd, 1)
    point = (0.0,) * sd
    assert el.tabulate(0, point)[(0,) * sd].shape == (el.space_dimension(),)
    assert el.tabulate(0, [point])[(0,) * sd].shape == (el.space_dimension(), 1)


@pytest.mark.parametrize("sd,dim,entity", [(2, 1, 0), (2, 1, 2), (3, 2, 1), (3, 1, 4), (3, 2, 3)])
def test_entity(elements, sd, dim, entity):
    key = f"ent_s{sd}_d{dim}_e{entity}"
    el = elements(sd, 3)
    check_tables(as_stack(el.tabulate(2, G[key + "_pts"], entity=(dim, entity)), sd, 2), corrected(G[key], sd, 3, 2), sd)


@pytest.mark.parametrize("sd", [1, 2, 3])
@pytest.mark.parametrize("n", [2, 4])
def test_per_request_cells(elements, sd, n):
    """tabulate_batch(order, physical points, verts) == the reference's element built on each physical cell."""
    el = elements(sd, n)
    verts, pts = G[f"phys_s{sd}_verts"], G[f"phys_s{sd}_pts"]
    from fiat_amd import runtime
    for order in (2, 3):
        out = runtime.fetch(el.tabulate_batch(order, pts, verts=verts))
        for r in range(len(verts)):
            ntab = len(keys(sd, 2))
            check_tables(out[r][:ntab], corrected(G[f"phys_s{sd}_n{n}_r{r}"], sd, n, 2), sd)
            if order == 3:
                lam, Gm = bary(verts[r], pts[r])
                check_tables(out[r], numpy_tables(lam, Gm, n, 3), sd)


@pytest.mark.parametrize("sd,n,order", [(2, 3, 1), (3, 2, 2), (3, 6, 2), (2, 8, 2), (3, 3, 4), (1, 4, 1)])
def test_tabulate_cells_equals_batch(elements, sd, n, order):
    """The shared-point route == tabulate_batch at the pushed-forward points with the same cells."""
    import torch
    from fiat_amd import runtime
    rng = np.random.default_rng(sd * 100 + n)
    el = elements(sd, n)
    ref = np.array(el.ref_el.get_vertices())
    A = np.eye(sd) + 0.3 * rng.standard_normal((37, sd, sd))
    A[::2, :, 0] *= -1.0
    verts = np.einsum("vd,red->rve", ref, A) + rng.standard_normal((37, 1, sd))
    e = rng.exponential(size=(9, sd + 1))
    ref_pts = (e / e.sum(1, keepdims=True)) @ ref
    phys = np.einsum("pv,rvd->rpd", e / e.sum(1, keepdims=True), verts)
    a = el.tabulate_cells(order, ref_pts, verts)
    b = el.tabulate_batch(order, phys, verts=verts, pushforward=True)
    torch.cuda.synchronize()
    x, y = runtime.fetch(a), runtime.fetch(b)
    assert np.abs(x - y).max() <= 1e-10 * max(1.0, np.abs(y).max())


def test_entity_cells(elements):
    """tabulate_cells(..., entity=) on a facet == tabulate_cells at the facet points mapped into the cell."""
    from fiat_amd import runtime
    el = elements(3, 3)
    rng = np.random.default_rng(7)
    verts = np.array(el.ref_el.get_vertices())[None] + 0.1 * rng.standard_normal((5, 4, 3))
    fpts = G["ent_s3_d2_e1_pts"]
    M, b = el.entity_map((2, 1))
    x = runtime.fetch(el.tabulate_cells(1, fpts, verts, entity=(2, 1)))
    y = runtime.fetch(el.tabulate_cells(1, fpts @ M.T + b, verts))
    assert np.abs(x - y).max() <= 1e-12 * max(1.0, np.abs(y).max())


@pytest.mark.parametrize("name,sd,n", [("p2tri", 2, 2), ("p3tri", 2, 3), ("p2tet", 3, 2)])
def test_pointwise_dual(elements, name, sd, n):
    el = elements(sd, n)
    lat = G[f"lat_{name}"]
    W = np.zeros((len(lat), len(lat)))
    index = {tuple(p): j for j, p in enumerate(lat)}
    for i, node in enumerate(el.dual_basis()):
        for pt, wcs in node.pt_dict.items():
            for w, comp in wcs:
                assert comp == ()
                W[i, index[tuple(pt)]] += w
    assert np.abs(W - G[f"dualw_{name}"]).max() <= 1e-10 * max(1.0, np.abs(W).max())
    V = el.tabulate(0, lat)[(0,) * sd]                    # (ndof, npts)
    assert np.abs(W @ V.T - np.eye(len(lat))).max() <= 1e-10


def test_entity_dofs_and_support(elements):
    from fiat_amd.finite_element import entity_support_dofs as esd
    el = elements(2, 3)
    ids = el.entity_dofs()
    assert sorted(i for d in ids for e in ids[d] for i in ids[d][e]) == list(range(10))
    closure = el.entity_closure_dofs()
    assert sorted(closure[2][0]) == list(range(10))
    support = esd(el, 1)
    for e, dofs in support.items():
        assert sorted(dofs) == sorted(closure[1][e])
    assert el.mapping() == ["affine"] * 10 and el.value_shape() == () and el.degree() == 3 and not el.is_nodal()


def test_requests_and_finat(elements):
    from fiat_amd import Request, tabulate_requests
    from fiat_amd import finat_adapter
    el = elements(3, 2)
    pts = G["pts_s3"]
    outs = tabulate_requests([Request(el, 1, pts), Request(el, 1, pts[:3])])
    ref = as_stack(el.tabulate(1, pts), 3, 1)
    assert np.abs(outs[0].cpu().numpy() - ref).max() == 0.0
    assert np.abs(outs[1].cpu().numpy() - ref[..., :3]).max() == 0.0
    fe = finat_adapter.FiatElement(el)
    assert fe.space_dimension() == 10 and fe.degree == 2


def test_errors(elements):
    from fiat_amd import Bernstein, ufc_simplex
    from fiat_amd.reference_element import UFCQuadrilateral
    with pytest.raises(NotImplementedError):
        Bernstein(ufc_simplex(2), 17)
    el = elements(2, 3)
    pts = G["pts_s2"]
    with pytest.raises(NotImplementedError):
        el.tabulate(9, pts)
    verts = G["phys_s2_verts"]
    with pytest.raises(NotImplementedError):
        el.tabulate_batch(5, G["phys_s2_pts"], verts=verts)
    with pytest.raises(NotImplementedError):
        el.tabulate_cells(5, pts, verts)
    with pytest.raises(ValueError):
        el.tabulate_batch(1, pts[None, :, :1])
    with pytest.raises(ValueError):
        Bernstein(UFCQuadrilateral(), 2)


# ---------------------------------------------------------------------------------------------------------------------
# full size

def full_batch(nreq, npts, seed):
    rng = np.random.default_rng(seed)
    e = rng.exponential(size=(nreq, npts, 4))
    return (e / e.sum(-1, keepdims=True))[..., 1:].copy()


def dubiner_route(el, order, pts_dev):
    """Bernstein as coefficients in the orthonormal Dubiner basis, tabulated by the existing contraction kernels."""
    from fiat_amd import ONPolynomialSet, PolynomialSet, make_lattice
    n, ref_el = el.degree(), el.ref_el
    on = ONPolynomialSet(ref_el, n)
    lat = np.array(make_lattice(ref_el.get_vertices(), n, variant="gll"))
    Vphi = on.tabulate(lat, 0)[(0, 0, 0)]                               # (nexp, npts)
    VB = el.tabulate(0, lat)[(0, 0, 0)]                                 # (ndof, npts)
    C = np.linalg.solve(Vphi.T, VB.T).T                                 # B = C phi
    ps = PolynomialSet(ref_el, n, n, on.get_expansion_set(), C)
    return ps.device_polyset().tabulate_batch(order, pts_dev)


@pytest.mark.parametrize("n,order,nreq", [(3, 1, 100_000), (6, 2, 125_000)])
def test_full_size(elements, n, order, nreq):
    import torch
    from fiat_amd import runtime
    el = elements(3, n)
    pts = torch.as_tensor(full_batch(nreq, 23, n)).cuda()
    out = el.tabulate_batch(order, pts)
    torch.cuda.synchronize()
    runtime.Context.get().check()
    v = out[:, 0]
    assert torch.abs(v.sum(1) - 1.0).max().item() < 1e-13                       # partition of unity
    assert v.min().item() >= 0.0                                                # non-negative inside the cell
    assert torch.abs(out[:, 1:].sum(2)).max().item() < 1e-10                    # derivatives of the unity: 0
    rng = np.random.default_rng(0)
    sample = np.sort(rng.choice(nreq, 400, replace=False))
    sample[0], sample[-1] = 0, nreq - 1
    got = out[torch.as_tensor(sample).cuda()].cpu().numpy()
    host_pts = pts[torch.as_tensor(sample).cuda()].cpu().numpy()
    Gm = np.concatenate([-np.ones((1, 3)), np.eye(3)])
    for k, r in enumerate(sample):
        lam, _ = bary(np.array(el.ref_el.get_vertices()), host_pts[k])
        check_tables(got[k], numpy_tables(lam, Gm, n, order), 3)
    # the whole batch against the Dubiner-coefficient route
    dub = dubiner_route(el, order, pts)
    diff = torch.abs(dub - out).amax().item()
    assert diff <= 1e-10 * max(1.0, torch.abs(out).amax().item()), diff
