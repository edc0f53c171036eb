"""Serendipity elements on the GPU: parity of tabulate / tabulate_batch with the reference's fixtures
(tests/golden/serendipity.npz), metadata, entity dofs, the pointwise dual, entity= tabulation, every kernel instance and
route against the NumPy restatement (tests/serendipity_reference.py), the tiling edges of the kernel, and the errors.
Tolerances: the project's standing 1e-12 on values and 1e-10 on derivatives, in the norm max|x - ref| / max(1, max|ref|)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import edge_reference as E  # noqa: E402  (guarded outputs, request samples)
import make_golden_serendipity as M  # noqa: E402
import serendipity_reference as R  # noqa: E402

TOL_VAL, TOL_DER = 1e-12, 1e-10
G = np.load(os.path.join(HERE, "golden", "serendipity.npz"))
IMAGE_BYTES = 40 * 1024
_ELS = {}


def element(name):
    import fiat_amd
    if name not in _ELS:
        _ELS[name] = M.build(fiat_amd, name)
    return _ELS[name]


def unit(sd, k):
    """S_k on the UFC quadrilateral / hexahedron."""
    import fiat_amd
    from fiat_amd import reference_element
    key = ("unit", sd, k)
    if key not in _ELS:
        _ELS[key] = fiat_amd.Serendipity(reference_element.ufc_hypercube(sd), k)
    return _ELS[key]


def rel_check(got, ref, what=""):
    """Per request: (ntab, ndof, npts) tables, values and derivatives apart."""
    got, ref = np.asarray(got, dtype=float), np.asarray(ref, dtype=float)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    for r in range(len(ref)):
        e0 = R.rel_err(got[r, :1], ref[r, :1])
        e1 = R.rel_err(got[r, 1:], ref[r, 1:]) if ref.shape[1] > 1 else 0.0
        assert e0 <= TOL_VAL, (what, r, "values", e0)
        assert e1 <= TOL_DER, (what, r, "derivatives", e1)


def stack(tab, sd, order):
    from fiat_amd import mis
    return np.stack([tab[a] for k in range(order + 1) for a in mis(sd, k)])


def run(sd, k, order, npts, nreq, rng, sample=None, expect=None):
    """``nreq`` requests with points in [-0.1, 1.1] on the unit box, ``sample`` (default: all) against the restatement."""
    import torch
    el = unit(sd, k)
    if expect is not None:
        assert el.kernel(order, npts) == expect
    pts = rng.uniform(-0.1, 1.1, size=(nreq, npts, sd))
    out = el.tabulate_batch(order, pts)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (nreq, len(R.mis(sd, order)), R.ndof(sd, k), npts)
    idx = np.arange(nreq) if sample is None else sample
    got = out[torch.as_tensor(idx, device=out.device)].cpu().numpy()
    rel_check(got, R.tabulate(sd, k, order, pts[idx]), (sd, k, order, npts, nreq))
    assert bool(torch.isfinite(out).all())
    return out


def requests_per_item(sd, k, order, npts):
    """P of the route report."""
    return int(unit(sd, k).kernel(order, npts).rsplit("P=", 1)[1])


# ---- the reference's fixtures ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(M.CASES))
def test_tabulate_against_fixture(name):
    kind, k, order, _ = M.CASES[name]
    el = element(name)
    sd = el.get_reference_element().get_spatial_dimension()
    pts, ref = G[f"{name}_pts"], G[f"{name}_tab"]
    tab = el.tabulate(order, pts)
    from fiat_amd import mis
    assert list(tab) == [a for o in range(order + 1) for a in mis(sd, o)]
    rel_check(stack(tab, sd, order)[None], ref[None], name)
    # the batch form: request 0 = the fixture's points, request 1 = the same points reversed
    dev = el.tabulate_batch(order, np.stack([pts, pts[::-1]])).cpu().numpy()
    rel_check(dev, np.stack([ref, ref[..., ::-1]]), name)


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_metadata_and_entity_dofs(name):
    kind, k, order, _ = M.CASES[name]
    el = element(name)
    assert list(M.metadata(el)) == list(G[f"{name}_meta"])
    assert el.degree() == k + 1 and el.value_shape() == () and el.get_formdegree() == 0
    assert el.mapping() == ["affine"] * el.space_dimension()
    assert np.array_equal(M.eids_rows(el.entity_dofs()), G[f"{name}_eids"])
    with pytest.raises(NotImplementedError):
        el.get_coeffs()
    closure = el.entity_closure_dofs()
    top = max(closure, key=repr) if kind in ("prod", "box") else max(closure)
    assert closure[top][0] == list(range(el.space_dimension()))


def test_constructor_as_the_reference():
    import fiat_amd
    from fiat_amd import reference_element
    line = fiat_amd.Serendipity(fiat_amd.UFCInterval(), 3)
    assert isinstance(line, fiat_amd.Lagrange) and line.space_dimension() == 4
    with pytest.raises(IndexError):
        fiat_amd.Serendipity(reference_element.Point(), 1)
    assert fiat_amd.supported_elements["S"] is fiat_amd.Serendipity


@pytest.mark.parametrize("name", sorted(n for n, c in M.CASES.items() if c[3]))
def test_dual_against_fixture(name):
    """unisolvent_pts, and the dual nodes' points and weights (the reference's systems have condition numbers <= 1.2e3 and
    no weight within a decade of the 1e-12 drop threshold); then Q phi = I."""
    from fiat_amd.serendipity import unisolvent_pts
    kind, k, order, _ = M.CASES[name]
    el = element(name)
    upts = np.array(unisolvent_pts(el.get_reference_element(), k), dtype=float)
    np.testing.assert_allclose(upts, G[f"{name}_upts"], rtol=0, atol=1e-15)
    W = M.dual_matrix(el, upts)
    ref = G[f"{name}_dual"]
    assert W.shape == ref.shape
    np.testing.assert_allclose(W, ref, rtol=0, atol=1e-10 * max(1.0, np.abs(ref).max()))
    assert np.array_equal(W != 0, ref != 0)
    sd = upts.shape[1]
    phi = el.tabulate(0, upts)[(0,) * sd]
    np.testing.assert_allclose(W @ phi.T, np.eye(len(W)), rtol=0, atol=1e-11)
    for node in el.dual_basis():
        assert node.get_reference_element() is el.get_reference_element()


@pytest.mark.parametrize("name", ["q7", "h7"])
def test_unisolvent_points_of_high_degrees(name):
    from fiat_amd.serendipity import unisolvent_pts
    kind, k, _, _ = M.CASES[name]
    upts = np.array(unisolvent_pts(M.cell(__import__("fiat_amd"), kind), k), dtype=float)
    np.testing.assert_allclose(upts, G[f"{name}_upts"], rtol=0, atol=1e-15)


@pytest.mark.parametrize("name,dim,ent", M.ENTITIES)
def test_entity_tabulation(name, dim, ent):
    el = element(name)
    sd = el.get_reference_element().get_spatial_dimension()
    key = ((1, 0), 0) if name == "b5" else (dim, ent)
    p, ref = G[f"ent_{name}_{dim}_{ent}_pts"], G[f"ent_{name}_{dim}_{ent}_tab"]
    rel_check(stack(el.tabulate(1, p, entity=key), sd, 1)[None], ref[None], (name, dim, ent))
    dev = el.tabulate_batch(1, np.stack([p, p[::-1]]), entity=key).cpu().numpy()
    rel_check(dev, np.stack([ref, ref[..., ::-1]]), (name, dim, ent))
    # the cell itself as the entity: the points as they are
    cell_key = (el.get_reference_element().get_dimension(), 0)
    q = G[f"{name}_pts"]
    assert np.array_equal(stack(el.tabulate(1, q, entity=cell_key), sd, 1), stack(el.tabulate(1, q), sd, 1))


@pytest.mark.parametrize("sd", [2, 3])
def test_s1_is_q1(sd):
    import fiat_amd
    L = fiat_amd.Lagrange(fiat_amd.UFCInterval(), 1)
    Q = fiat_amd.TensorProductElement(L, L)
    if sd == 3:
        Q = fiat_amd.TensorProductElement(Q, L)
    pts = np.random.default_rng(sd).uniform(-0.1, 1.1, size=(13, sd))
    got, ref = unit(sd, 1).tabulate(2, pts), Q.tabulate(2, pts)
    assert list(got) == list(ref)
    rel_check(stack(got, sd, 2)[None], stack(ref, sd, 2)[None], "Q1")


def test_finat_adapter_accepts_the_element():
    from fiat_amd import finat_adapter as ad
    el = unit(3, 3)
    fe = ad.FiatElement(el)
    pts = np.random.default_rng(5).uniform(size=(2, 6, 3))
    ref = R.tabulate(3, 3, 2, pts)
    res = fe.basis_evaluation(2, ad.PointSet(pts[0]))
    bres = fe.basis_evaluation_batch(2, pts)
    for t, alpha in enumerate(R.mis(3, 2)):
        tol = TOL_VAL if t == 0 else TOL_DER
        assert R.rel_err(res[alpha].array.reshape(32, 6), ref[0, t]) <= tol
        assert R.rel_err(bres[alpha].array.cpu().numpy(), ref[:, t]) <= tol


# ---- every instance and route ----------------------------------------------------------------------------------------

SPEC = [(sd, k, order) for sd in (2, 3) for k in range(1, 7) for order in range(3)]


@pytest.mark.parametrize("sd,k,order", SPEC)
def test_compile_time_instances(sd, k, order):
    """Every compile-time instance on its image route (3 points: the largest request is 25 KB) and streaming (64 points
    where that exceeds the image)."""
    reqsize = len(R.mis(sd, order)) * R.ndof(sd, k)
    P = min(64 // 3, IMAGE_BYTES // (reqsize * 3 * 8))
    run(sd, k, order, 3, 2 * P + 1, np.random.default_rng(sd * 100 + k * 10 + order),
        expect=f"fxk::serendipity_kernel<{sd},{k},{order}> image P={P}")
    if reqsize * 64 * 8 > IMAGE_BYTES:
        run(sd, k, order, 64, 3, np.random.default_rng(k), expect=f"fxk::serendipity_kernel<{sd},{k},{order}> stream P=1")


GENERIC = [(2, 7, 1, 9), (2, 8, 2, 5), (2, 10, 3, 7), (2, 12, 3, 70), (3, 7, 1, 10), (3, 8, 2, 4), (3, 10, 3, 3), (3, 12, 3, 5),
           (2, 3, 3, 11), (3, 2, 3, 10), (3, 1, 3, 64), (2, 1, 3, 1)]


@pytest.mark.parametrize("sd,k,order,npts", GENERIC)
def test_generic_instance(sd, k, order, npts):
    P = 64 // npts if npts <= 64 else 1
    run(sd, k, order, npts, 2 * P + 1, np.random.default_rng(k + npts), expect=f"fxk::serendipity_generic<{sd}> stream P={P}")


# ---- tiling edges ------------------------------------------------------------------------------------------------------

POINT_COUNTS = [1, 7, 21, 32, 33, 63, 64, 65, 130]
POINT_ELEMENTS = [(2, 4, 2), (3, 2, 1), (3, 3, 0), (2, 9, 1)]     # image and streaming by size; the last one generic


@pytest.mark.parametrize("npts", POINT_COUNTS)
@pytest.mark.parametrize("sd,k,order", POINT_ELEMENTS)
def test_point_counts(sd, k, order, npts):
    """Every point count with every remainder of the last item: nreq in {1, P - 1, P, P + 1, 3 P + 2}."""
    P = requests_per_item(sd, k, order, npts)
    for nreq in E.nreq_list(P):
        run(sd, k, order, npts, nreq, np.random.default_rng(npts * 13 + nreq))


def test_every_requests_per_item():
    """S_1 quadrilateral values: 32 bytes per point, so P = 64 // npts for every npts; a partial last item for each."""
    seen = set()
    for npts in range(1, 66):
        P = requests_per_item(2, 1, 0, npts)
        assert P == (64 // npts if npts <= 64 else 1)
        if P in seen:
            continue
        seen.add(P)
        run(2, 1, 0, npts, 2 * P + max(1, P // 2), np.random.default_rng(npts))
    assert seen == {64 // n for n in range(1, 65)}


# (sd, k, order, npts below / at the switch, npts above): the largest request of <= 40 KB and the first one beyond
IMAGE_EDGE = [(3, 6, 2, 4, 5), (3, 3, 1, 40, 41), (2, 6, 2, 28, 29), (3, 2, 2, 25, 26)]


@pytest.mark.parametrize("sd,k,order,below,above", IMAGE_EDGE)
def test_image_boundary(sd, k, order, below, above):
    reqsize = len(R.mis(sd, order)) * R.ndof(sd, k)
    assert reqsize * below * 8 <= IMAGE_BYTES < reqsize * above * 8
    run(sd, k, order, below, 5, np.random.default_rng(below), expect=f"fxk::serendipity_kernel<{sd},{k},{order}> image P=1")
    run(sd, k, order, above, 3 * (64 // above) + 1, np.random.default_rng(above),
        expect=f"fxk::serendipity_kernel<{sd},{k},{order}> stream P={64 // above}")


def test_shrunk_items():
    """Requests of which 64 // npts do not fit the image together: the item shrinks to those that do."""
    for sd, k, order, npts, P in [(3, 3, 1, 27, 1), (3, 2, 2, 8, 3), (2, 5, 2, 9, 4), (3, 4, 1, 8, 3)]:
        assert P < 64 // npts
        for nreq in E.nreq_list(P):
            run(sd, k, order, npts, nreq, np.random.default_rng(nreq), expect=f"fxk::serendipity_kernel<{sd},{k},{order}> image P={P}")


@pytest.mark.parametrize("sd,k,order,npts,nreq", [(2, 4, 0, 3, 5), (2, 5, 1, 7, 12), (3, 6, 0, 1, 49), (2, 4, 1, 5, 7)])
def test_odd_totals(sd, k, order, npts, nreq):
    """Items of an odd number of doubles: the 8-byte copy loop instead of the 16-byte flush."""
    P = requests_per_item(sd, k, order, npts)
    reqsize = len(R.mis(sd, order)) * R.ndof(sd, k) * npts
    assert (min(P, nreq) * reqsize) % 2 == 1 or (nreq % P) * reqsize % 2 == 1
    run(sd, k, order, npts, nreq, np.random.default_rng(nreq))


OFFSET_SHAPES = [(2, 2, 1, 9, 1), (3, 3, 1, 27, 1), (3, 2, 2, 8, 3), (3, 6, 2, 64, 1), (3, 7, 1, 10, 1), (2, 2, 1, 9, 16)]


@pytest.mark.parametrize("sd,k,order,npts,offset", OFFSET_SHAPES)
def test_offset_out_with_guard_bands(sd, k, order, npts, offset):
    """An out= view at an 8-byte offset (and one on a line boundary): guards untouched, every entry written, equal to a
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
        rel_check(out.cpu().numpy(), R.tabulate(sd, k, order, pts), (sd, k, nreq))


def test_grid_stride():
    """More items than the grid holds: every workgroup takes several."""
    import torch
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    P = requests_per_item(2, 1, 0, 4)
    nreq = 2 * num_cu * 64 * P + P + 3
    sample = E.sample_requests(nreq, P, nitems_per_trip=num_cu * 64, k=16, seed=4)
    run(2, 1, 0, 4, nreq, np.random.default_rng(nreq), sample=sample)


FULL = [(2, 2, 1, 9, 200000), (3, 3, 1, 27, 20000)]


@pytest.mark.parametrize("sd,k,order,npts,nreq", FULL)
def test_full_size_batch(sd, k, order, npts, nreq):
    """One large batch per dimension, every entry against the restatement."""
    run(sd, k, order, npts, nreq, np.random.default_rng(nreq))


# ---- errors: nothing is launched -------------------------------------------------------------------------------------------

def test_errors_launch_nothing():
    import torch
    from fiat_amd import runtime
    el = unit(2, 2)
    pts = np.random.default_rng(0).uniform(size=(3, 4, 2))
    launched = []

    def count(call):
        names = E.launched(call)
        launched.extend(n for n in names if "serendipity" in n)

    def beyond_order():
        with pytest.raises(NotImplementedError, match="order 4"):
            el.tabulate_batch(4, pts)

    def beyond_degree():
        with pytest.raises(NotImplementedError, match="degree 13"):
            runtime.serendipity_tabulate_batch(2, 13, [0.0, 0.0], [1.0, 1.0], 0, pts)

    def wrong_dimension():
        with pytest.raises(ValueError):
            el.tabulate_batch(1, np.zeros((3, 4, 3)))

    def with_out():
        out = torch.full((3, 1, 8, 4), 7.0, dtype=torch.float64, device="cuda")
        with pytest.raises(ValueError):
            el.tabulate_batch(1, pts, out=out)
        assert bool((out == 7.0).all())

    for call in (beyond_order, beyond_degree, wrong_dimension, with_out):
        count(call)
    assert launched == []
    with pytest.raises(NotImplementedError):
        el.tabulate_batch(1, pts, verts=np.zeros((3, 4, 2)))
    with pytest.raises(ValueError, match="empty box"):
        runtime.serendipity_tabulate_batch(2, 2, [0.0, 1.0], [1.0, 1.0], 0, pts)
    # and a good call still works afterwards
    rel_check(el.tabulate_batch(1, pts).cpu().numpy(), R.tabulate(2, 2, 1, pts))
