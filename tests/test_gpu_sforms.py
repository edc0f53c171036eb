"""BDMCE / BDMCF and the trimmed serendipity families on the GPU: parity of tabulate / tabulate_batch with the reference's
fixtures (tests/golden/sforms.npz), metadata, entity dofs, entity= tabulation, every (class, cell, degree, order) on both
output routes against the NumPy evaluation of the descriptor (tests/sforms_reference.py), the tiling edges of the kernel,
and the errors.  Tolerances: the project's standing 1e-12 on values and 1e-10 on derivatives, in the norm
max|x - ref| / max(1, max|ref|), per request."""
import os
import re
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import edge_reference as E  # noqa: E402  (guarded outputs, request samples)
import make_golden_sforms as M  # noqa: E402
import sforms_reference as R  # noqa: E402

TOL_VAL, TOL_DER = 1e-12, 1e-10
G = np.load(os.path.join(HERE, "golden", "sforms.npz"))
_ELS = {}

# (class key of make_golden_sforms, cell, degree): the table of the issue
ALL = [(c, "quad", k) for c in M.CLASSES for k in range(1, 7)] + \
      [(c, "hex", k) for c, ks in M.HEX_DEGREES.items() for k in ks]


def element(name):
    import fiat_amd
    if name not in _ELS:
        _ELS[name] = M.build(fiat_amd, name)
    return _ELS[name]


def unit(c, kind, k):
    """Class ``c`` of degree k on the UFC quadrilateral / hexahedron."""
    import fiat_amd
    from importlib import import_module
    key = (c, kind, k)
    if key not in _ELS:
        module, cls = M.CLASSES[c]
        _ELS[key] = getattr(import_module("fiat_amd." + module), cls)(M.cell(fiat_amd, kind), k)
    return _ELS[key]


def rel_check(got, ref, what=""):
    """Per request: (ntab, nrows, sd, npts) tables, values and derivatives apart."""
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


def report(el, order, npts):
    """(instance, route, P, image budget in bytes) of the route report."""
    m = re.fullmatch(r"(fxk::sforms_kernel<\d,\d>) (image|stream) P=(\d+) budget=(\d+)", el.kernel(order, npts))
    assert m, el.kernel(order, npts)
    return m.group(1), m.group(2), int(m.group(3)), int(m.group(4))


def point_bytes(el, order):
    """Bytes of one request per point."""
    return len(R.mis(el.fdim, order)) * el.num_rows() * el.fdim * 8


def expected_route(el, order, npts):
    """The route as the header documents it, from the reported budget: a request that fits goes through the image, the
    item shrunk to the requests that fit together."""
    budget = report(el, order, npts)[3]
    whole = 64 // npts if npts <= 64 else 1
    req = point_bytes(el, order) * npts
    if req <= budget:
        return "image", min(whole, budget // req)
    return "stream", whole


def run(el, order, npts, nreq, rng, sample=None, route=None):
    """``nreq`` requests with points in [-0.1, 1.1] on the unit box, ``sample`` (default: all) against the restatement."""
    import torch
    sd = el.fdim
    name, got_route, P, _ = report(el, order, npts)
    assert name == f"fxk::sforms_kernel<{sd},{order}>"
    assert (got_route, P) == expected_route(el, order, npts)
    if route is not None:
        assert got_route == route
    pts = rng.uniform(-0.1, 1.1, size=(nreq, npts, sd))
    out = el.tabulate_batch(order, pts)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (nreq, len(R.mis(sd, order)), el.num_rows(), sd, npts) == el.out_shape(order, nreq, npts)
    idx = np.arange(nreq) if sample is None else sample
    got = out[torch.as_tensor(idx, device=out.device)].cpu().numpy()
    coef, codes = el.descriptor()
    rel_check(got, R.tabulate(coef, codes, el.degree(), order, pts[idx]), (type(el).__name__, el.degree(), order, npts, nreq))
    assert bool(torch.isfinite(out).all())
    return out


# ---- the reference's fixtures ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(M.CASES))
def test_tabulate_against_fixture(name):
    c, kind, k, order = M.CASES[name]
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
    c, kind, k, order = M.CASES[name]
    el = element(name)
    sd = el.get_reference_element().get_spatial_dimension()
    assert list(M.metadata(el)) == list(G[f"{name}_meta"])
    assert el.degree() == k and el.get_order() == k and el.value_shape() == (sd,)
    assert el.get_formdegree() == (sd - 1 if c == "smd" else 1)
    contravariant = c in ("bdmcf", "smf", "smd")
    assert el.mapping() == ["contravariant piola" if contravariant else "covariant piola"] * el.space_dimension()
    assert np.array_equal(M.eids_rows(el.entity_dofs()), G[f"{name}_eids"])
    assert np.array_equal(M.eids_rows(el.entity_closure_dofs()), G[f"{name}_cids"])
    for method in (el.get_coeffs, el.dual_basis):
        with pytest.raises(NotImplementedError):
            method()


def test_registry_and_constructor_as_the_reference():
    import fiat_amd
    from fiat_amd import reference_element as RE
    S = fiat_amd.supported_elements
    assert S["Brezzi-Douglas-Marini Cube Edge"] is fiat_amd.BrezziDouglasMariniCubeEdge
    assert S["Brezzi-Douglas-Marini Cube Face"] is fiat_amd.BrezziDouglasMariniCubeFace
    assert S["SminusE"] is fiat_amd.TrimmedSerendipityEdge and S["SminusF"] is fiat_amd.TrimmedSerendipityFace
    assert S["SminusCurl"] is fiat_amd.TrimmedSerendipityCurl and S["SminusDiv"] is fiat_amd.TrimmedSerendipityDiv
    quad, hexa = RE.UFCQuadrilateral(), RE.UFCHexahedron()
    for cls in (S["Brezzi-Douglas-Marini Cube Edge"], S["Brezzi-Douglas-Marini Cube Face"], S["SminusE"], S["SminusF"],
                S["SminusCurl"], S["SminusDiv"]):
        with pytest.raises(Exception, match="only valid for k >= 1"):
            cls(quad, 0)
        with pytest.raises(Exception, match="only valid for dimension"):
            cls(fiat_amd.UFCInterval(), 2)
        with pytest.raises(NotImplementedError):
            cls(quad, 7)
    for cls in (S["Brezzi-Douglas-Marini Cube Edge"], S["Brezzi-Douglas-Marini Cube Face"], S["SminusF"]):
        with pytest.raises(Exception, match="only valid for dimension 2"):
            cls(hexa, 2)
    with pytest.raises(NotImplementedError, match="disagree"):
        S["SminusE"](hexa, 4)
    with pytest.raises(NotImplementedError, match="two Legendre polynomials"):
        S["SminusCurl"](hexa, 6)
    # the degree-1 trimmed quadrilateral elements: 5 counted, 4 listed and tabulated
    el = unit("smc", "quad", 1)
    assert el.space_dimension() == 5 and el.tabulate(0, np.zeros((1, 2)))[(0, 0)].shape == (4, 2, 1)


@pytest.mark.parametrize("name,key,edim", M.ENTITIES)
def test_entity_tabulation(name, key, edim):
    el = element(name)
    sd = el.get_reference_element().get_spatial_dimension()
    p, ref = G[M.ent_name(name, key) + "_pts"], G[M.ent_name(name, key) + "_tab"]
    rel_check(stack(el.tabulate(1, p, entity=key), sd, 1)[None], ref[None], (name, key))
    dev = el.tabulate_batch(1, np.stack([p, p[::-1]]), entity=key).cpu().numpy()
    rel_check(dev, np.stack([ref, ref[..., ::-1]]), (name, key))
    # the cell itself as the entity: the points as they are
    cell_key = (el.get_reference_element().get_dimension(), 0)
    q = G[f"{name}_pts"]
    assert np.array_equal(stack(el.tabulate(1, q, entity=cell_key), sd, 1), stack(el.tabulate(1, q), sd, 1))


def test_finat_adapter_accepts_the_element():
    from fiat_amd import finat_adapter as ad
    el = unit("smd", "hex", 2)
    fe = ad.FiatElement(el)
    assert fe.value_shape == (3,) and fe.mapping == "contravariant piola" and fe.formdegree == 2
    pts = np.random.default_rng(5).uniform(size=(2, 6, 3))
    ref = R.tabulate(*el.descriptor(), 2, 2, pts)
    res = fe.basis_evaluation(2, ad.PointSet(pts[0]))
    bres = fe.basis_evaluation_batch(2, pts)
    for t, alpha in enumerate(R.mis(3, 2)):
        tol = TOL_VAL if t == 0 else TOL_DER
        assert res[alpha].array.shape == (21, 3, 6)
        assert R.rel_err(res[alpha].array, ref[0, t]) <= tol
        assert R.rel_err(bres[alpha].array.cpu().numpy(), ref[:, t]) <= tol


# ---- every instance and route ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("c,kind,k", ALL)
def test_instances_and_routes(c, kind, k):
    """Every (class, cell, degree, order): the image route at 3 points with 2 P + 1 requests (at 1 point where 3 do not fit
    the budget; the largest hexahedral tables of derivatives fit at no point count), and streaming at 64 points with
    3 requests where that exceeds the image."""
    el = unit(c, kind, k)
    for order in range(3):
        rng = np.random.default_rng(k * 10 + order)
        budget = report(el, order, 3)[3]
        q = point_bytes(el, order)
        for npts in (3, 1):
            if q * npts <= budget:
                P = report(el, order, npts)[2]
                run(el, order, npts, 2 * P + 1, rng, route="image")
                break
        else:
            assert kind == "hex" and k >= 4 and order >= 1
        if q * 64 > budget:
            run(el, order, 64, 3, rng, route="stream")


def test_zero_components_are_exact_zeros():
    import torch
    rng = np.random.default_rng(11)
    for c, kind, k, order, npts in [("bdmcf", "quad", 3, 2, 5), ("smc", "hex", 3, 1, 2), ("smd", "hex", 4, 1, 64)]:
        el = unit(c, kind, k)
        out = el.tabulate_batch(order, rng.uniform(-0.1, 1.1, size=(4, npts, el.fdim)))
        zero = torch.as_tensor(el.descriptor()[0] == 0.0, device=out.device)
        frac = float(zero.double().mean())
        assert frac > (0.35 if kind == "quad" else 0.55)         # FIAT's layout: about half / two thirds of the entries
        assert bool((out[:, :, zero] == 0.0).all())
        assert bool((out[:, 0][:, ~zero] != 0.0).any())


# ---- tiling edges ------------------------------------------------------------------------------------------------------

POINT_COUNTS = [1, 7, 21, 32, 33, 63, 64, 65, 130]
# a quadrilateral on the image route at every count, a hexahedron whose item shrinks, one that streams from 3 points on
POINT_ELEMENTS = [("bdmce", "quad", 1, 0), ("smd", "hex", 1, 1), ("smc", "hex", 3, 1)]


@pytest.mark.parametrize("npts", POINT_COUNTS)
@pytest.mark.parametrize("c,kind,k,order", POINT_ELEMENTS)
def test_point_counts(c, kind, k, order, npts):
    """Every point count with every remainder of the last item: nreq in {1, P - 1, P, P + 1, 3 P + 2}."""
    el = unit(c, kind, k)
    route, P = expected_route(el, order, npts)
    if c == "bdmce":
        assert route == "image"
    if c == "smd" and npts == 7:
        assert route == "image" and P < 64 // npts
    if c == "smc" and npts >= 7:
        assert route == "stream"
    for nreq in E.nreq_list(P):
        run(el, order, npts, nreq, np.random.default_rng(npts * 13 + nreq))


def test_every_requests_per_item():
    """BDMCE_1 values: 8 x 2 doubles per point, so P = 64 // npts for every npts; a partial last item for each."""
    el = unit("bdmce", "quad", 1)
    seen = set()
    for npts in range(1, 66):
        P = report(el, 0, npts)[2]
        assert P == (64 // npts if npts <= 64 else 1)
        if P in seen:
            continue
        seen.add(P)
        run(el, 0, npts, 2 * P + max(1, P // 2), np.random.default_rng(npts), route="image")
    assert seen == {64 // n for n in range(1, 65)}


@pytest.mark.parametrize("c,kind,k,order", [("smd", "hex", 2, 1), ("bdmcf", "quad", 4, 2)])
def test_image_boundary(c, kind, k, order):
    """The largest request that fits the reported image budget and the first that does not."""
    el = unit(c, kind, k)
    budget = report(el, order, 1)[3]
    below = budget // point_bytes(el, order)
    above = below + 1
    assert 1 <= below and above <= 64
    assert report(el, order, below)[3] == budget == report(el, order, above)[3]
    assert report(el, order, below)[1:3] == ("image", 1)
    assert report(el, order, above)[1:3] == ("stream", 64 // above)
    run(el, order, below, 5, np.random.default_rng(below), route="image")
    run(el, order, above, 3 * (64 // above) + 1, np.random.default_rng(above), route="stream")


@pytest.mark.parametrize("k,npts,nreq", [(2, 3, 5), (3, 1, 30), (2, 1, 7)])
def test_odd_totals(k, npts, nreq):
    """Items of an odd number of doubles (SminusDiv values on the hexahedron: an odd number of rows times 3 components):
    the 8-byte copy loop instead of the 16-byte flush, and later items that start 8 bytes off a 16-byte boundary."""
    el = unit("smd", "hex", k)
    route, P = expected_route(el, 0, npts)
    reqsize = el.num_rows() * 3 * npts
    assert route == "image" and (min(P, nreq) * reqsize) % 2 == 1
    run(el, 0, npts, nreq, np.random.default_rng(nreq), route="image")


OFFSET_SHAPES = [("bdmcf", "quad", 1, 1, 9, 1), ("smd", "hex", 1, 1, 7, 1), ("smc", "hex", 2, 1, 27, 1), ("smd", "quad", 2, 1, 9, 16),
                 ("sme", "hex", 3, 2, 64, 16)]


@pytest.mark.parametrize("c,kind,k,order,npts,offset", OFFSET_SHAPES)
def test_offset_out_with_guard_bands(c, kind, k, order, npts, offset):
    """An out= view at an 8-byte offset (and one on a line boundary): guards untouched, every entry written, equal to a
    fresh out and to the restatement."""
    import torch
    el = unit(c, kind, k)
    P = report(el, order, npts)[2]
    for nreq in (P, 3 * P + 1):
        pts = np.random.default_rng(npts + nreq).uniform(-0.1, 1.1, size=(nreq, npts, el.fdim))
        fresh = el.tabulate_batch(order, pts)
        buf, out = E.guarded_out(tuple(fresh.shape), offset, fresh.device)
        assert el.tabulate_batch(order, pts, out=out) is out
        torch.cuda.synchronize()
        E.check_guarded(buf, out)
        assert torch.equal(out, fresh)
        rel_check(out.cpu().numpy(), R.tabulate(*el.descriptor(), k, order, pts), (c, kind, k, nreq))


def test_grid_stride():
    """More items than the grid holds: every workgroup takes several."""
    import torch
    el = unit("bdmce", "quad", 1)
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    P = report(el, 0, 4)[2]
    assert P == 16
    nreq = 2 * num_cu * 64 * P + P + 3
    sample = E.sample_requests(nreq, P, nitems_per_trip=num_cu * 64, k=16, seed=4)
    run(el, 0, 4, nreq, np.random.default_rng(nreq), sample=sample, route="image")


# ---- errors: nothing is launched -------------------------------------------------------------------------------------------

def test_errors_launch_nothing():
    import torch
    from fiat_amd import reference_element as RE
    from fiat_amd import runtime
    import fiat_amd
    el = unit("bdmcf", "quad", 2)
    el.tabulate_batch(0, np.zeros((1, 1, 2)))       # the term table is on the device before anything is counted
    pts = np.random.default_rng(0).uniform(size=(3, 4, 2))
    launched = []

    def count(call):
        names = E.launched(call)
        launched.extend(n for n in names if "sforms" in n)

    def beyond_order():
        with pytest.raises(NotImplementedError, match="order 3"):
            el.tabulate_batch(3, pts)
        with pytest.raises(NotImplementedError, match="order 3"):
            runtime.sforms_tabulate_batch(el._table(), el._lo, el._hi, 3, pts)

    def beyond_degree():
        with pytest.raises(NotImplementedError, match="degree 7"):
            fiat_amd.TrimmedSerendipityDiv(RE.UFCQuadrilateral(), 7)
        with pytest.raises(NotImplementedError, match="degree 7"):
            runtime.SFormsTable(2, 7, np.ones((4, 2)), np.zeros((4, 2, 2), dtype=np.int32))
        with pytest.raises(ValueError, match="outside the 1-D family"):
            runtime.SFormsTable(2, 1, np.ones((4, 2)), np.full((4, 2, 2), 6, dtype=np.int32))

    def wrong_dimension():
        with pytest.raises(ValueError):
            el.tabulate_batch(1, np.zeros((3, 4, 3)))

    def with_out():
        out = torch.full((3, 3, 14, 4), 7.0, dtype=torch.float64, device="cuda")       # the component axis is missing
        with pytest.raises(ValueError):
            el.tabulate_batch(1, pts, out=out)
        assert bool((out == 7.0).all())

    def with_verts():
        with pytest.raises(NotImplementedError, match="per-request cells"):
            el.tabulate_batch(1, pts, verts=np.zeros((3, 4, 2)))

    def empty_box():
        with pytest.raises(ValueError, match="empty box"):
            runtime.sforms_tabulate_batch(el._table(), [0.0, 1.0], [1.0, 1.0], 0, pts)

    for call in (beyond_order, beyond_degree, wrong_dimension, with_out, with_verts, empty_box):
        count(call)
    assert launched == []
    # and a good call still works afterwards
    rel_check(el.tabulate_batch(1, pts).cpu().numpy(), R.tabulate(*el.descriptor(), 2, 1, pts))
    # pushforward changes nothing
    assert torch.equal(el.tabulate_batch(1, pts, pushforward=True), el.tabulate_batch(1, pts))
