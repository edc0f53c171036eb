"""``tabulate_on_cells`` and ``cell_geometry_batch`` on the GPU: the fused kernel of 1-D Lagrange products and the general pass
against the NumPy restatement (tests/cellmap_reference.py), which is fed the element's own reference tables; closed-form checks
that do not use the restatement; the reference's fixture (tests/golden/cellmap.npz); the refusals.  Cells are the box moved by
up to 15 % of its edges per corner coordinate (det J >= 0.39), points lie in the box.  Tolerances are the project's bars,
1e-12 on values and 1e-10 on derivatives in the norm max|x - ref| / max(1, max|ref|)."""
import itertools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import cellmap_reference as R  # noqa: E402
import edge_reference as E  # noqa: E402  (guarded outputs, launched kernels, request counts, grid points)
import instance_manifest  # noqa: E402  (kernel names as the profiler and the code object spell them)
import make_golden_cellmap as M  # noqa: E402
import make_golden_hdivcurl as MH  # noqa: E402

G = np.load(os.path.join(HERE, "golden", "cellmap.npz"))
_ELS = {}


def cached(key, make):
    if key not in _ELS:
        _ELS[key] = make()
    return _ELS[key]


def Q(sd, *degrees, gll=False):
    """Q_(k0, k1[, k2]) on the unit cell (one degree: the same in every direction)."""
    import fiat_amd as F
    degrees = degrees * sd if len(degrees) == 1 else degrees

    def make():
        I = F.ufc_simplex(1)
        fs = [(F.GaussLobattoLegendre if gll else F.Lagrange)(I, k) for k in degrees]
        el = F.TensorProductElement(fs[0], fs[1])
        return el if sd == 2 else F.TensorProductElement(el, fs[2])
    return cached(("Q", sd, degrees, gll), make)


def family(name):
    import fiat_amd as F
    from fiat_amd.reference_element import UFCHexahedron, UFCQuadrilateral
    make = {"q32": lambda: Q(2, 3, 2), "s2": lambda: F.Serendipity(UFCQuadrilateral(), 2), "s3": lambda: F.Serendipity(UFCHexahedron(), 3),
            "bdmcf1": lambda: F.BrezziDouglasMariniCubeFace(UFCQuadrilateral(), 1),
            "sminuscurl1": lambda: F.TrimmedSerendipityCurl(UFCHexahedron(), 1), "dpc2": lambda: F.DPC(UFCQuadrilateral(), 2)}
    return cached(name, make.get(name, lambda: MH.build(F, name)))


def sd_of(el):
    return el.get_reference_element().get_spatial_dimension()


def plan_p(el, order, npts, push=False, grid=False):
    from fiat_amd import cellmap
    return int(cellmap.kernel(el, order, npts, push, grid).split("P=")[1].split()[0])


def instance(el, order, npts, push=False, grid=False):
    from fiat_amd import cellmap
    return cellmap.kernel(el, order, npts, push, grid).split(": ", 1)[1].split("+ ")[-1].split()[0]


def kernels_of(call):
    return set(instance_manifest.normalise_all(sorted(E.launched(call))))


def batch(el, nreq, npts, seed, grid=False):
    """(points as passed, explicit points, corners) of a seeded batch on the unit cell."""
    sd = sd_of(el)
    rng = np.random.default_rng(seed)
    corners = R.perturbed_cells(rng, nreq, sd)
    if grid:
        g = rng.uniform(0.0, 1.0, size=(nreq, sd, npts))
        return g, E.grid_points(g), corners
    pts = R.box_points(rng, nreq, npts, np.zeros(sd), np.ones(sd))
    return pts, pts, corners


def restated(el, order, pts, corners, push=False):
    sd = sd_of(el)
    ref = el.tabulate_batch(order, pts).cpu().numpy()
    return R.apply(np.zeros(sd), np.ones(sd), pts, corners, ref, R.MAPPINGS[el.mapping()[0]] if push else R.AFFINE)


def each(cases, fn):
    """fn(*case) for every case of a group, all of them even after one fails (whatever it raises); the failing cases are
    reported together, each with its arguments."""
    failed = []
    for case in cases:
        try:
            fn(*(case if isinstance(case, tuple) else (case,)))
        except Exception as e:      # noqa: BLE001  (reported below, with the case)
            failed.append((case, f"{type(e).__name__}: {str(e)[:400]}"))
    assert not failed, failed


def close(got, want, what):
    e0, e1 = R.errors(got, want)
    print(f"{what}: values {e0:.2e} derivatives {e1:.2e}")
    assert e0 <= R.VALUES and e1 <= R.DERIVATIVES, (what, e0, e1)


# ---- the fused route -----------------------------------------------------------------------------------------------------

def _fused_against_restatement(sd, k, order, npts):
    """Q1 and Q2, guarded outputs at offsets 0 and 1 doubles (the chunked flush and the copy loop), 3 P + 2 requests (whole
    items and a partial last one), exactly the named instance launched."""
    import torch
    from fiat_amd import cellmap
    el = Q(sd, k)
    P = plan_p(el, order, npts)
    nreq = 3 * P + 2 if npts <= 9 else 3
    pts, _, corners = batch(el, nreq, npts, 1000 * sd + 100 * k + npts)
    want = restated(el, order, pts, corners)
    name = f"fxk::cellmap_tensor_kernel<{sd},{k + 1},{order},false>"
    assert instance(el, order, npts) == name
    for off in (0, 1):
        buf, out = E.guarded_out(want.shape, off, "cuda")
        if off == 0:
            assert kernels_of(lambda: cellmap.tabulate_on_cells(el, order, pts, corners, out=out)) == {name}
        else:
            assert cellmap.tabulate_on_cells(el, order, pts, corners, out=out) is out
        torch.cuda.synchronize()
        E.check_guarded(buf, out)
        close(out.cpu().numpy(), want, f"Q{k} sd {sd} order {order} npts {npts} offset {off}")


def _fused_request_counts(sd, k, npts):
    """nreq around the item size P: one request, a partial item, whole items, one more, several items and a rest."""
    from fiat_amd import cellmap
    el = Q(sd, k)
    P = plan_p(el, 1, npts)
    assert 1 < P <= 64 // npts
    for nreq in E.nreq_list(P):
        pts, _, corners = batch(el, nreq, npts, nreq)
        close(cellmap.tabulate_on_cells(el, 1, pts, corners).cpu().numpy(), restated(el, 1, pts, corners), f"nreq {nreq} of P {P}")


def test_fused_q4_hexahedron_grid_streams():
    """The benchmark family: Q4 on hexahedra at a 5-point grid, 125 points in three chunks, rows streamed."""
    import torch
    from fiat_amd import cellmap
    el = Q(3, 4)
    g, pts, corners = batch(el, 3, 5, 44, grid=True)
    assert "stream P=1" in cellmap.kernel(el, 1, 5, grid=True)
    want = restated(el, 1, pts, corners)
    buf, out = E.guarded_out(want.shape, 1, "cuda")
    assert kernels_of(lambda: cellmap.tabulate_on_cells(el, 1, g, corners, out=out, grid=True)) == {"fxk::cellmap_tensor_kernel<3,5,1,true>"}
    E.check_guarded(buf, out)
    close(out.cpu().numpy(), want, "Q4 hexahedron grid")
    explicit = cellmap.tabulate_on_cells(el, 1, pts, corners)
    assert torch.equal(explicit, out)


def test_fused_other_nodes():
    """GLL nodes, and more distinct node sets than the library keeps on the device (64): the node-data cache starts over and
    every call still gets the data of its own nodes."""
    _fused_gll_nodes()
    import torch
    from fiat_amd import runtime
    rng = np.random.default_rng(8)
    lo, hi = np.zeros(2), np.ones(2)
    pts, corners = R.box_points(rng, 5, 9, lo, hi), R.perturbed_cells(rng, 5, 2)
    ctx = runtime.Context.get()
    dpts, dcorners = runtime._as_device(pts, ctx), runtime._as_device(corners, ctx)
    sets = [np.array([0.0, 0.5, 1.0]) + rng.uniform(-0.2, 0.2, size=(2, 3)) for _ in range(70)]      # (gaps of 0.1 at least)
    outs = []
    for nodes in sets + sets[:3]:                                      # (the first sets again, after the cache started over)
        out = torch.empty((5, 3, 9, 9), dtype=torch.float64, device=ctx.device)
        outs.append(runtime.cellmap_tensor_batch(2, np.ascontiguousarray(nodes), lo, hi, 1, dpts, dcorners, out))
    for nodes, out in zip(sets + sets[:3], outs):
        lines = [E.line_lagrange_reference(nodes[d], pts[..., d].ravel(), 1).astype(float) for d in range(2)]
        ref = np.stack([np.einsum("ip,jp->ijp", lines[0][a], lines[1][b]).reshape(9, 5, 9) for a, b in ((0, 0), (1, 0), (0, 1))])
        want = R.apply(lo, hi, pts, corners, np.moveaxis(ref, 2, 0))
        close(out.cpu().numpy(), want, "random nodes")


def _fused_gll_nodes():
    from fiat_amd import cellmap
    el = Q(2, 3, gll=True)
    pts, _, corners = batch(el, 9, 9, 5)
    assert instance(el, 1, 9) == "fxk::cellmap_tensor_kernel<2,4,1,false>"
    close(cellmap.tabulate_on_cells(el, 1, pts, corners).cpu().numpy(), restated(el, 1, pts, corners), "Q3 GLL")
    # the node itself: the barycentric formula's exact Kronecker delta
    nodes = np.array([list(n.get_point_dict().keys())[0] for n in el.dual_basis()])[None]
    vals = cellmap.tabulate_on_cells(el, 0, nodes, corners[:1]).cpu().numpy()[0, 0]
    assert np.array_equal(vals, np.eye(16))


def _grid_input_equals_explicit_points(sd, k, q, order):
    import torch
    from fiat_amd import cellmap
    el = Q(sd, k)
    nreq = 2 * plan_p(el, order, q, grid=True) + 1
    g, pts, corners = batch(el, nreq, q, 7 + q, grid=True)
    a = cellmap.tabulate_on_cells(el, order, g, corners, grid=True)
    b = cellmap.tabulate_on_cells(el, order, pts, corners)
    assert torch.equal(a, b)
    close(a.cpu().numpy(), restated(el, order, pts, corners), f"grid Q{k} sd {sd} q {q}")
    c = cellmap.tabulate_on_cells(el, order, g, corners, grid=True, route="general")        # the pass expands the grid itself
    assert R.rel(c.cpu().numpy(), a.cpu().numpy()) <= 1e-13


def _fused_agrees_with_general(sd, k, order, npts):
    from fiat_amd import cellmap
    el = Q(sd, k)
    pts, _, corners = batch(el, 5, npts, 3 * npts + k)
    fused = cellmap.tabulate_on_cells(el, order, pts, corners, route="fused").cpu().numpy()
    names = kernels_of(lambda: cellmap.tabulate_on_cells(el, order, pts, corners, route="general"))
    assert not [n for n in names if "cellmap_tensor_kernel" in n] and (order == 0 or f"fxk::cellmap_apply_kernel<{sd},{order},0>" in names)
    general = cellmap.tabulate_on_cells(el, order, pts, corners, route="general").cpu().numpy()
    assert R.rel(fused, general) <= 1e-13


# ---- the general route ---------------------------------------------------------------------------------------------------

FAMILIES = ["q32", "rtcf1d0", "rtce2d0", "ncf1d0", "nce1d0", "s2", "s3", "bdmcf1", "sminuscurl1", "dpc2"]
VECTOR = {"rtcf1d0": 2, "rtce2d0": 1, "ncf1d0": 2, "nce1d0": 1, "bdmcf1": 2, "sminuscurl1": 1}           # FX_MAP_* of the family
GENERAL_CASES = [(n, False) for n in FAMILIES] + [(n, True) for n in FAMILIES if n in VECTOR]


def _general_against_restatement(name, push, order):
    """Every family once per mapping it has, at 1, 9, 65 and 130 points (P = 64, 7, 1 in two and in three chunks), the
    launched kernels exactly the element's own and the named instance of the pass, guarded outputs at offsets 0 and 1 doubles,
    and the pass in place equal to the pass out of place bit for bit."""
    import torch
    from fiat_amd import cellmap, runtime
    el = family(name)
    sd = sd_of(el)
    code = VECTOR[name] if push else 0
    assert R.MAPPINGS[el.mapping()[0]] == VECTOR.get(name, 0)
    for npts in (1, 9, 65, 130):
        nreq = {1: 70, 9: 16}.get(npts, 2)
        pts, _, corners = batch(el, nreq, npts, 31 * npts + order)
        ref = el.tabulate_batch(order, pts)
        want = R.apply(np.zeros(sd), np.ones(sd), pts, corners, ref.cpu().numpy(), code)
        inst = f"fxk::cellmap_apply_kernel<{sd},{order},{code}>"
        assert instance(el, order, npts, push) == inst
        passes = {inst} if order == 1 or code != 0 else set()           # (values of the affine map: nothing to do in place)
        for off in (0, 1):
            buf, out = E.guarded_out(want.shape, off, "cuda")
            own = kernels_of(lambda: el.tabulate_batch(order, pts, out=out))
            assert own and not [n for n in own if "cellmap" in n], own
            names = kernels_of(lambda: cellmap.tabulate_on_cells(el, order, pts, corners, out=out, pushforward=push))
            assert names == own | passes, (names, own, passes)          # exactly the element's own kernel(s) and the pass
            E.check_guarded(buf, out)
            close(out.cpu().numpy(), want, f"{name} push {push} order {order} npts {npts} offset {off}")
        apart = torch.full_like(ref, float("nan"))
        dpts, dcorners = runtime._as_device(pts, runtime.Context.get()), runtime._as_device(corners, runtime.Context.get())
        assert kernels_of(lambda: runtime.cellmap_apply(sd, code, order, np.zeros(sd), np.ones(sd), dpts, dcorners, ref, out=apart)) == {inst}
        assert torch.equal(apart, out)


# ---- closed forms, independent of the restatement -----------------------------------------------------------------------

def q1_images(corners, X):
    """x(X) of one cell from the definition: corners (2^sd, sd), X (n, sd) on the unit cell."""
    sd = X.shape[1]
    x = np.zeros_like(X)
    for i, b in enumerate(itertools.product((0, 1), repeat=sd)):
        x += np.prod([X[:, d] if b[d] else 1 - X[:, d] for d in range(sd)], axis=0)[:, None] * corners[i]
    return x


def _linear_reproduction(sd, k, route):
    """a . x + b lies in Q_k on the mapped cell (x itself is Q1), so its nodal interpolant has the gradient a at every
    point: sum_i (a . x(X_i) + b) grad_x phi_i = a, to 1e-10."""
    from fiat_amd import cellmap
    el = Q(sd, k)
    nodes = np.array([list(n.get_point_dict().keys())[0] for n in el.dual_basis()])
    pts, _, corners = batch(el, 6, 11, 17 * k + sd)
    rng = np.random.default_rng(k)
    a, b = rng.standard_normal(sd), rng.standard_normal()
    out = cellmap.tabulate_on_cells(el, 1, pts, corners, route=route).cpu().numpy()
    assert ("fused" in cellmap.kernel(el, 1, 11)) == (k <= 4)
    for r in range(len(pts)):
        u = q1_images(corners[r], nodes) @ a + b
        grad = np.einsum("i,dip->dp", u, out[r, 1:])
        assert np.abs(grad - a[:, None]).max() <= 1e-10, (r, np.abs(grad - a[:, None]).max())
        assert np.abs(np.einsum("i,ip->p", u, out[r, 0]) - (q1_images(corners[r], pts[r]) @ a + b)).max() <= 1e-12


def _divergence_identity(name):
    """div_x phi = div_X Phi / det J from the output's gradient tables, det J from cell_geometry_batch, to 1e-10."""
    from fiat_amd import cell_geometry_batch, cellmap
    el = family(name)
    sd = sd_of(el)
    pts, _, corners = batch(el, 6, 9, 23)
    ref = el.tabulate_batch(1, pts).cpu().numpy()
    out = cellmap.tabulate_on_cells(el, 1, pts, corners, pushforward=True).cpu().numpy()
    det = cell_geometry_batch(el.get_reference_element(), pts, corners)[2].cpu().numpy()
    div = lambda t: sum(t[:, 1 + d, :, d] for d in range(sd))       # noqa: E731
    assert np.abs(div(out) - div(ref) / det[:, None, :]).max() <= 1e-10


def _curl_identity(name):
    """curl_x phi = J curl_X Phi / det J (the scalar curl_X Phi / det J on quadrilaterals), to 1e-10."""
    from fiat_amd import cell_geometry_batch, cellmap
    el = family(name)
    sd = sd_of(el)
    pts, _, corners = batch(el, 6, 9, 29)
    ref = el.tabulate_batch(1, pts).cpu().numpy()
    out = cellmap.tabulate_on_cells(el, 1, pts, corners, pushforward=True).cpu().numpy()
    _, J, det = (t.cpu().numpy() for t in cell_geometry_batch(el.get_reference_element(), pts, corners))
    if sd == 2:
        curl = lambda t: t[:, 1, :, 1] - t[:, 2, :, 0]                # noqa: E731  d_0 phi_1 - d_1 phi_0
        assert np.abs(curl(out) - curl(ref) / det[:, None, :]).max() <= 1e-10
    else:
        curl = lambda t: np.stack([t[:, 2, :, 2] - t[:, 3, :, 1], t[:, 3, :, 0] - t[:, 1, :, 2], t[:, 1, :, 1] - t[:, 2, :, 0]], 2)  # noqa: E731
        want = np.einsum("rpab,ribp->riap", J, curl(ref)) / det[:, None, None, :]
        assert np.abs(curl(out) - want).max() <= 1e-10


def _parallelogram_cells_have_the_constant_jacobian_closed_form(name, push):
    """corners = v0 + A (unit vertices): J = A everywhere, the tables are M Phi and M d Phi A^-1 with the constant M."""
    from fiat_amd import cellmap
    el = {"q2": lambda: Q(2, 2), "q2hex": lambda: Q(3, 2)}.get(name, lambda: family(name))()
    sd = sd_of(el)
    rng = np.random.default_rng(3)
    nreq = 9
    A = np.eye(sd) + 0.3 * rng.standard_normal((nreq, sd, sd))
    A[::3, :, 0] *= -1.0                                                  # every third cell reflected
    corners = np.einsum("rad,id->ria", A, R.unit_corners(sd)) + rng.standard_normal((nreq, 1, sd))
    pts = R.box_points(rng, nreq, 9, np.zeros(sd), np.ones(sd))
    ref = el.tabulate_batch(1, pts).cpu().numpy()
    Ainv = np.linalg.inv(A)
    if not push:
        Mc = np.broadcast_to(np.eye(sd), A.shape)
    elif el.mapping()[0] == "contravariant piola":
        Mc = A / np.linalg.det(A)[:, None, None]
    else:
        Mc = np.swapaxes(Ainv, 1, 2)
    want = np.empty_like(ref)
    if ref.ndim == 4:
        want[:, 0] = ref[:, 0]
        want[:, 1:] = np.einsum("reip,red->rdip", ref[:, 1:], Ainv)
    else:
        want[:, 0] = np.einsum("rck,rikp->ricp", Mc, ref[:, 0])
        want[:, 1:] = np.einsum("rck,reikp,red->rdicp", Mc, ref[:, 1:], Ainv)
    close(cellmap.tabulate_on_cells(el, 1, pts, corners, pushforward=push).cpu().numpy(), want, f"parallelogram {name}")


def _fixture_box_cases(name):
    """The reference's own tables.  Scalar cases: the unit-cell element mapped to the box's vertices is the reference's
    element built on the box.  Vector cases: the element built on the box (its tables are the reference's there) pushed to the
    fixture's cell against the generator's Piola image."""
    import fiat_amd
    from fiat_amd import cellmap
    sd, mapping = M.CASES[name]
    lo, hi = G[f"{name}_lo"], G[f"{name}_hi"]
    if mapping == "affine":
        el = cached(("unit", name), lambda: M.build(fiat_amd, name))
        got = cellmap.tabulate_on_cells(el, 1, G[f"{name}_X"][None], R.unit_corners(sd, lo, hi)[None])
        close(got.cpu().numpy(), G[f"{name}_tab"][None], name)
        return
    el = cached(("box", name), lambda: M.build(fiat_amd, name, M.BOX[sd]))
    assert [list(v) for v in cellmap.box_of(el.get_reference_element())[1:]] == [list(lo), list(hi)]
    close(el.tabulate_batch(1, G[f"{name}_x"][None]).cpu().numpy(), G[f"{name}_tab"][None], name + " on its box")
    got = cellmap.tabulate_on_cells(el, 1, G[f"{name}_x"][None], G[f"{name}_corners"][None], pushforward=True)
    close(got.cpu().numpy(), G[f"{name}_pushed"][None], name)


# ---- geometry, streams ---------------------------------------------------------------------------------------------------

def _cell_geometry_batch(sd):
    """x, J and det J against the restatement on a box that is not the unit cell; a reflected cell has det J < 0; the corners
    themselves come back at the box's vertices, in the order of get_vertices()."""
    import fiat_amd as F
    from fiat_amd import cell_geometry_batch
    lo, hi = G["q2hex_lo"][:sd], G["q2hex_hi"][:sd]
    I = [M.interval(F, lo[d], hi[d]) for d in range(sd)]
    cell = F.reference_element.TensorProductCell(*I)
    rng = np.random.default_rng(sd)
    nreq, npts = 70, 9
    corners = R.perturbed_cells(rng, nreq, sd, lo, hi)
    corners[1::2, :, 0] *= -1.0
    pts = R.box_points(rng, nreq, npts, lo, hi)
    x, J, det = (t.cpu().numpy() for t in cell_geometry_batch(cell, pts, corners))
    wx, wJ, wdet, _ = R.geometry(lo, hi, pts, corners)
    assert R.rel(x, wx) <= 1e-12 and R.rel(J, wJ) <= 1e-12 and R.rel(det, wdet) <= 1e-12
    assert (det[0::2] > 0).all() and (det[1::2] < 0).all()
    verts = np.broadcast_to(np.array(F.reference_element.flatten_reference_cube(cell).get_vertices()), (nreq, 2 ** sd, sd))
    assert np.abs(cell_geometry_batch(cell, verts.copy(), corners)[0].cpu().numpy() - corners).max() <= 1e-14
    unit = F.reference_element.ufc_hypercube(sd)
    one = np.zeros((1, 1, sd))
    one[0, 0, sd - 1] = 1.0                                              # the LAST coordinate runs fastest: vertex 1
    assert np.abs(cell_geometry_batch(unit, one, corners[:1])[0].cpu().numpy()[0, 0] - corners[0, 1]).max() <= 1e-14


def test_non_default_stream():
    import torch
    from fiat_amd import cell_geometry_batch, cellmap
    s = torch.cuda.Stream()
    for el, push in ((Q(2, 2), False), (family("rtcf1d0"), True)):
        pts, _, corners = batch(el, 40, 9, 2)
        want = cellmap.tabulate_on_cells(el, 1, pts, corners, pushforward=push)
        dpts, dcorners = torch.as_tensor(pts).cuda(), torch.as_tensor(corners).cuda()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            got = cellmap.tabulate_on_cells(el, 1, dpts, dcorners, stream=s, pushforward=push)
            geo = cell_geometry_batch(el.get_reference_element(), dpts, dcorners, stream=s)
        s.synchronize()
        assert torch.equal(got, want)
        assert torch.equal(geo[2], cell_geometry_batch(el.get_reference_element(), dpts, dcorners)[2])


# ---- the tests: one per group of cases -------------------------------------------------------------------------------------

def test_fused_against_restatement():
    """Q1 and Q2 on quadrilaterals and hexahedra, orders 0 and 1, at 1, 7, 9, 63, 64 and 65 points.  (_fused_against_restatement: what a case checks.)"""
    each([(sd, k, order, npts) for sd in (2, 3) for k in (1, 2) for order in (0, 1) for npts in (1, 7, 9, 63, 64, 65)], _fused_against_restatement)
    each([(2, 2, 9), (3, 2, 9), (3, 1, 7)], _fused_request_counts)          # request counts around the item size P


def test_grid_input_equals_explicit_points():
    """grid=True equals the explicit points of the same grid, bit for bit.  (_grid_input_equals_explicit_points: what a case checks.)"""
    each([(2, 2, 3, 1), (3, 1, 2, 1), (2, 4, 9, 0), (3, 3, 4, 1)], _grid_input_equals_explicit_points)


def test_fused_agrees_with_general():
    """route="fused" against route="general", to 1e-13.  (_fused_agrees_with_general: what a case checks.)"""
    each([(2, 1, 1, 9), (2, 2, 0, 9), (2, 4, 1, 65), (3, 1, 1, 7), (3, 2, 1, 64), (3, 4, 1, 9)], _fused_agrees_with_general)


def test_general_against_restatement():
    """Ten families, once per mapping each has, orders 0 and 1.  (_general_against_restatement: what a case checks.)"""
    each([(n, p, order) for n, p in GENERAL_CASES for order in (0, 1)], _general_against_restatement)


def test_linear_reproduction():
    """Linear reproduction through the nodal interpolant, both routes.  (_linear_reproduction: what a case checks.)"""
    each([(2, 1, None), (2, 3, None), (3, 2, None), (3, 4, None), (2, 2, "general"), (2, 5, None)], _linear_reproduction)


def test_divergence_and_curl_identities():
    """The div identity from the output gradient tables of the H(div) families and the curl identity of the H(curl) families.
    (_divergence_identity, _curl_identity: what a case checks.)"""
    each(["rtcf1d0", "ncf1d0", "bdmcf1"], _divergence_identity)
    each(["rtce2d0", "nce1d0", "sminuscurl1"], _curl_identity)


def test_parallelogram_cells_have_the_constant_jacobian_closed_form():
    """Parallelogram corners against the constant-Jacobian closed form.  (_parallelogram_cells_have_the_constant_jacobian_closed_form: what a case checks.)"""
    each([("q2", False), ("q2hex", False), ("rtcf1d0", True), ("nce1d0", True), ("s3", False)], _parallelogram_cells_have_the_constant_jacobian_closed_form)


def test_fixture_box_cases():
    """The fixture's box cases against the reference's tables.  (_fixture_box_cases: what a case checks.)"""
    each(sorted(M.CASES), _fixture_box_cases)


def test_cell_geometry_batch():
    """cell_geometry_batch on quadrilaterals and hexahedra, reflected cells included.  (_cell_geometry_batch: what a case checks.)"""
    each([2, 3], _cell_geometry_batch)


# ---- refusals ------------------------------------------------------------------------------------------------------------

class _DoublePiola:
    """An element whose mapping is a double Piola map (none of the cube families has one)."""

    def __init__(self, el):
        self._el = el

    def __getattr__(self, name):
        return getattr(self._el, name)

    def mapping(self):
        return ["double covariant piola"] * self._el.space_dimension()


def test_refusals():
    import fiat_amd as F
    import torch
    from fiat_amd import cell_geometry_batch, cellmap
    el = Q(2, 2)
    pts, _, corners = batch(el, 3, 9, 0)
    T = cellmap.tabulate_on_cells
    with pytest.raises(NotImplementedError, match="order 2"):
        T(el, 2, pts, corners)
    with pytest.raises(NotImplementedError, match="order 2"):
        cellmap.kernel(family("s2"), 2, 9)
    with pytest.raises(NotImplementedError, match="double covariant piola"):
        T(_DoublePiola(family("rtcf1d0")), 1, pts, corners, pushforward=True)
    tri = F.Lagrange(F.ufc_simplex(2), 2)
    with pytest.raises(NotImplementedError, match=r"tabulate_batch\(verts=\)"):
        T(tri, 1, pts, corners)
    with pytest.raises(NotImplementedError, match="dimension 1"):
        T(F.Lagrange(F.ufc_simplex(1), 2), 1, pts[..., :1], corners[:, :2, :1])
    # ... whatever the route: the cell is validated first
    with pytest.raises(NotImplementedError, match=r"tabulate_batch\(verts=\)"):
        T(tri, 1, pts, corners, route="fused")
    with pytest.raises(NotImplementedError, match="dimension 1"):
        T(F.Lagrange(F.ufc_simplex(1), 2), 1, pts[..., :1], corners[:, :2, :1], route="fused")
    prism = F.TensorProductElement(F.Lagrange(F.ufc_simplex(2), 1), F.Lagrange(F.ufc_simplex(1), 1))
    with pytest.raises(NotImplementedError, match="prisms"):
        T(prism, 1, np.zeros((3, 9, 3)), np.zeros((3, 8, 3)))
    with pytest.raises(NotImplementedError, match="prisms"):
        T(prism, 1, np.zeros((3, 9, 3)), np.zeros((3, 8, 3)), route="fused")
    with pytest.raises(NotImplementedError, match="order 2"):
        T(family("s2"), 2, pts, corners, route="fused")
    with pytest.raises(NotImplementedError, match="prisms"):
        cell_geometry_batch(prism.get_reference_element(), np.zeros((3, 9, 3)), np.zeros((3, 8, 3)))
    # the fused route where it does not apply
    with pytest.raises(NotImplementedError, match="unequal node counts"):
        T(family("q32"), 1, pts, corners, route="fused")
    with pytest.raises(NotImplementedError, match="6 nodes"):
        T(Q(2, 5), 1, pts, corners, route="fused")
    with pytest.raises(NotImplementedError, match="no product"):
        T(family("s2"), 1, pts, corners, route="fused")
    with pytest.raises(NotImplementedError, match="grid"):
        T(family("s2"), 1, np.zeros((3, 2, 3)), corners, grid=True)
    # everything else: ValueError before any launch
    launched = E.launched
    bad = [dict(points=pts[0]), dict(points=pts[..., :1]), dict(corners=corners[:2]), dict(corners=corners[:, :3]),
           dict(points=pts.astype(np.float32)), dict(corners=torch.as_tensor(corners, dtype=torch.float32)),
           dict(order=-1), dict(route="direct"), dict(out=torch.empty((3, 3, 9, 8), dtype=torch.float64, device="cuda")),
           dict(out=torch.empty((3, 3, 9, 9), dtype=torch.float32, device="cuda")), dict(out=torch.empty((3, 3, 9, 9), dtype=torch.float64)),
           dict(out=torch.empty((3, 3, 9, 18), dtype=torch.float64, device="cuda")[..., ::2]),
           dict(points=np.zeros((3, 9, 2)), grid=True)]
    for kw in bad:
        args = dict(order=1, points=pts, corners=corners)
        args.update(kw)

        def call():
            with pytest.raises(ValueError):
                T(el, args.pop("order"), args.pop("points"), args.pop("corners"), **args)
        assert not launched(call), kw
    with pytest.raises(ValueError, match="Piola map needs a vector"):
        T(_Mapped(el), 1, pts, corners, pushforward=True)
    with pytest.raises(ValueError, match="index arithmetic"):           # 4 tables x 125 dofs x npts >= 2^31
        big = torch.empty((1, 2 ** 31 // 500 + 1, 3), dtype=torch.float64, device="cuda")
        T(Q(3, 4), 1, big, np.zeros((1, 8, 3)))
    with pytest.raises(ValueError, match="three contiguous"):
        cell_geometry_batch(el.get_reference_element(), pts, corners, out=(torch.empty(3, 9, 2, device="cuda", dtype=torch.float64),) * 3)


class _Mapped(_DoublePiola):
    def mapping(self):
        return ["covariant piola"] * self._el.space_dimension()


def _singular_cell_gives_non_finite_entries_at_that_point_only():
    """A cell collapsed at one vertex: det J = 0 there.  Nothing inspects the cells; the other points are served."""
    import torch
    from fiat_amd import cellmap
    el = Q(2, 1)
    corners = R.unit_corners(2)[None].copy()
    corners[0, 1] = corners[0, 0]                                        # the edge X_0 = 0 collapses
    pts = np.array([[[0.0, 0.5], [0.5, 0.5], [1.0, 0.25]]])
    out = cellmap.tabulate_on_cells(el, 1, pts, corners)
    assert not bool(torch.isfinite(out[0, 1:, :, 0]).all()) and bool(torch.isfinite(out[0, :, :, 1:]).all())
    assert bool(torch.isfinite(out[0, 0]).all())


def _cube_families_still_refuse_verts():
    """Existing behaviour: tabulate_batch(verts=) of the cube families keeps raising."""
    pts = np.zeros((1, 4, 2))
    with pytest.raises(NotImplementedError, match="no per-request cells"):
        family("s2").tabulate_batch(1, pts, verts=np.zeros((1, 4, 2)))
    with pytest.raises(NotImplementedError, match="no per-request cells"):
        family("dpc2").tabulate_batch(1, pts, verts=np.zeros((1, 4, 2)))
    with pytest.raises(TypeError):
        Q(2, 2).tabulate_batch(1, pts, verts=np.zeros((1, 4, 2)))


def test_cells_are_not_inspected_and_verts_stay_refused():
    _singular_cell_gives_non_finite_entries_at_that_point_only()
    _cube_families_still_refuse_verts()
