"""Derivative orders 7 and 8 on the device (csrc/api.hip ensure_high_order + mix_any_order, csrc/table_kernels.hpp
table_mix_any_kernel), against tests/golden/high_order.npz (the unmodified reference), the oracle (pinned at these orders by
tests/test_high_order_host.py) and the chain-rule reference of tests/high_order_reference.py.

Three parts of the route run only at these orders: table_mix_any_kernel with cnt == CMAX tables of one order (9 in 2-D, 45 in
3-D) and first[] / cnt[] / moff[] past index 6; the internal element of ensure_high_order with ntab x rows rows (1 260 for P6
triangles, 13 860 for DG6 tetrahedra, 27 225 for a degree-8 tetrahedron set) through plan_launch; differentiation-matrix products
of depth 7 and 8 with the structural-zero rule.  Standing tolerances throughout, per order and per request: 1e-12 values, 1e-10
derivatives, as max|x - ref| / max(1, max|ref| over the tables of that order)."""
import os
import re
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import edge_reference as R  # noqa: E402
import high_order_reference as H  # noqa: E402

ORDER = H.MAX_ORDER

# fixture cases (tests/golden/high_order.npz) and the degree-6 / 7 cases of round4.npz
MAKE = {"on10int": lambda fa, c: fa.ONPolynomialSet(c, 10), "p8tri": lambda fa, c: fa.Lagrange(c, 8),
        "rt8tri": lambda fa, c: fa.RaviartThomas(c, 8), "on8tet": lambda fa, c: fa.ONPolynomialSet(c, 8),
        "dg6tet": lambda fa, c: fa.DiscontinuousLagrange(c, 6), "p6tri": lambda fa, c: fa.Lagrange(c, 6),
        "on7int": lambda fa, c: fa.ONPolynomialSet(c, 7), "on8tri": lambda fa, c: fa.ONPolynomialSet(c, 8)}
SD = {"on10int": 1, "p8tri": 2, "rt8tri": 2, "on8tet": 3, "dg6tet": 3, "p6tri": 2, "on7int": 1, "on8tri": 2}
_ELS, _TAKEN, _MIX_REF, _SWEEP_REF, _SWEEP = {}, {}, {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _release_module_caches():
    """Elements, internal elements and reference tables are shared by the tests of this module and dropped after the last one."""
    yield
    for cache in (_ELS, _TAKEN, _MIX_REF, _SWEEP_REF, _SWEEP):
        cache.clear()


def element(name):
    import fiat_amd as fa
    if name not in _ELS:
        _ELS[name] = MAKE[name](fa, fa.ufc_simplex(SD[name]))
    return _ELS[name]


def is_element(base):
    return hasattr(base, "dual_basis")


def device(base):
    return base if is_element(base) else base.device_polyset()


def describe(base):
    """(degree, coefficients, scale, variant) of a facade element or polynomial set: what the oracle tabulates."""
    ps = base.get_nodal_basis() if is_element(base) else base
    n = ps.get_embedded_degree()
    es = ps.get_expansion_set()
    return n, np.asarray(ps.get_coeffs(), dtype=float), es.get_scale(n), es.variant


def single_call(base, order, pts, sd):
    tab = base.tabulate(order, pts) if is_element(base) else base.tabulate(pts, order)
    keys = H.jet(sd, order)
    assert list(tab) == keys
    return np.stack([tab[a] for a in keys])


def show(tag, errs):
    print(f"{tag}: worst {max(errs):.2e}  per order " + " ".join(f"{e:.1e}" for e in errs))


def requests(sd, nreq, npts, seed):
    """(reference points, physical points, cells): cells as in the fixtures, every third one negatively oriented."""
    rng = np.random.default_rng(seed)
    e = rng.exponential(size=(nreq, npts, sd + 1))
    bary = e / e.sum(-1, keepdims=True)
    ref = H.ufc_simplex(sd)
    A = np.eye(sd) + 0.2 * rng.standard_normal((nreq, sd, sd))
    A[::3, :, 0] *= -1.0
    assert np.abs(np.linalg.det(A)).min() > 0.2            # inputs: no nearly degenerate cell
    verts = np.einsum("vd,red->rve", ref, A) + rng.standard_normal((nreq, 1, sd))
    return np.einsum("rpv,vd->rpd", bary, ref), np.einsum("rpv,rvd->rpd", bary, verts), verts


def mix_kernel_ran(names, sd):
    return any(f"table_mix_any_kernel<{sd}>" in n for n in names)


# ---- the fixture: own cell and per-request cells ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(H.CASES))
@pytest.mark.parametrize("order", [7, 8])
def test_own_cell_against_the_reference(golden, name, order):
    """tabulate_batch(order, reference points) and, for the first request, tabulate(order, .) equal the reference's tables.  Order 7
    is a call of its own: it builds its own internal element."""
    g = golden("high_order")
    sd = SD[name]
    base = element(name)
    ref_pts = g[f"ho_{name}_refpts"]
    got = device(base).tabulate_batch(order, ref_pts).cpu().numpy()
    for r in range(ref_pts.shape[0]):
        want = H.truncate(g[f"ho_{name}_o8_ref{r}"], sd, order)
        show(f"{name} order {order} own cell, request {r}", H.assert_close(got[r], want, sd, order, (name, r)))
    want = H.truncate(g[f"ho_{name}_o8_ref0"], sd, order)
    show(f"{name} order {order} own cell, tabulate()", H.assert_close(single_call(base, order, ref_pts[0], sd), want, sd, order, name))


@pytest.mark.parametrize("name", list(H.CASES))
@pytest.mark.parametrize("order", [7, 8])
def test_cells_against_the_reference(golden, name, order):
    """Per-request cells (the second one negatively oriented): the chain-rule reference applied to the reference's reference-cell
    tables, and for the P8 triangle also the reference's element built ON the physical cell."""
    g = golden("high_order")
    sd = SD[name]
    base = element(name)
    verts, pts = g[f"ho_{name}_verts"], g[f"ho_{name}_pts"]
    names = R.launched(lambda: device(base).tabulate_batch(order, pts, verts=verts))
    assert mix_kernel_ran(names, sd), sorted(names)
    got = device(base).tabulate_batch(order, pts, verts=verts).cpu().numpy()
    for r in range(verts.shape[0]):
        want = H.chain_rule_tables(H.truncate(g[f"ho_{name}_o8_ref{r}"], sd, order), sd, order, verts[r])
        show(f"{name} order {order} cells, request {r}, chain rule", H.assert_close(got[r], want, sd, order, (name, r, "chain rule")))
        if H.CASES[name][2]:
            want = H.truncate(g[f"ho_{name}_o8_phys{r}"], sd, order)
            show(f"{name} order {order} cells, request {r}, element on the physical cell",
                 H.assert_close(got[r], want, sd, order, (name, r, "physical cell")))


# ---- above the degree ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,degree,rebuild", [("dg6tet", 6, True), ("p6tri", 6, True), ("on7int", 7, False)])
@pytest.mark.parametrize("order", [7, 8])
def test_above_the_degree(golden, name, degree, rebuild, order):
    """Cases of round4.npz at orders 7 and 8: the tables of orders <= 6 equal the fixture; every table of an order above the degree
    is EXACTLY 0.0 on the own cell (the structural zeros of the differentiation matrices) and within the standing
    tolerance of zero with cells.  (Degree 7 on the interval: its order-7 tables do not vanish -- they are compared with the
    oracle and must be constant over the points.)"""
    g = golden("round4")
    sd = SD[name]
    base = element(name)
    verts, pts, ref_pts = g[f"ho_{name}_verts"], g[f"ho_{name}_pts"], g[f"ho_{name}_refpts"]
    n, coeffs, scale, variant = describe(base)
    assert n == degree
    f = H.firsts(sd, order)
    own = device(base).tabulate_batch(order, ref_pts).cpu().numpy()
    cells = device(base).tabulate_batch(order, pts, verts=verts).cpu().numpy()
    for r in range(verts.shape[0]):
        low = g[f"ho_{name}_o6_ref{r}"]
        show(f"{name} order {order} own cell, request {r}, orders <= 6", H.assert_close(own[r][:f[7]].reshape(low.shape), low, sd, 6, (name, r)))
        if rebuild:
            low_x = g[f"ho_{name}_o6_phys{r}"]
        else:
            low_x = H.chain_rule_tables(low, sd, 6, verts[r])
        show(f"{name} order {order} cells, request {r}, orders <= 6", H.assert_close(cells[r][:f[7]].reshape(low.shape), low_x, sd, 6, (name, r, "cells")))
        for k in range(7, order + 1):
            o, c = own[r][f[k]:f[k + 1]], cells[r][f[k]:f[k + 1]]
            if k > degree:
                assert np.count_nonzero(o) == 0, (name, r, k, np.abs(o).max())
                assert np.abs(c).max() <= H.TOL_DER, (name, r, k, np.abs(c).max())
            else:
                want = H.oracle_tables(sd, n, coeffs, k, ref_pts[r], scale, variant)[f[k]:f[k + 1]]
                assert np.abs(o - want.reshape(o.shape)).max() <= H.TOL_DER * max(1.0, np.abs(want).max())
                assert np.abs(o - o[..., :1]).max() <= H.TOL_DER * max(1.0, np.abs(want).max())
                want_x = H.chain_rule_tables(np.concatenate([np.zeros((f[k],) + want.shape[1:]), want]), sd, k, verts[r])[f[k]:f[k + 1]]
                assert np.abs(c - want_x.reshape(c.shape)).max() <= H.TOL_DER * max(1.0, np.abs(want_x).max())


# ---- edges of table_mix_any_kernel -----------------------------------------------------------------------------------------
# n = rows x npts positions of a request: one workgroup of 256 threads per (request, slice), slices = min(16, ceil(n / 1024)).
# (rows, npts) with the LAST rows of the degree-8 ON set (the highest degrees: their order-8 tables do not vanish): n = 1, 255, 256,
# 257, 1024 | 1025 (one slice | two), 2049 (three) and, past 15 360 (16 slices), 15 375 = 15 360 + 15.  257 and 2049 = 3 x 683 need
# hundreds of points: on tetrahedra their reference is tabulated for the taken rows, request by request (MIX_POOL: the whole set's
# tables at 2 049 points would be 450 MB).
MIX_EDGES = {2: [(1, 1), (15, 17), (16, 16), (1, 257), (32, 32), (25, 41), (3, 683), (41, 375)],
             3: [(1, 1), (15, 17), (16, 16), (1, 257), (32, 32), (25, 41), (3, 683), (125, 123)]}
MIX_EDGES_ORDER_7 = {2: MIX_EDGES[2], 3: [(15, 17), (1, 257), (32, 32), (25, 41), (125, 123)]}
MIX_POOL = {1: 100, 2: 683, 3: 123}          # points a request of the shared pool
MIX_SET = {1: "on10int", 2: "on8tri", 3: "on8tet"}


def mix_reference(sd, order):
    """Oracle tables of the whole ON set at a pool of 3 requests x the largest point count, cells and their chain-rule matrices:
    computed once, sliced by every shape."""
    if (sd, order) not in _MIX_REF:
        maxpts = MIX_POOL[sd]
        ref_pts, pts, verts = requests(sd, 3, maxpts, 80 + sd)
        n, coeffs, scale, variant = describe(element(MIX_SET[sd]))
        tab = H.oracle_tables(sd, n, coeffs, order, ref_pts.reshape(-1, sd), scale, variant)
        tab = tab.reshape(tab.shape[:2] + (3, maxpts))
        Ms = [H.chain_rule_matrices(sd, order, H.cell_jacobian_inverse(v)) for v in verts]
        _MIX_REF[(sd, order)] = (pts, verts, tab, Ms)
    return _MIX_REF[(sd, order)]


def mix_reference_of_rows(sd, order, rows, npts):
    """The same for one shape of more points than the pool holds: the oracle with the coefficient rows of the taken members, one
    request at a time."""
    key = (sd, order, rows, npts)
    if key not in _MIX_REF:
        ref_pts, pts, verts = requests(sd, 3, npts, 90 + sd)
        n, coeffs, scale, variant = describe(element(MIX_SET[sd]))
        tab = np.stack([H.oracle_tables(sd, n, coeffs[len(coeffs) - rows:], order, x, scale, variant) for x in ref_pts], axis=2)
        Ms = [H.chain_rule_matrices(sd, order, H.cell_jacobian_inverse(v)) for v in verts]
        _MIX_REF[key] = (pts, verts, tab, Ms)
    return _MIX_REF[key]


def run_mix_edge(sd, order, rows, npts, nreq):
    full = element(MIX_SET[sd])
    N = full.get_num_members()
    if npts <= MIX_POOL[sd]:
        pts, verts, tab, Ms = mix_reference(sd, order)
        tab = tab[:, N - rows:]
    else:
        pts, verts, tab, Ms = mix_reference_of_rows(sd, order, rows, npts)
    if (sd, rows) not in _TAKEN:
        _TAKEN[(sd, rows)] = full.take(list(range(N - rows, N))).device_polyset()
    ps = _TAKEN[(sd, rows)]
    p, v = np.ascontiguousarray(pts[:nreq, :npts]), verts[:nreq]
    names = R.launched(lambda: ps.tabulate_batch(order, p, verts=v))
    assert mix_kernel_ran(names, sd), sorted(names)
    got = ps.tabulate_batch(order, p, verts=v).cpu().numpy()
    worst = [0.0] * (order + 1)
    for r in range(nreq):
        want = H.chain_rule_apply(Ms[r], tab[:, :, r, :npts], sd, order)
        worst = np.maximum(worst, H.assert_close(got[r], want, sd, order, (sd, order, rows, npts, nreq, r)))
    return list(worst)


@pytest.mark.parametrize("sd,order", [(2, 8), (3, 8), (2, 7), (3, 7)])
@pytest.mark.parametrize("nreq", [1, 3])
def test_table_mix_any_kernel_edges(sd, order, nreq):
    shapes = MIX_EDGES[sd] if order == 8 else MIX_EDGES_ORDER_7[sd]
    for rows, npts in shapes:
        errs = run_mix_edge(sd, order, rows, npts, nreq)
        show(f"mix edge sd {sd} order {order} n = {rows} x {npts} = {rows * npts}, {nreq} request(s)", errs)


@pytest.mark.parametrize("npts", [1, 5, 100])
@pytest.mark.parametrize("nreq", [1, 3])
def test_table_mix_any_kernel_on_the_interval(npts, nreq):
    """sd = 1 at order 8 with n = 11 x npts (1 100: two slices)."""
    show(f"mix edge sd 1 order 8 n = 11 x {npts}, {nreq} request(s)", run_mix_edge(1, 8, 11, npts, nreq))


# ---- the internal element across the planner ---------------------------------------------------------------------------------
SWEEP_NPTS = [1, 5, 16, 17, 48, 49, 64, 65, 129]
SWEEP_ELEMENTS = ["p8tri", "on8tet", "dg6tet"]


def sweep_reference(name, nreq=3, npts=129):
    key = (name, nreq, npts)
    if key not in _SWEEP_REF:
        sd = SD[name]
        ref_pts, pts, verts = requests(sd, nreq, npts, 800 + sd + nreq)
        n, coeffs, scale, variant = describe(element(name))
        tab = H.oracle_tables(sd, n, coeffs, ORDER, ref_pts.reshape(-1, sd), scale, variant)
        tab = tab.reshape(tab.shape[:2] + (nreq, npts))
        Ms = [H.chain_rule_matrices(sd, ORDER, H.cell_jacobian_inverse(v)) for v in verts]
        _SWEEP_REF[key] = (ref_pts, pts, verts, tab, Ms)
    return _SWEEP_REF[key]


def families(names):
    """Kernel families of a launch without the table-mixing pass: "tabulate_simplex_stacked", ..."""
    out = set()
    for n in names:
        m = re.search(r"fxk::(\w+)", n)
        if m and not m.group(1).startswith("table_mix"):
            out.add(m.group(1))
    return out


def run_shape(name, cells, npts, nreq, ref):
    """One order-8 call: (kernel names, worst error per order over the requests, first failure or None)."""
    sd = SD[name]
    ref_pts, pts, verts, tab, Ms = ref
    dev = device(element(name))
    p = np.ascontiguousarray((pts if cells else ref_pts)[:nreq, :npts])
    v = verts[:nreq] if cells else None
    names = R.launched(lambda: dev.tabulate_batch(ORDER, p, verts=v))
    got = dev.tabulate_batch(ORDER, p, verts=v).cpu().numpy()
    worst, failure = np.zeros(ORDER + 1), None
    for r in range(nreq):
        want = tab[:, :, r, :npts]
        if cells:
            want = H.chain_rule_apply(Ms[r], want, sd, ORDER)
        errs = H.order_errors(got[r].reshape(want.shape), want, sd, ORDER)
        worst = np.maximum(worst, errs)
        bad = [k for k, e in enumerate(errs) if not e <= (H.TOL_VAL if k == 0 else H.TOL_DER)]
        if bad and failure is None:
            failure = (name, "cells" if cells else "own cell", npts, nreq, "request", r, "orders", bad, errs)
    return sorted(names), list(worst), failure


def sweep(name, cells):
    if (name, cells) not in _SWEEP:
        ref = sweep_reference(name)
        rows = []
        for npts in SWEEP_NPTS:
            for nreq in (1, 3):
                if name == "on8tet" and npts == 129 and nreq == 3:
                    continue            # 28 MB a request: one is enough
                rows.append((npts, nreq) + run_shape(name, cells, npts, nreq, ref))
        _SWEEP[(name, cells)] = rows
    return _SWEEP[(name, cells)]


@pytest.mark.parametrize("name", SWEEP_ELEMENTS)
@pytest.mark.parametrize("cells", [False, True], ids=["own", "cells"])
def test_internal_element_across_the_planner(name, cells):
    """Order 8 of the P8 triangle (45 x 45 = 2 025 rows), the ON degree-8 tetrahedron set (165 x 165 = 27 225) and the DG6
    tetrahedron (165 x 84 = 13 860): point counts on both sides of the planner's windows, 1 and 3 requests, every request against
    the oracle (with cells: through the chain-rule reference)."""
    rows = sweep(name, cells)
    for npts, nreq, names, worst, failure in rows:
        print(f"{name} {'cells' if cells else 'own'} npts {npts:3d} nreq {nreq}: {', '.join(sorted(families(names)))}"
              f"  worst {max(worst):.2e} (order {int(np.argmax(worst))})")
    failures = [r[4] for r in rows if r[4] is not None]
    assert not failures, failures
    if cells:
        assert all(mix_kernel_ran(r[2], SD[name]) for r in rows)


def test_internal_elements_meet_more_than_one_kernel_family():
    """the internal element runs "on whichever kernel serves the shape"."""
    seen = {}
    for name in SWEEP_ELEMENTS:
        for cells in (False, True):
            for npts, nreq, names, worst, failure in sweep(name, cells):
                for fam in families(names):
                    seen.setdefault(fam, []).append((name, "cells" if cells else "own", npts, nreq))
    for fam, shapes in sorted(seen.items()):
        print(f"{fam}: {len(shapes)} shapes, e.g. {shapes[0]}")
    assert len(seen) > 1, sorted(seen)


def test_many_requests_of_the_p8_triangle():
    ref = sweep_reference("p8tri", nreq=37, npts=17)
    for cells in (False, True):
        names, worst, failure = run_shape("p8tri", cells, 17, 37, ref)
        print(f"p8tri {'cells' if cells else 'own'} npts 17 nreq 37: {', '.join(sorted(families(names)))}  worst {max(worst):.2e}")
        assert failure is None, failure


# ---- guarded output, rebuild, refusal ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,npts,nreq,cells", [("p8tri", 17, 3, True), ("dg6tet", 5, 3, False)])
def test_guarded_output(name, npts, nreq, cells):
    """Two shapes of the sweep into an ``out`` view at 0, 1, 7 and 8 doubles past a 128-byte line inside a NaN-filled buffer: guards
    untouched, every entry written, equal to a fresh ``out`` -- and that one equal to the oracle."""
    import torch
    sd = SD[name]
    ref_pts, pts, verts, tab, Ms = sweep_reference(name)
    dev = device(element(name))
    p = np.ascontiguousarray((pts if cells else ref_pts)[:nreq, :npts])
    v = verts[:nreq] if cells else None
    shape = (nreq, H.ntables(sd, ORDER)) + tab.shape[1:2] + (npts,)
    fresh = R.compare(lambda o: dev.tabulate_batch(ORDER, p, verts=v, out=o), shape, torch.device("cuda", torch.cuda.current_device()))
    fresh = fresh.cpu().numpy()
    for r in range(nreq):
        want = tab[:, :, r, :npts]
        H.assert_close(fresh[r], H.chain_rule_apply(Ms[r], want, sd, ORDER) if cells else want, sd, ORDER, (name, r))


def test_set_coeffs_rebuilds_the_internal_element():
    """fx_element_set_coeffs invalidates the internal elements: an order-8 call after it reflects the new coefficients."""
    import fiat_amd as fa
    sd, n = 2, 8
    ps = fa.ONPolynomialSet(fa.ufc_simplex(sd), n).device_polyset()          # a set of its own: the module's elements stay as they are
    ref_pts, pts, verts = requests(sd, 3, 7, 5)
    _, coeffs, scale, variant = describe(element("on8tri"))
    rng = np.random.default_rng(88)
    for C in (coeffs, rng.standard_normal(coeffs.shape), rng.standard_normal((31, coeffs.shape[1]))):
        if C is not coeffs:
            ps.set_coeffs(C)
        own = ps.tabulate_batch(ORDER, ref_pts).cpu().numpy()
        cells = ps.tabulate_batch(ORDER, pts, verts=verts).cpu().numpy()
        for r in range(3):
            want = H.oracle_tables(sd, n, C, ORDER, ref_pts[r], scale, variant)
            show(f"set_coeffs {C.shape} own cell, request {r}", H.assert_close(own[r], want, sd, ORDER, ("own", r)))
            H.assert_close(cells[r], H.chain_rule_tables(want, sd, ORDER, verts[r]), sd, ORDER, ("cells", r))


def test_set_coeffs_with_another_ndof_drops_every_cache(kernel_policy):
    """A P2 triangle, 2 requests of 3 points on its own cell under policy stacked_small: orders 0 and 2 build the stacked matrices
    of the element, order 3 its internal element.  fx_element_set_coeffs with 4 rows in place of 6 replaces the coefficient
    buffers and drops all of those; the same orders afterwards are the new matrix times the tables of a fresh
    identity-coefficient element of the same expansion set."""
    import fiat_amd as fa
    sd, n, orders = 2, 2, (0, 2, 3)
    kernel_policy("stacked_small")
    ps = fa.Lagrange(fa.ufc_simplex(sd), n).get_nodal_basis()
    es, C6 = ps.get_expansion_set(), np.asarray(ps.get_coeffs(), dtype=float)
    ref_pts, _, _ = requests(sd, 2, 3, 11)
    raw = es.device_polyset(n)                                               # identity coefficients: the expansion set itself
    phi = {k: raw.tabulate_batch(k, ref_pts).cpu().numpy() for k in orders}  # (nreq, ntab, nexp, npts)
    dev = es.device_polyset(n, coeffs=C6)
    C4 = np.random.default_rng(89).standard_normal((4, C6.shape[1]))
    for C in (C6, C4):
        if C is not C6:
            dev.set_coeffs(C)
        for k in orders:
            got = dev.tabulate_batch(k, ref_pts).cpu().numpy()
            assert got.shape == (2, H.ntables(sd, k), C.shape[0], 3)
            for r in range(2):
                want = np.einsum("ij,tjp->tip", C, phi[k][r])
                show(f"set_coeffs {C.shape} order {k}, request {r}", H.assert_close(got[r], want, sd, k, (C.shape, k, r)))


@pytest.mark.parametrize("name", ["rt8tri", "on10int"])
def test_order_9_is_refused(golden, name):
    g = golden("high_order")
    dev = device(element(name))
    with pytest.raises(NotImplementedError):
        dev.tabulate_batch(9, g[f"ho_{name}_refpts"])
    with pytest.raises(NotImplementedError):
        dev.tabulate_batch(9, g[f"ho_{name}_pts"], verts=g[f"ho_{name}_verts"])
    if is_element(element(name)):
        with pytest.raises(NotImplementedError):
            element(name).tabulate(9, g[f"ho_{name}_refpts"][0])
