"""One request per manifest case (tests/instance_manifest.py): ``prepare(case)`` builds the seeded inputs, the device call and
a plain reference of the same operation.  Shared by tests/test_gpu_instances.py (launch set + tables) and
tools/instance_search.py (which only launches).  References: the pinned C oracle for simplex tabulation (on the physical cells
where cells are given), its affine tables pushed forward here in float64 for the Piola maps, tests/edge_reference.py for
Bernstein, H(div) / H(curl) and 1-D Lagrange factors (long double), NumPy products of factor tables for tensor / prism
elements, the Python oracle for macro elements, the NumPy statement of the operation for the auxiliary kernels."""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE, os.path.join(HERE, "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import edge_reference as R  # noqa: E402

TOL_VAL, TOL_DER = 1e-12, 1e-10          # value tables / derivative tables, relative to max(1, max |ref|) of the table

MACRO = {"cg2_alfeld_tri": ("Lagrange", 2, 2, "equispaced,alfeld"), "cg1_iso_tri": ("Lagrange", 2, 1, "equispaced,iso"),
         "cg2_iso_tri": ("Lagrange", 2, 2, "equispaced,iso"), "cg3_alfeld_tri": ("Lagrange", 2, 3, "equispaced,alfeld"),
         "cg1_iso_tet": ("Lagrange", 3, 1, "equispaced,iso"), "cg2_alfeld_tet": ("Lagrange", 3, 2, "equispaced,alfeld"),
         "cg3_alfeld_tet": ("Lagrange", 3, 3, "equispaced,alfeld"),
         "dg1_alfeld_tet": ("DiscontinuousLagrange", 3, 1, "equispaced_interior,alfeld"),
         "cg1_iso_int": ("Lagrange", 1, 1, "equispaced,iso"), "cg2_iso_int": ("Lagrange", 1, 2, "equispaced,iso")}

_elements = {}
_mappings = {}          # polynomial sets that are not elements: the map of the element they come from


def element(family, sd, degree):
    """The element (or, family "ONPolynomialSet", the raw expansion set) -- built once: construction solves a Vandermonde."""
    import fiat_amd as fa
    key = (family, sd, degree)
    if key not in _elements:
        cell = fa.ufc_simplex(sd)
        if family == "ONPolynomialSet":
            _elements[key] = fa.ONPolynomialSet(cell, degree)
        elif family == "VectorON":      # vector-valued copies of the expansion set (no library family has degree 0 / few rows)
            _elements[key] = fa.ONPolynomialSet(cell, degree, shape=(sd,))
            _mappings[id(_elements[key])] = "contravariant piola"
        elif family.startswith("Random/"):
            # k members with seeded random coefficients over the expansion set (more members than the set has are fine for
            # tabulation): row counts -- row-tile classes, parities -- that no family of this degree has
            k = int(family.split("/")[1])
            es = fa.ExpansionSet(cell)
            nexp = es.get_num_members(degree)
            coeffs = np.random.default_rng(1000 * sd + 10 * degree + k).standard_normal((k, nexp)) / np.sqrt(nexp)
            _elements[key] = fa.PolynomialSet(cell, degree, degree, es, coeffs)
        elif family.endswith("-1") or "/" in family:
            # the nodal basis without its last member (the other parity of the table size), or its first k members (a
            # sub-space with few rows): PolynomialSet.take, pushed forward like the whole element
            base = element(family[:-2] if family.endswith("-1") else family.split("/")[0], sd, degree)
            basis = polyset(base)
            k = len(basis) - 1 if family.endswith("-1") else int(family.split("/")[1])
            if not 0 < k < len(basis):
                raise ValueError(f"{family}: the basis has {len(basis)} members")
            _elements[key] = basis.take(list(range(k)))
            _mappings[id(_elements[key])] = mapping_of(base)
        elif family in MACRO:
            fam, msd, deg, variant = MACRO[family]
            _elements[key] = getattr(fa, fam)(fa.ufc_simplex(msd), deg, variant)
        else:
            _elements[key] = getattr(fa, family)(cell, degree)
    return _elements[key]


def polyset(el):
    return el.get_nodal_basis() if hasattr(el, "get_nodal_basis") else el


def mapping_of(el):
    return el.mapping()[0] if hasattr(el, "mapping") else _mappings.get(id(el), "affine")


def simplex_batch(rng, sd, nreq, npts, cells, shared=False):
    """(pts, verts): points inside the cells; cells of both orientations (every third one mirrored)."""
    from oracle import fiat_oracle as fo
    e = rng.exponential(size=((1,) if shared else (nreq,)) + (npts, sd + 1))
    bary = e / e.sum(-1, keepdims=True)
    if not cells:
        return bary[..., 1:].copy(), None, bary
    A = np.eye(sd) + 0.15 * rng.standard_normal((nreq, sd, sd))
    A[::3, :, 0] *= -1.0
    verts = np.einsum("vd,red->rve", fo.UFC_SIMPLEX[sd], A) + rng.standard_normal((nreq, 1, sd))
    pts = np.einsum("rpv,rvd->rpd", np.broadcast_to(bary, (nreq, npts, sd + 1)), verts)
    return pts, verts, bary


def oracle_tables(el, order, pts, verts):
    """(nreq, ntab, ndof, [vdim,] npts) from the C oracle: the recurrence ON the cells ``verts`` (derivatives physical)."""
    from oracle import c_oracle
    from oracle import fiat_oracle as fo
    ps = polyset(el)
    sd = pts.shape[-1]
    n = ps.get_embedded_degree()
    es = ps.get_expansion_set()
    coeffs = ps.get_coeffs()
    tab = c_oracle.tabulate_batch(fo.UFC_SIMPLEX[sd], n, coeffs, order, pts, verts=verts, scale=es.get_scale(n),
                                  variant=getattr(es, "variant", None))
    return tab.reshape((pts.shape[0], tab.shape[1]) + tuple(coeffs.shape[:-1]) + (pts.shape[1],))


def push_forward(tab, verts, mapping):
    """Piola maps of vector-valued tables (nreq, ntab, ndof, sd, npts) in float64: J = dx/dX between the UFC simplex and the
    request's cell, covariant J^-T Phi, contravariant J Phi / det J (derivative tables map the same way: J is constant)."""
    if mapping == "affine":
        return tab
    sd = verts.shape[-1]
    ref = R.ufc_simplex(sd)
    E0 = (ref[1:] - ref[0]).T
    out = np.empty_like(tab)
    for r in range(tab.shape[0]):
        J = (verts[r][1:] - verts[r][0]).T @ np.linalg.inv(E0)
        if mapping == "covariant piola":
            M = np.linalg.inv(J).T
        elif mapping == "contravariant piola":
            M = J / np.linalg.det(J)
        else:
            raise ValueError(mapping)
        out[r] = np.einsum("cd,tkdp->tkcp", M, tab[r])
    return out


class Prepared:
    """run(out=None) -> device tensor; shape of out (None: the call owns its output); reference() -> ndarray shaped like the
    output; table_axis: axis of the derivative tables (1) or None (one tolerance: TOL_VAL, or ``tol``)."""

    def __init__(self, run, shape, reference, table_axis=1, tol=None):
        self.run, self.shape, self.reference, self.table_axis, self.tol = run, shape, reference, table_axis, tol


def _device():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def D(x):
    """Input staged on the device before the call: run() itself launches nothing but the library's kernels."""
    import torch
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64)).to(_device())


def _simplex(case, rng):
    el = element(case["family"], case["sd"], case["degree"])
    dev = polyset(el).device_polyset()
    sd, order, npts, nreq = case["sd"], case["order"], case["npts"], case["nreq"]
    entry = case["entry"]
    cells = case.get("cells", False) or entry != "tabulate_batch"
    mapping = mapping_of(el) if entry in ("tabulate_batch_mapped", "tabulate_cells") else "affine"
    pts, verts, bary = simplex_batch(rng, sd, nreq, npts, cells, shared=entry == "tabulate_cells")
    dpts, dverts = D(pts), D(verts)
    if entry == "tabulate_cells":
        ref_pts = D(bary[0] @ R.ufc_simplex(sd))
        run = lambda out=None: dev.tabulate_batch_shared(order, ref_pts, dverts, mapping=mapping, out=out)     # noqa: E731
    else:
        run = lambda out=None: dev.tabulate_batch(order, dpts, verts=dverts, out=out,                           # noqa: E731
                                                  mapping=None if mapping == "affine" else mapping)
    reference = lambda: push_forward(oracle_tables(el, order, pts, verts), verts, mapping)                       # noqa: E731
    return Prepared(run, dev.out_shape(order, nreq, npts), reference)


def _macro(case, rng):
    from oracle import fiat_oracle as fo
    el = element(case["family"], case["sd"], case["degree"])
    S = el.get_reference_complex()
    sd, order, npts, nreq = case["sd"], case["order"], case["npts"], case["nreq"]
    es = el.get_nodal_basis().get_expansion_set()
    n = el.degree()
    pts, verts, bary = simplex_batch(rng, sd, nreq, npts, case.get("cells", False))
    dev = el.device_polyset()
    dpts, dverts = D(pts), D(verts)
    run = lambda out=None: dev.tabulate_batch(order, dpts, verts=dverts, out=out)        # noqa: E731

    def reference():
        Vs, top = np.array(S.get_vertices()), S.get_topology()
        vb = np.concatenate([1.0 - Vs.sum(-1, keepdims=True), Vs], axis=-1)
        cmap, coeffs = es.get_cell_node_map(n), el.get_coeffs()
        parent = np.array(S.get_parent().get_vertices())
        out = []
        for r in range(nreq):
            pv = vb @ (parent if verts is None else verts[r])
            cells = [pv[list(top[sd][c])] for c in sorted(top[sd])]
            ref = fo.macro_element_tabulate(parent if verts is None else verts[r], cells, cmap, n, coeffs, order, pts[r],
                                            es.scale, es.variant)
            out.append(np.stack([ref[a] for a in fo.jet_indices(sd, order)]))
        return np.stack(out)
    return Prepared(run, dev.out_shape(order, nreq, npts), reference)


def _nodes(nn, rng):
    """nn distinct nodes of [0, 1]: equispaced, jittered inside (not symmetric: a mirrored basis would be caught)."""
    if nn == 1:
        return np.array([0.5])
    x = np.linspace(0.0, 1.0, nn)
    x[1:-1] += rng.uniform(-0.2, 0.2, size=nn - 2) / (nn - 1)
    return x


def _tensor(case, rng):
    from fiat_amd import runtime
    nf, nns, order, npts, nreq = case["nf"], case["nn"], case["order"], case["npts"], case["nreq"]
    nns = [nns] * nf if isinstance(nns, int) else list(nns)
    nodes = [_nodes(nn, rng) for nn in nns]
    L = [runtime.LineLagrange(x) for x in nodes]
    grid = case["entry"] == "tensor_grid"
    if grid:
        q = case["q"]
        g = rng.uniform(0.0, 1.0, size=(nreq, nf, q))
        pts = R.grid_points(g)
        inp = D(g)
    else:
        pts = rng.uniform(0.0, 1.0, size=(nreq, npts, nf))
        inp = D(pts)
    npts = pts.shape[1]
    shape = (nreq, R.ntables(nf, order), int(np.prod(nns)), npts)
    run = lambda out=None: runtime.tensor_tabulate_batch(L, order, inp, out=out, grid=grid)       # noqa: E731

    def reference():
        flat = pts.reshape(-1, nf)
        T = [R.line_lagrange_reference(nodes[f], flat[:, f], order) for f in range(nf)]
        out = []
        for a in R.jet(nf, order):
            prod = T[0][a[0]]
            for f in range(1, nf):
                prod = (prod[:, None, :] * T[f][a[f]][None, :, :]).reshape(-1, flat.shape[0])
            out.append(prod)
        out = np.stack(out).reshape(len(out), -1, nreq, npts)
        return np.moveaxis(out, 2, 0).astype(float)
    return Prepared(run, shape, reference)


def _line(case, rng):
    from fiat_amd import runtime
    nn, order, npts, nreq = case["nn"], case["order"], case["npts"], case["nreq"]
    nodes = _nodes(nn, rng)
    L = runtime.LineLagrange(nodes)
    pts = rng.uniform(0.0, 1.0, size=(nreq, npts))
    dpts = D(pts)
    run = lambda out=None: L.tabulate_batch(order, dpts, out=out)        # noqa: E731
    reference = lambda: np.moveaxis(R.line_lagrange_reference(nodes, pts.reshape(-1), order).reshape(order + 1, nn, nreq, npts), 2, 0).astype(float)   # noqa: E731
    return Prepared(run, (nreq, order + 1, nn, npts), reference)


def _prism(case, rng):
    from fiat_amd import runtime
    el = element(case["family"], 2, case["degree"])
    tri = polyset(el).device_polyset()
    nn, order, npts, nreq = case["nn"], case["order"], case["npts"], case["nreq"]
    nodes = _nodes(nn, rng)
    line = runtime.LineLagrange(nodes)
    xy, _, _ = simplex_batch(rng, 2, nreq, npts, False)
    pts = np.concatenate([xy, rng.uniform(0.0, 1.0, size=(nreq, npts, 1))], -1)
    shapeA = tri.out_shape(order, nreq, npts)
    shape = (nreq, R.ntables(3, order), shapeA[2] * nn) + tuple(shapeA[3:])
    dpts = D(pts)

    def run(out=None):
        res = runtime.prism_tabulate_batch(tri, line, order, dpts, out=out)
        assert res is not None, "no fused prism instance for this shape"
        return res

    def reference():
        A = oracle_tables(el, order, np.ascontiguousarray(pts[..., :2]), None)         # (nreq, ntabA, ndofA, [vdim,] npts)
        B = np.moveaxis(R.line_lagrange_reference(nodes, pts[..., 2].reshape(-1), order).reshape(order + 1, nn, nreq, npts), 2, 0).astype(float)
        posA = {a: i for i, a in enumerate(R.jet(2, order))}
        out = np.empty(shape)
        for t, a in enumerate(R.jet(3, order)):
            ta, tb = A[:, posA[a[:2]]], B[:, a[2]]                                    # (nreq, ndofA, [vdim,] npts), (nreq, nn, npts)
            tb = tb.reshape((nreq, 1, nn) + (1,) * (ta.ndim - 3) + (npts,))
            out[:, t] = (ta[:, :, None] * tb).reshape((nreq, -1) + ta.shape[2:])
        return out
    return Prepared(run, shape, reference)


def _bernstein(case, rng):
    from fiat_amd import Bernstein, ufc_simplex
    sd, n, order, npts, nreq, mode = case["sd"], case["degree"], case["order"], case["npts"], case["nreq"], case["mode"]
    el = Bernstein(ufc_simplex(sd), n)
    shape = el.out_shape(order, nreq, npts)
    if mode == "own":
        pts = R.simplex_points(rng, (nreq, npts), sd)
        dpts = D(pts)
        run = lambda out=None: el.tabulate_batch(order, dpts, out=out)                                   # noqa: E731
        reference = lambda: np.asarray(R.bernstein_reference(sd, n, order, pts), dtype=float)            # noqa: E731
    else:
        pts, verts, bary = simplex_batch(rng, sd, nreq, npts, True, shared=mode == "shared")
        dpts, dverts = D(pts), D(verts)
        if mode == "cells":
            run = lambda out=None: el.tabulate_batch(order, dpts, verts=dverts, out=out)                 # noqa: E731
            reference = lambda: np.asarray(R.bernstein_reference(sd, n, order, pts, verts=verts), dtype=float)   # noqa: E731
        else:
            ref_pts = bary[0] @ R.ufc_simplex(sd)
            dref = D(ref_pts)
            run = lambda out=None: el.tabulate_cells(order, dref, dverts, out=out)                       # noqa: E731
            reference = lambda: np.asarray(R.bernstein_reference(sd, n, order, ref_pts, verts=verts, shared=True), dtype=float)   # noqa: E731
    return Prepared(run, shape, reference)


def _hdivcurl(case, rng):
    import torch
    import fiat_amd
    import make_golden_hdivcurl as M
    from fiat_amd import hdivcurl
    el = M.build(fiat_amd, case["name"])
    sd = el.get_reference_element().get_spatial_dimension()
    order, npts, nreq, grid = case["order"], case["npts"], case["nreq"], case["entry"] == "hdivcurl_grid"
    if grid:
        g = rng.uniform(-0.1, 1.1, size=(nreq, sd, case["q"]))
        pts = R.grid_points(g)
        inp = D(g)
    else:
        pts = rng.uniform(-0.1, 1.1, size=(nreq, npts, sd))
        inp = D(pts)
    _, kind, cn, dn, offsets, signs = hdivcurl.fused_descriptor(el)
    nb = R.hdc_nb(sd, len(dn), R._kind(kind)) * sum(1 for o in offsets if o >= 0)
    shape = (nreq, R.ntables(sd, order), nb, sd, pts.shape[1])
    run = lambda out=None: el.tabulate_batch(order, inp, grid=True, out=out) if grid else el.tabulate_batch(order, inp, out=out)   # noqa: E731
    reference = lambda: np.asarray(R.hdivcurl_reference(kind, cn, dn, offsets, signs, sd, order, pts), dtype=float)                # noqa: E731
    return Prepared(run, shape, reference)


def _aux(case, rng):
    """The auxiliary kernels against the NumPy statement of the operation."""
    import torch
    from fiat_amd import runtime
    from oracle import fiat_oracle as fo
    entry, a = case["entry"], case
    dev = _device()
    if entry == "classify_tables":
        x = rng.standard_normal((a["ntables"], a["rows"], a["npts"]))
        x[::2] = x[::2, :, :1]          # constant tables
        rtol = 1e-5

        def reference():
            return np.stack([np.abs(x).max((1, 2)), (np.abs(x - x[..., :1]) - rtol * np.abs(x[..., :1])).max((1, 2))], -1)
        xd = D(x)
        return Prepared(lambda out=None: runtime.classify_tables(xd, rtol=rtol), None, reference, None)
    if entry == "tables_squared_norm":
        x = rng.standard_normal((a["ntables"], a["rows"], a["vdim"], a["npts"]))
        w = rng.uniform(0.1, 1.0, size=a["npts"])
        xd, wd = D(x), D(w)
        return Prepared(lambda out=None: runtime.tables_squared_norm(xd, wd), None, lambda: np.einsum("p,trcp->tr", w, x * x), None,
                        TOL_VAL * a["npts"] * a["vdim"])     # (a sum of npts * vdim positive terms)
    if entry == "tables_point_major":
        x = rng.standard_normal((a["ntables"], a["rows"], a["npts"]))
        xd = D(x)
        return Prepared(lambda out=None: runtime.tables_point_major(xd, out=out), (a["ntables"], a["npts"], a["rows"]),
                        lambda: np.swapaxes(x, 1, 2).copy(), None, 0.0)
    if entry == "map_points":
        M, b = rng.standard_normal((a["dout"], a["din"])), rng.standard_normal(a["dout"])
        x = rng.standard_normal((a["nreq"], a["npts"], a["din"]))
        xd = D(x)
        return Prepared(lambda out=None: runtime.map_points(M, b, xd), None, lambda: x @ M.T + b, None)
    if entry == "table_outer":
        sdA, sdB, order, nreq, npts = a["sdA"], a["sdB"], a["order"], a["nreq"], a["npts"]
        va, vb = a.get("vdimA", 0), a.get("vdimB", 0)
        tA = rng.standard_normal((nreq, R.ntables(sdA, order), a["rowsA"]) + ((va,) if va else ()) + (npts,))
        tB = rng.standard_normal((nreq, R.ntables(sdB, order), a["rowsB"]) + ((vb,) if vb else ()) + (npts,))
        posA = {al: i for i, al in enumerate(R.jet(sdA, order))} if sdA else {(): 0}
        posB = {al: i for i, al in enumerate(R.jet(sdB, order))} if sdB else {(): 0}

        def reference():
            out = []
            for al in R.jet(sdA + sdB, order):
                xa, xb = tA[:, posA[al[:sdA]]], tB[:, posB[al[sdA:]]]
                xa = xa if va else xa[:, :, None]
                xb = xb if vb else xb[:, :, None]
                prod = xa[:, :, None] * xb[:, None]                       # (nreq, rowsA, rowsB, vdim, npts)
                prod = prod.reshape((nreq, a["rowsA"] * a["rowsB"]) + prod.shape[3:])
                out.append(prod if (va or vb) else prod[:, :, 0])
            return np.stack(out, 1)
        dA, dB = D(tA), D(tB)
        return Prepared(lambda out=None: runtime.table_outer(order, sdA, sdB, dA, dB, out=out), None, reference, 1, 0.0)
    if entry == "table_place":
        nreq, ntab, rows, vs, vd, npts, rd, off = a["nreq"], a["ntab"], a["rows"], a["vdim_src"], a["vdim_dst"], a["npts"], a["rows_dst"], a["row_offset"]
        src = rng.standard_normal((nreq, ntab, rows, vs, npts))
        comp = np.array([(c % (vs + 1)) - 1 for c in range(vd)])          # -1 (zero), 0, 1, ...
        sgn = np.array([1 if c % 2 == 0 else -1 for c in range(vd)])
        base = rng.standard_normal((nreq, ntab, rd, vd, npts))

        dsrc, dbase = D(src), D(base)

        def run(out=None):
            dst = torch.empty_like(dbase) if out is None else out
            dst.copy_(dbase)                                   # (a device-to-device copy, no kernel)
            return runtime.table_place(dsrc, dst, off, comp, sgn)

        def reference():
            ref = base.copy()
            for c in range(vd):
                ref[:, :, off:off + rows, c] = 0.0 if comp[c] < 0 else sgn[c] * src[:, :, :, comp[c]]
            return ref
        return Prepared(run, (nreq, ntab, rd, vd, npts), reference, None, 0.0)
    if entry == "riesz_assemble":
        w, ev = rng.standard_normal((a["nrows"], a["nq"])), rng.standard_normal((a["nexp"], a["nq"]))
        dw, dev_ = D(w), D(ev)
        return Prepared(lambda out=None: runtime.riesz_assemble(dw, dev_), None, lambda: w @ ev.T, None,
                        TOL_VAL * a["nq"])      # (a sum of nq products of O(1) numbers, measured against max(1, max |ref|))
    if entry == "vandermonde_solve":
        nsys, ndof, m = a["nsys"], a["ndof"], a["m"]
        Q = np.linalg.qr(rng.standard_normal((nsys, m, m)))[0][:, :ndof]            # orthonormal rows: V = A B^T well conditioned
        A = Q + 0.05 * rng.standard_normal((nsys, ndof, m))
        B = Q

        def reference():
            return np.stack([np.linalg.solve((A[s] @ B[s].T).T, B[s]) for s in range(nsys)])
        dA, dB = D(A), D(B)
        return Prepared(lambda out=None: runtime.vandermonde_solve_batch(dA, dB), None, reference, None,
                        1e-10)   # (a solve: condition number ~ 2 times the 1e-12 of a value table times ndof)
    if entry == "collapsed_quadrature":
        sd, m = a["sd"], a["m"]
        verts = None
        if a.get("cells"):
            verts = R.ufc_simplex(sd) @ (np.eye(sd) + 0.2 * rng.standard_normal((sd, sd))) + rng.standard_normal(sd)

        def run(out=None):
            p, w = runtime.collapsed_quadrature(sd, m, verts=verts)
            return torch.cat([p, w[:, None]], 1)

        def reference():
            # the host rule: SciPy's Gauss-Jacobi roots collapsed in NumPy (fiat_amd/quadrature.py), on the same cell
            import fiat_amd
            from fiat_amd import quadrature, reference_element
            cell = fiat_amd.ufc_simplex(sd)
            if verts is not None:
                cell = reference_element.UFCSimplex(cell.get_shape(), tuple(map(tuple, verts)), cell.get_topology())
            Q = quadrature.CollapsedQuadratureSimplexRule(cell, m)
            return np.concatenate([np.asarray(Q.get_points()), np.asarray(Q.get_weights())[:, None]], 1)
        return Prepared(run, None, reference, None)
    if entry == "jacobi":
        al, be, n, order, npts = a["a"], a["b"], a["n"], a["order"], a["npts"]
        xs = rng.uniform(-1.0, 1.0, size=npts)

        from fiat_amd import jacobi
        dx = D(xs)
        run = lambda out=None: jacobi.jacobi_table(al, be, n, dx, order=order)        # noqa: E731

        def reference():
            if order == 0:
                return np.asarray(fo.jacobi_table(al, be, n, xs), dtype=float)
            return np.asarray(fo.jacobi_deriv_table(al, be, n, xs, order), dtype=float)
        return Prepared(run, None, reference, None, TOL_DER if order else TOL_VAL)
    raise KeyError(entry)


GOLDEN_HIGH = {"round3": ("pc", {"p4tet": ("Lagrange", 3, 4, True), "dg5tet": ("DiscontinuousLagrange", 3, 5, True),
                                "p5tri": ("Lagrange", 2, 5, True), "rt3tri": ("RaviartThomas", 2, 3, False),
                                "on6int": ("ONPolynomialSet", 1, 6, False)}),
               "round4": ("ho", {"dg6tet": ("DiscontinuousLagrange", 3, 6, True), "p6tri": ("Lagrange", 2, 6, True),
                                 "p5tet": ("Lagrange", 3, 5, True), "n4tri": ("Nedelec", 2, 4, False),
                                 "on7int": ("ONPolynomialSet", 1, 7, False)})}


def _chain_rule_tables(ref_tab, sd, order, Kt):
    """d^alpha_x from tables with respect to X, Kt[c, d] = dX_c / dx_d: the sum over ordered source directions (NumPy)."""
    import itertools
    keys = R.jet(sd, order)
    pos = {a: i for i, a in enumerate(keys)}
    out = []
    for alpha in keys:
        dirs = [d for d, m in enumerate(alpha) for _ in range(m)]
        acc = 0.0
        for src in itertools.product(range(sd), repeat=len(dirs)):
            beta = tuple(src.count(c) for c in range(sd))
            acc = acc + float(np.prod([Kt[c, d] for c, d in zip(src, dirs)])) * ref_tab[pos[beta]]
        out.append(acc)
    return np.stack(out)


def _golden_high(case, rng):
    """Derivative orders 3-6 (differentiation matrices; with cells the table-mixing passes) against the recorded tables of
    the reference implementation (tests/golden/round3.npz, round4.npz): elements built ON the physical cells where the family
    is affine, else the chain rule applied in NumPy to its reference-cell tables."""
    prefix, names = GOLDEN_HIGH[case["fixture"]]
    family, sd, degree, rebuild = names[case["name"]]
    g = np.load(os.path.join(HERE, "golden", case["fixture"] + ".npz"))
    order, key = case["order"], f"{prefix}_{case['name']}"
    el = element(family, sd, degree)
    dev = polyset(el).device_polyset()
    verts = g[key + "_verts"]
    ref = R.ufc_simplex(sd)
    if case.get("cells"):
        dpts, dverts = D(g[key + "_pts"]), D(verts)
    else:
        dpts, dverts = D(g[key + "_refpts"]), None
    run = lambda out=None: dev.tabulate_batch(order, dpts, verts=dverts, out=out)        # noqa: E731

    def reference():
        out = []
        for r in range(verts.shape[0]):
            if not case.get("cells"):
                out.append(g[f"{key}_o{order}_ref{r}"])
            elif rebuild:
                out.append(g[f"{key}_o{order}_phys{r}"])
            else:
                J = (verts[r][1:] - verts[r][0]).T @ np.linalg.inv((ref[1:] - ref[0]).T)
                out.append(_chain_rule_tables(g[f"{key}_o{order}_ref{r}"], sd, order, np.linalg.inv(J)))
        return np.stack(out).reshape(dev.out_shape(order, verts.shape[0], dpts.shape[1]))
    return Prepared(run, dev.out_shape(order, verts.shape[0], dpts.shape[1]), reference)


ENTRIES = {"golden_high_order": _golden_high, "tabulate_batch": _simplex, "tabulate_batch_mapped": _simplex, "tabulate_cells": _simplex, "macro": _macro,
           "tensor": _tensor, "tensor_grid": _tensor, "line": _line, "prism": _prism, "bernstein": _bernstein,
           "hdivcurl": _hdivcurl, "hdivcurl_grid": _hdivcurl,
           "classify_tables": _aux, "tables_squared_norm": _aux, "tables_point_major": _aux, "map_points": _aux,
           "table_outer": _aux, "table_place": _aux, "riesz_assemble": _aux, "vandermonde_solve": _aux,
           "collapsed_quadrature": _aux, "jacobi": _aux}


def seed_of(case):
    return sum(ord(c) * (i + 1) for i, c in enumerate(case["id"])) % (2 ** 31)


def prepare(case):
    return ENTRIES[case["entry"]](case, np.random.default_rng(seed_of(case)))


def compare_tables(got, ref, table_axis, tol=None):
    """Worst (error, bound, table) over the tables: 1e-12 for values, 1e-10 for derivative tables, relative to
    max(1, max |ref|) of the table over the batch."""
    got, ref = np.asarray(got, dtype=float), np.asarray(ref, dtype=float)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    worst = (0.0, TOL_VAL, 0)
    if table_axis is None:
        err = float(np.abs(got - ref).max() / max(1.0, np.abs(ref).max())) if got.size else 0.0
        return [(err, TOL_VAL if tol is None else tol, 0)]
    rows = []
    for t in range(got.shape[table_axis]):
        g, r = np.take(got, t, table_axis), np.take(ref, t, table_axis)
        rows.append((float(np.abs(g - r).max() / max(1.0, np.abs(r).max())), TOL_VAL if t == 0 else TOL_DER, t))
    return rows or [worst]
