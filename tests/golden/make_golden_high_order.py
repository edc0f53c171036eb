"""Golden vectors of derivative orders 7 and 8, generated from the *unmodified reference* in the build container:

    PYTHONPATH=oracle/restated_deps:/root/reference OMP_NUM_THREADS=1 python -B tests/golden/make_golden_high_order.py

``ho_*`` as in make_golden_round4.py (two cells per case, the second negatively oriented; physical points and their reference
pre-images), at the orders round4.npz does not reach.  Only the ORDER-8 jets are stored, tables in mis() order: the order-7
expectation is their first C(sd + 7, sd) tables.  ``_ref{r}``: the element on the UFC cell at the reference points;
``_phys{r}`` (Lagrange only): the reference's element built ON the physical cell at the physical points.  ``ho_rt8tri_coeffs``:
the reference's coefficients of the vector-valued family (host tests tabulate the oracle with them).

Before saving, the interval, P8-triangle and tetrahedron arrays are compared with the exact rational evaluation of
tests/high_order_reference.py (<= 1e-13 per order, max|x - ref| / max(1, max|ref| over the tables of the order)): Lagrange P8
directly; the ON sets as the exact tables of equispaced P10 / P8 contracted with the set's values at the lattice nodes (its
coefficients in the Lagrange basis, tabulated by the reference).  Plain numbers only."""
import os
import sys

import numpy as np

import FIAT
from FIAT import polynomial_set
from FIAT.polynomial_set import mis
from FIAT.reference_element import UFCSimplex

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                      # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))     # the repository (oracle/)
import high_order_reference as H  # noqa: E402

ORDER = 8


def stack(tab, sd, order):
    return np.stack([np.asarray(tab[a]) for k in range(order + 1) for a in mis(sd, k)])


def physical(sd, verts):
    ref = FIAT.ufc_simplex(sd)
    return UFCSimplex(ref.get_shape(), tuple(map(tuple, verts)), ref.get_topology())


def exact_check(name, sd, degree, base, is_element, ref_pts, arrays):
    """The stored reference-cell arrays of one case against the exact rational evaluation."""
    if is_element:
        values = None
    else:
        nodes = np.array(H.lattice_numerators(sd, degree), dtype=float)[:, 1:] / degree
        values = np.asarray(base.tabulate(nodes, 0)[(0,) * sd])                         # member i at lattice node j
    for r, tab in enumerate(arrays):
        hi, lo = H.lagrange_exact_tables(sd, degree, ORDER, ref_pts[r])
        want = hi if values is None else H.on_set_from_lagrange(values, hi, lo)
        errs = H.order_errors(tab, want, sd, ORDER)
        print(f"  {name} cell {r}: worst error against the exact rational evaluation {max(errs):.2e}  (per order: "
              + " ".join(f"{e:.1e}" for e in errs) + ")", flush=True)
        assert max(errs) <= H.TOL_EXACT, (name, r, errs)


def main():
    rng = np.random.default_rng(7008)
    out = {}
    cases = [("on10int", 1, 10, 3, lambda c: polynomial_set.ONPolynomialSet(c, 10), False, True),
             ("p8tri", 2, 8, 3, lambda c: FIAT.Lagrange(c, 8), True, True),
             ("rt8tri", 2, 8, 3, lambda c: FIAT.RaviartThomas(c, 8), False, False),
             ("on8tet", 3, 8, 2, lambda c: polynomial_set.ONPolynomialSet(c, 8), False, True)]
    for name, sd, degree, npts, make, rebuild, exact in cases:
        ref = np.array(FIAT.ufc_simplex(sd).get_vertices(), dtype=float)
        ncell = 2
        A = np.eye(sd) + 0.25 * rng.standard_normal((ncell, sd, sd))
        A[-1, :, 0] *= -1.0                                          # one negatively oriented cell
        verts = np.einsum("vd,red->rve", ref, A) + rng.standard_normal((ncell, 1, sd))
        e = rng.exponential(size=(ncell, npts, sd + 1))
        bary = e / e.sum(-1, keepdims=True)
        pts, ref_pts = np.einsum("rpv,rvd->rpd", bary, verts), np.einsum("rpv,vd->rpd", bary, ref)
        out[f"ho_{name}_verts"], out[f"ho_{name}_pts"], out[f"ho_{name}_refpts"] = verts, pts, ref_pts
        base = make(FIAT.ufc_simplex(sd))
        is_element = hasattr(base, "dual_basis")
        assert (base.get_nodal_basis() if is_element else base).get_embedded_degree() == degree
        if name == "rt8tri":
            out[f"ho_{name}_coeffs"] = np.asarray(base.get_coeffs())
        for r in range(ncell):
            tab = base.tabulate(ORDER, ref_pts[r]) if is_element else base.tabulate(ref_pts[r], ORDER)
            out[f"ho_{name}_o{ORDER}_ref{r}"] = stack(tab, sd, ORDER)
            if rebuild:
                out[f"ho_{name}_o{ORDER}_phys{r}"] = stack(make(physical(sd, verts[r])).tabulate(ORDER, pts[r]), sd, ORDER)
        print(name, out[f"ho_{name}_o{ORDER}_ref0"].shape, flush=True)
        if exact:
            exact_check(name, sd, degree, base, is_element, ref_pts, [out[f"ho_{name}_o{ORDER}_ref{r}"] for r in range(ncell)])
    path = os.path.join(HERE, "high_order.npz")
    np.savez_compressed(path, **out)
    print(len(out), "arrays ->", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 1 << 20


if __name__ == "__main__":
    main()
