"""Golden vectors of ``tabulate_on_cells``, generated from the *unmodified reference* in the build container (seconds):

    PYTHONPATH=oracle/restated_deps:/root/reference python -B tests/golden/make_golden_cellmap.py

The reference builds products of interval elements on any intervals, so an element on an axis-aligned box
[0.2, 0.7] x [-1, 0.5] (x [1, 3]) is the reference's own answer to "the unit-cell element mapped to that box".  Every
element is built by ``build(F, name, box)`` below, with F the reference's FIAT (here) or fiat_amd (the tests).  Per case:

``{name}_lo`` / ``_hi``  the box;
``{name}_X``        seeded points of the unit cell, (npts, sd);  ``{name}_x`` their images in the box;
``{name}_tab``      the reference's tabulate(1, x) of the element built ON the box, stacked in mis() order: (ntab, ndof, npts)
                    for the scalar cases (q32: Q3 x Q2 on the quadrilateral, q2hex: Q2^3 on the hexahedron) -- the expected
                    result of tabulate_on_cells(unit-cell element, X, corners = the box's vertices) -- and (ntab, ndof, sd, npts)
                    for the vector cases (rtcf1, nce1), where it is the field on the element's own cell, the box;
``{name}_corners``  vector cases: one seeded cell, the box's vertices moved by up to 15 % of the edges;
``{name}_pushed``   vector cases: the Piola image of ``_tab`` on that cell, tables with respect to the physical coordinates,
                    by this file's own formulas (``pushed`` below): per point, the product rule on J Phi / det J with the
                    determinant differentiated term by term, and J^T phi = Phi differentiated and solved for the covariant map.
Plain float64 and int64 only."""
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

BOX = {2: ((0.2, -1.0), (0.7, 0.5)), 3: ((0.2, -1.0, 1.0), (0.7, 0.5, 3.0))}
CASES = {"q32": (2, "affine"), "q2hex": (3, "affine"), "rtcf1": (2, "contravariant piola"), "nce1": (3, "covariant piola")}
NPTS = 7
ORDER = 1


def mis(sd, k):
    if sd == 2:
        return [(k - i, i) for i in range(k + 1)]
    return [(k - i, i - j, j) for i in range(k + 1) for j in range(i + 1)]


def interval(F, a, b):
    base = F.ufc_simplex(1)
    return F.reference_element.UFCSimplex(base.get_shape(), ((float(a),), (float(b),)), base.get_topology())


def build(F, name, box=None):
    """The case's element on the box (lo, hi) -- default: the unit cell."""
    sd = CASES[name][0]
    lo, hi = box if box is not None else ((0.0,) * sd, (1.0,) * sd)
    I = [interval(F, lo[d], hi[d]) for d in range(sd)]
    T = F.TensorProductElement
    CG = lambda d, n: F.Lagrange(I[d], n)                    # noqa: E731
    DG = lambda d, n: F.DiscontinuousLagrange(I[d], n)       # noqa: E731
    if name == "q32":
        return T(CG(0, 3), CG(1, 2))
    if name == "q2hex":
        return T(T(CG(0, 2), CG(1, 2)), CG(2, 2))
    if name == "rtcf1":
        return F.EnrichedElement(F.Hdiv(T(CG(0, 1), DG(1, 0))), F.Hdiv(T(DG(0, 0), CG(1, 1))))
    if name == "nce1":
        rtce = F.EnrichedElement(F.Hcurl(T(CG(0, 1), DG(1, 0))), F.Hcurl(T(DG(0, 0), CG(1, 1))))
        return F.EnrichedElement(F.Hcurl(T(rtce, CG(2, 1))), F.Hcurl(T(T(CG(0, 1), CG(1, 1)), DG(2, 0))))
    raise ValueError(name)


def q1_map(lo, hi, V, X):
    """J (sd, sd) and dJ[e] = dJ / dX_e of the multilinear map of the box [lo, hi] onto the corners V at the box point X."""
    sd = len(X)
    xi = [(X[d] - lo[d]) / (hi[d] - lo[d]) for d in range(sd)]
    J = np.zeros((sd, sd))
    dJ = np.zeros((sd, sd, sd))
    for i, b in enumerate(itertools.product((0, 1), repeat=sd)):
        f = [xi[d] if b[d] else 1.0 - xi[d] for d in range(sd)]
        s = [(1.0 if b[d] else -1.0) / (hi[d] - lo[d]) for d in range(sd)]
        for d in range(sd):
            J[:, d] += V[i] * s[d] * np.prod([f[m] for m in range(sd) if m != d])
            for e in range(sd):
                if e != d:
                    dJ[e][:, d] += V[i] * s[d] * s[e] * np.prod([f[m] for m in range(sd) if m not in (d, e)])
    return J, dJ


def det_and_derivative(J, dJe):
    """det J and its derivative along one direction, term by term over the permutations."""
    sd = len(J)
    det = ddet = 0.0
    for perm in itertools.permutations(range(sd)):
        sign = np.linalg.det(np.eye(sd)[list(perm)])
        det += sign * np.prod([J[r, perm[r]] for r in range(sd)])
        for k in range(sd):
            ddet += sign * dJe[k, perm[k]] * np.prod([J[r, perm[r]] for r in range(sd) if r != k])
    return det, ddet


def pushed(lo, hi, V, x, tab, mapping):
    """tab (1 + sd, ndof, sd, npts), the field on the box and its box derivatives -> the Piola image on the cell V and its
    derivatives with respect to the physical coordinates."""
    sd = len(lo)
    out = np.zeros_like(tab)
    for p in range(tab.shape[-1]):
        J, dJ = q1_map(lo, hi, V, x[p])
        for i in range(tab.shape[1]):
            Phi, dPhi = tab[0, i, :, p], tab[1:, i, :, p]               # dPhi[e] = d Phi / dX_e
            dref = np.zeros((sd, sd))                                   # dref[e] = d phi / dX_e
            if mapping == "contravariant piola":
                det = det_and_derivative(J, dJ[0])[0]
                phi = J @ Phi / det
                for e in range(sd):
                    ddet = det_and_derivative(J, dJ[e])[1]
                    dref[e] = (dJ[e] @ Phi + J @ dPhi[e]) / det - J @ Phi * ddet / det ** 2
            else:
                phi = np.linalg.solve(J.T, Phi)                         # J^T phi = Phi
                for e in range(sd):
                    dref[e] = np.linalg.solve(J.T, dPhi[e] - dJ[e].T @ phi)
            out[0, i, :, p] = phi
            out[1:, i, :, p] = np.linalg.solve(J.T, dref)              # d/dx_d = sum_e G_ed d/dX_e
    return out


def main():
    import FIAT
    rng = np.random.default_rng(20260712)
    data = {}
    for name, (sd, mapping) in CASES.items():
        lo, hi = (np.array(v) for v in BOX[sd])
        X = rng.uniform(0.05, 0.95, size=(NPTS, sd))
        x = lo + X * (hi - lo)
        el = build(FIAT, name, BOX[sd])
        tab = el.tabulate(ORDER, [tuple(p) for p in x])
        tab = np.stack([np.asarray(tab[a], dtype=np.float64) for k in range(ORDER + 1) for a in mis(sd, k)])
        data.update({f"{name}_lo": lo, f"{name}_hi": hi, f"{name}_X": X, f"{name}_x": x, f"{name}_tab": tab})
        if mapping != "affine":
            assert el.mapping()[0] == mapping
            base = np.array(list(itertools.product(*zip(lo, hi))))
            V = base + rng.uniform(-0.15, 0.15, size=base.shape) * (hi - lo)
            data[f"{name}_corners"] = V
            data[f"{name}_pushed"] = pushed(lo, hi, V, x, tab, mapping)
    np.savez_compressed(os.path.join(HERE, "cellmap.npz"), **data)
    for k, v in data.items():
        print(k, v.shape, v.dtype)


if __name__ == "__main__":
    main()
