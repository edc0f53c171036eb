"""NumPy restatement of the DPC basis on quadrilaterals and hexahedra in closed form (the structure fiat_amd/csrc/dpc.hpp
rests on), for batches too large for fixtures.  Checked against the reference's fixtures in tests/test_dpc_host.py.

DPC_k is P_k with point evaluations at the equispaced degree-k lattice of a simplex that an affine map places over the
cube (FIAT/discontinuous_pc.py:49-97).  The nodal basis of such a lattice is
    phi_alpha(x) = prod_i l_{alpha_i}(lambda_i(x)),   l_a(t) = prod_{j < a} (k t - j) / (j + 1),   |alpha| = k,
lambda the barycentric coordinates of the mapped simplex.  Float64, or ``longdouble=True``: the extended precision of the
host (80 bits on x86), against which the reference's own error is measured."""
import math

import numpy as np


def simplex_vertices(sd, verts=None):
    """Vertices of the mapped simplex (FIAT/discontinuous_pc.py:59-73) on the flattened cell with vertices ``verts``
    (lexicographic; default: the unit cube): the first vertex, the first vertex of the second half, then per further
    direction a vertex plus the mean of every second vertex."""
    if verts is None:
        verts = [[float((i >> (sd - 1 - d)) & 1) for d in range(sd)] for i in range(2 ** sd)]
    v = np.asarray(verts, dtype=float)
    out = [v[0], v[len(v) // 2]]
    for d in range(1, sd):
        out.append(v[sd - d] + np.mean(v[::2], axis=0))
    return np.array(out)


def barycentric_map(sd, verts=None, dtype=np.float64):
    """(lam0 (sd + 1,), G (sd + 1, sd)): lambda = lam0 + G x on the mapped simplex."""
    V = simplex_vertices(sd, verts).astype(dtype)
    H = np.vstack([V.T, np.ones(sd + 1, dtype=dtype)])
    # (numpy.linalg has no extended precision: Gauss-Jordan elimination with partial pivoting in ``dtype``)
    n = sd + 1
    A = np.hstack([H, np.eye(n, dtype=dtype)])
    for c in range(n):
        p = c + int(np.argmax(np.abs(A[c:, c])))
        A[[c, p]] = A[[p, c]]
        A[c] = A[c] / A[c, c]
        for r in range(n):
            if r != c:
                A[r] = A[r] - A[r, c] * A[c]
    M = A[:, n:]
    return M[:, sd].copy(), M[:, :sd].copy()


def _compositions(d, total):
    """multiindex_equal(d, total, 1) of the reference: positive d-tuples summing to total, the last entry slowest."""
    if d == 1:
        if total >= 1:
            yield (total,)
        return
    for last in range(1, total - (d - 1) + 1):
        for head in _compositions(d - 1, total - last):
            yield head + (last,)


_SUBSETS = {2: [[(0,), (1,), (2,)], [(1, 2), (0, 2), (0, 1)], [(0, 1, 2)]],
            3: [[(0,), (1,), (2,), (3,)], [(2, 3), (1, 3), (1, 2), (0, 3), (0, 2), (0, 1)],
                [(1, 2, 3), (0, 2, 3), (0, 1, 3), (0, 1, 2)], [(0, 1, 2, 3)]]}


def descriptor(sd, k):
    """Rows alpha (sd + 1 entries, |alpha| = k) in the reference's node order: the simplex's vertices, edges, faces,
    interior (UFC numbering), each entity's interior lattice from make_points."""
    if k == 0:
        return np.zeros((1, sd + 1), dtype=np.int64)      # DPC0: the constant
    rows = []
    for dim, entities in enumerate(_SUBSETS[sd]):
        for vids in entities:
            for local in _compositions(dim + 1, k):
                alpha = [0] * (sd + 1)
                for v, a in zip(vids, local):
                    alpha[v] = a
                rows.append(alpha)
    return np.array(rows, dtype=np.int64).reshape(-1, sd + 1)


def ndof(sd, k):
    return math.comb(k + sd, sd)


def mis(sd, order):
    """Multi-indices of the tables, all orders <= order, in FIAT's mis() order."""
    out = []
    for o in range(order + 1):
        if sd == 2:
            out += [(o - i, i) for i in range(o + 1)]
        else:
            out += [(o - i, i - j, j) for i in range(o + 1) for j in range(i + 1)]
    return out


def lagrange_functions(k, order, lam):
    """(order + 1, k + 1, n): the m-th derivative in t of l_a at t = lam, by the recurrence l_a = l_{a-1} (k t - a + 1) / a
    and Leibniz: l_a^(m) = (l_{a-1}^(m) (k t - a + 1) + m k l_{a-1}^(m-1)) / a."""
    L = np.zeros((order + 1, k + 1) + lam.shape, dtype=lam.dtype)
    L[0, 0] = 1
    for a in range(1, k + 1):
        f = k * lam - (a - 1)
        for m in range(order + 1):
            s = L[m, a - 1] * f
            if m:
                s = s + m * k * L[m - 1, a - 1]
            L[m, a] = s / a
    return L


def tabulate(sd, k, order, pts, verts=None, longdouble=False):
    """pts (..., npts, sd) -> (..., ntab, ndof, npts) on the flattened cell with vertices ``verts`` (default: the unit
    cube).  Any order: the Cartesian derivative d^alpha is the sum over the ways of giving every derivative to one
    barycentric coordinate."""
    dtype = np.longdouble if longdouble else np.float64
    pts = np.asarray(pts, dtype=dtype)
    lead, npts = pts.shape[:-2], pts.shape[-2]
    flat = pts.reshape(-1, sd)
    lam0, G = barycentric_map(sd, verts, dtype)
    lam = lam0[:, None] + G @ flat.T                              # (sd + 1, n)
    L = [lagrange_functions(k, order, lam[i]) for i in range(sd + 1)]
    rows = descriptor(sd, k)
    alphas = mis(sd, order)
    out = np.zeros((len(alphas), len(rows), flat.shape[0]), dtype=dtype)
    for t, alpha in enumerate(alphas):
        dirs = [d for d in range(sd) for _ in range(alpha[d])]   # one Cartesian direction per derivative
        # every assignment of the derivatives to barycentric coordinates
        for assign in np.ndindex(*([sd + 1] * len(dirs))):
            w = dtype(1)
            for d, i in zip(dirs, assign):
                w = w * G[i, d]
            if w == 0:
                continue
            m = [assign.count(i) for i in range(sd + 1)]
            v = w * np.ones_like(out[t])
            for i in range(sd + 1):
                v = v * L[i][m[i]][rows[:, i]]
            out[t] += v
    out = out.reshape(len(alphas), len(rows), *lead, npts)
    return np.moveaxis(out, (0, 1), (-3, -2)) if lead else out


def rel_err(got, ref):
    """The project's norm: max |x - ref| / max(1, max |ref|)."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.max(np.abs(got - ref)) / max(1.0, float(np.max(np.abs(ref))))) if ref.size else 0.0


# Tolerances against the *reference's fixtures*, (values, derivatives), by degree.  The closed form is within 6e-16 of its
# extended-precision evaluation at every degree; the reference loses digits in its Vandermonde solve (measured distance of
# the fixture from the extended-precision closed form in tests/test_dpc_host.py).  Degrees <= 5: the project's standing
# bounds.  Degree 6: the reference's own hexahedron values are 1.6e-12 away, so 1e-10 on both.  Degree 7 (the general route
# only): ten times the measured distance, 3.7e-13 / 6.0e-13; the factor covers a different LU on the device.
STANDING = (1e-12, 1e-10)
FIXTURE_TOL = {6: (1e-10, 1e-10), 7: (3.7e-12, 6.0e-12)}


def fixture_tol(k):
    return FIXTURE_TOL.get(k, STANDING)
