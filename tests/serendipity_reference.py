"""NumPy restatement of the Serendipity basis S_k on quadrilaterals and hexahedra as signed products of 1-D functions
(the structure fiat_amd/csrc/serendipity.hpp rests on), for batches too large for fixtures.  Checked against the reference's
fixtures in tests/test_serendipity_host.py.

On direction d of the flattened cell, v0 / v1 the first / last vertex coordinate, h = v1 - v0:
lambda0 = (v1 - x) / h, lambda1 = (x - v0) / h, b = lambda0 lambda1, t = 2 x - (v0 + v1); code 0 is lambda0, code 1 lambda1,
code 2 + j is b L_j(t) (Legendre).  A dof is a row (sign; code_x, code_y[, code_z])."""
import math

import numpy as np


def B(j):
    return 2 + j


def descriptor(sd, k):
    """Rows (sign, code_x, code_y[, code_z]) in FIAT's dof order: vertices, edges, faces, interior."""
    ab = (0, 1)
    rows = []
    if sd == 2:
        rows += [(1, a, b) for a in ab for b in ab]
        rows += [(-1, a, B(j)) for a in ab for j in range(k - 1)]
        rows += [(-1, B(j), b) for b in ab for j in range(k - 1)]
        rows += [(1, B(j), B(m - 4 - j)) for m in range(4, k + 1) for j in range(m - 3)]
    elif sd == 3:
        rows += [(1, a, b, c) for a in ab for b in ab for c in ab]
        rows += [(-1, b, a, B(j)) for b in ab for a in ab for j in range(k - 1)]
        rows += [(-1, a, B(j), c) for a in ab for c in ab for j in range(k - 1)]
        rows += [(-1, B(j), c, b) for c in ab for b in ab for j in range(k - 1)]
        rows += [(1, a, B(j), B(m - 4 - j)) for a in ab for m in range(4, k + 1) for j in range(m - 3)]
        rows += [(1, B(m - 4 - j), b, B(j)) for b in ab for m in range(4, k + 1) for j in range(m - 3)]
        rows += [(1, B(j), B(m - 4 - j), c) for c in ab for m in range(4, k + 1) for j in range(m - 3)]
        rows += [(-1, B(l - 6 - j), B(j - i), B(i)) for l in range(6, k + 1) for j in range(l - 5) for i in range(j + 1)]
    else:
        raise ValueError(sd)
    return np.array(rows, dtype=np.int64)


def ndof(sd, k):
    """Closed forms: vertices + edges + faces (+ interior)."""
    face = (k - 3) * (k - 2) // 2 if k >= 4 else 0
    if sd == 2:
        return 4 + 4 * (k - 1) + face
    return 8 + 12 * (k - 1) + 6 * face + (math.comb(k - 3, 3) if k >= 6 else 0)


def mis(sd, order):
    """Multi-indices of the tables, all orders <= order, in FIAT's mis() order."""
    out = []
    for o in range(order + 1):
        if sd == 2:
            out += [(o - i, i) for i in range(o + 1)]
        else:
            out += [(o - i, i - j, j) for i in range(o + 1) for j in range(i + 1)]
    return out


def line_functions(k, order, x, v0, v1):
    """(order + 1, k + 1, len(x)): the m-th derivative in x of the function of code c.  L_j and its derivatives in t by the
    three-term recurrence j L_j = (2j - 1) t L_{j-1} - (j - 1) L_{j-2}, differentiated; then Leibniz with b, b', b'' and
    dt/dx = 2."""
    x = np.asarray(x, dtype=float)
    h = v1 - v0
    out = np.zeros((order + 1, k + 1, len(x)))
    out[0, 0], out[0, 1] = (v1 - x) / h, (x - v0) / h
    if order >= 1:
        out[1, 0], out[1, 1] = -1.0 / h, 1.0 / h
    ne = k - 1
    if ne <= 0:
        return out
    t = 2.0 * x - (v0 + v1)
    bd = [out[0, 0] * out[0, 1], -t / h ** 2, np.full_like(x, -2.0 / h ** 2)]   # b, b', b''
    L = np.zeros((order + 1, ne, len(x)))
    L[0, 0] = 1.0
    if ne > 1:
        L[0, 1] = t
        if order >= 1:
            L[1, 1] = 1.0
    for j in range(2, ne):
        for m in range(order + 1):
            s = t * L[m, j - 1] + (m * L[m - 1, j - 1] if m else 0.0)
            L[m, j] = ((2 * j - 1) * s - (j - 1) * L[m, j - 2]) / j
    for m in range(order + 1):
        for i in range(min(m, 2) + 1):      # b has three nonzero derivatives
            out[m, 2:] += math.comb(m, i) * bd[i] * 2.0 ** (m - i) * L[m - i]
    return out


def tabulate(sd, k, order, pts, lo=None, hi=None):
    """pts (..., npts, sd) -> (..., ntab, ndof, npts) on the box [lo, hi] (default: the unit box)."""
    pts = np.asarray(pts, dtype=float)
    lo = np.zeros(sd) if lo is None else np.asarray(lo, dtype=float)
    hi = np.ones(sd) if hi is None else np.asarray(hi, dtype=float)
    lead, npts = pts.shape[:-2], pts.shape[-2]
    flat = pts.reshape(-1, sd)
    F = [line_functions(k, order, flat[:, d], lo[d], hi[d]) for d in range(sd)]
    rows = descriptor(sd, k)
    alphas = mis(sd, order)
    out = np.empty((len(alphas), len(rows), flat.shape[0]))
    for t, alpha in enumerate(alphas):
        v = rows[:, 0, None].astype(float)
        for d in range(sd):
            v = v * F[d][alpha[d]][rows[:, 1 + d]]
        out[t] = v
    out = out.reshape(len(alphas), len(rows), *lead, npts)
    return np.moveaxis(out, (0, 1), (-3, -2)) if lead else out


def rel_err(got, ref):
    """The project's norm: max |x - ref| / max(1, max |ref|)."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.max(np.abs(got - ref)) / max(1.0, float(np.max(np.abs(ref))))) if ref.size else 0.0
