"""NumPy restatement of the IntegratedLegendre tables, written from the definition (FIAT/hierarchical.py:103-114 over
FIAT/expansions.py:140-322); the oracle of tests/test_gpu_hierarchical.py and the subject of tests/test_hierarchical_host.py.

The element's nodal basis is the C0 hierarchy of the bubble-variant expansion set times one scale per entity dimension:
  1. members phi_(p, q, r) of the (-1, 1)^sd simplex by the integrated-Jacobi Dubiner recurrence, first member -sqrt(1 / |K|),
     normalised codimension by codimension;
  2. the corrections that recover the vertex, edge and face functions from them;
  3. the order: vertices, edges, faces, interior, as the reference leaves them;
  4. the scale of the dof's entity dimension (SCALES).
Every member carries its value, gradient and Hessian (a jet); a recurrence step is a product rule.  ``longdouble=True`` runs
the same arithmetic in extended precision: the yardstick for the reference's own round-off."""
import math

import numpy as np

# diag of get_coeffs() by (sd, entity dimension): 1 / (|first member| * prod of the entity's level norms), see scales()
SCALES = {1: (1.154700538379, 1.0),
          2: (1.032795558989, 0.894427191000, 1.074569931824),
          3: (0.780720058359, 0.676123403783, 0.812298515986, 1.189207115003)}


def scales(sd, dtype=np.float64):
    """SCALES to full precision.  The vertex scale is the reciprocal of the normalised first member, sqrt(1 / |K|)
    prod_d sqrt((d + 1/2) / d) with |K| = 2, 2, 4/3 the volume of the (-1, 1)^sd simplex: a vertex function is 1 at its vertex.
    The others are the square roots of 1 | 4/5, 2/sqrt(3) | 16/35, (2/sqrt(3)) (4/7), sqrt(2), read off the reference's
    coefficients; the host test pins this function and SCALES to the diagonal of the fixture's ``get_coeffs()``."""
    one = dtype(1)
    vol = {1: dtype(2), 2: dtype(2), 3: dtype(4) / dtype(3)}[sd]
    lead = np.sqrt(one / vol)
    for d in range(1, sd + 1):
        lead = lead * np.sqrt((dtype(d) + one / 2) / dtype(d))
    out = [one / lead]
    sq = {1: (one,), 2: (dtype(4) / 5, dtype(2) / np.sqrt(dtype(3))), 3: (dtype(16) / 35, dtype(2) / np.sqrt(dtype(3)) * 4 / 7, np.sqrt(dtype(2)))}[sd]
    out.extend(np.sqrt(s) for s in sq)
    return tuple(out)


def mis(sd, order):
    """Multi-indices of one derivative order, first entry descending (the order of the tables)."""
    if sd == 1:
        return [(order,)]
    return [(order - i,) + rest for i in range(order + 1) for rest in mis(sd - 1, i)]


def member_index(idx):
    p, q, r = (tuple(idx) + (0, 0))[:3]
    if len(idx) == 1:
        return p
    if len(idx) == 2:
        return (p + q) * (p + q + 1) // 2 + q
    t, u = p + q + r, q + r
    return t * (t + 1) * (t + 2) // 6 + u * (u + 1) // 2 + r


def lattice(sd, degree):
    """All (p, q, r) with sum <= degree."""
    if sd == 1:
        return [(p,) for p in range(degree + 1)]
    if sd == 2:
        return [(p, q) for p in range(degree + 1) for q in range(degree + 1 - p)]
    return [(p, q, r) for p in range(degree + 1) for q in range(degree + 1 - p) for r in range(degree + 1 - p - q)]


def dof_table(sd, n):
    """[(lattice index, entity dimension)] per dof, in the element's order."""
    rows = []
    if sd == 1:
        rows += [((0,), 0), ((1,), 0)]
        rows += [((i,), 1) for i in range(2, n + 1)]
    elif sd == 2:
        rows += [((0, 0), 0), ((1, 0), 0), ((0, 1), 0)]
        rows += [((1, i - 1), 1) for i in range(2, n + 1)]
        rows += [((0, i), 1) for i in range(2, n + 1)]
        rows += [((i, 0), 1) for i in range(2, n + 1)]
        rows += [((i, j), 2) for j in range(1, n + 1) for i in range(2, n - j + 1)]
    else:
        rows += [((0, 0, 0), 0), ((1, 0, 0), 0), ((0, 1, 0), 0), ((0, 0, 1), 0)]
        rows += [((0, 1, i - 1), 1) for i in range(2, n + 1)]
        rows += [((1, 0, i - 1), 1) for i in range(2, n + 1)]
        rows += [((1, i - 1, 0), 1) for i in range(2, n + 1)]
        rows += [((0, 0, i), 1) for i in range(2, n + 1)]
        rows += [((0, i, 0), 1) for i in range(2, n + 1)]
        rows += [((i, 0, 0), 1) for i in range(2, n + 1)]
        rows += [((1, i - 1, j), 2) for j in range(1, n + 1) for i in range(2, n - j + 1)]
        rows += [((0, i, j), 2) for j in range(1, n + 1) for i in range(2, n - j + 1)]
        rows += [((i, 0, j), 2) for j in range(1, n + 1) for i in range(2, n - j + 1)]
        rows += [((i, j, 0), 2) for j in range(1, n + 1) for i in range(2, n - j + 1)]
        rows += [((i, j, k), 3) for k in range(1, n + 1) for j in range(1, n - k + 1) for i in range(2, n - j - k + 1)]
    return rows


def _jacobi_abc(a, b, n):
    s = a + b
    an = (2 * n + 1 + s) * (2 * n + 2 + s) / (2 * (n + 1) * (n + 1 + s))
    bn = s * (a - b) * (2 * n + 1 + s) / (2 * (n + 1) * (n + 1 + s) * (2 * n + s))
    cn = (n + a) * (n + b) * (2 * n + 2 + s) / ((n + 1) * (n + 1 + s) * (2 * n + s))
    return an, bn, cn


def _integrated_abc(a, b, n):
    if n == 1:
        return (a + b + 2) / 2, (a - 3 * b - 2) / 2, 0 * a
    return _jacobi_abc(a - 1, b + 1, n - 1)


class Jet:
    """Value (npts,), gradient (sd, npts) and Hessian (sd, sd, npts) of one function."""

    def __init__(self, v, g, h):
        self.v, self.g, self.h = v, g, h

    def __mul__(self, o):
        if not isinstance(o, Jet):
            return Jet(self.v * o, self.g * o, self.h * o)
        cross = self.g[:, None] * o.g[None, :]
        return Jet(self.v * o.v, self.g * o.v + self.v * o.g, self.h * o.v + self.v * o.h + cross + cross.transpose(1, 0, 2))

    __rmul__ = __mul__

    def __add__(self, o):
        return Jet(self.v + o.v, self.g + o.g, self.h + o.h)

    def __sub__(self, o):
        return Jet(self.v - o.v, self.g - o.g, self.h - o.h)

    def __neg__(self):
        return Jet(-self.v, -self.g, -self.h)


def expansion_jets(sd, n, pts, A, b, dtype):
    """{lattice index: Jet} of the normalised bubble-variant members at ``pts`` (npts, sd); X = A x + b is the map of the
    element's cell onto the (-1, 1)^sd simplex."""
    pts = np.asarray(pts, dtype=dtype).reshape(-1, sd)
    A = np.asarray(A, dtype=dtype)
    npts = pts.shape[0]
    X = (pts @ A.T + np.asarray(b, dtype=dtype)).T
    zero_g, zero_h = np.zeros((sd, npts), dtype=dtype), np.zeros((sd, sd, npts), dtype=dtype)

    def coordinate(i):   # padded with the constant -1
        if i < sd:
            return Jet(X[i], A[i][:, None] * np.ones(npts, dtype=dtype), zero_h)
        return Jet(-np.ones(npts, dtype=dtype), zero_g, zero_h)

    vol = {1: dtype(2), 2: dtype(2), 3: dtype(4) / dtype(3)}[sd]
    half = dtype(1) / 2
    first = -np.sqrt(dtype(1) / vol)
    pad = lambda idx: tuple(idx) + (0,) * (sd - len(idx))
    mem = {pad(()): Jet(first * np.ones(npts, dtype=dtype), zero_g, zero_h)}
    for codim in range(sd):
        x, y, z = coordinate(codim), coordinate(codim + 1), coordinate(codim + 2)
        fb = (y + z) * half
        fa = x + fb + Jet(np.ones(npts, dtype=dtype), zero_g, zero_h)
        fc = fb * fb
        prefixes = [idx for idx in lattice(codim, n - 1)] if codim else [()]
        for sub in prefixes:
            s = sum(sub)
            alpha = dtype(2 * s)
            a = bcoef = -half
            chain = [pad(sub + (i,)) for i in range(n - s + 1)]
            mem[chain[1]] = mem[chain[0]] * (fa * a - fb * bcoef)
            for i in range(1, n - s):
                a, bcoef, c = _integrated_abc(alpha, dtype(0), dtype(i))
                mem[chain[i + 1]] = mem[chain[i]] * (fa * a - fb * bcoef) - mem[chain[i - 1]] * (fc * c)
        d = codim + 1
        for idx in lattice(d, n):
            p, al = idx[-1], 2 * sum(idx[:-1]) - 1
            norm2 = (dtype(d) + half) / dtype(d)
            if p > 0 and p + al > 0:
                norm2 = norm2 * dtype((p + al) * (2 * p + al)) / dtype(p)
            mem[pad(idx)] = mem[pad(idx)] * np.sqrt(norm2)
    return mem


def c0_jets(sd, n, mem):
    """The corrections that turn the members into vertex, edge and face functions (in place, returns ``mem``)."""
    pad = lambda *idx: tuple(idx) + (0,) * (sd - len(idx))
    unit = [tuple(int(i == j) for i in range(sd)) for j in range(sd)]
    v0 = -mem[pad()]
    for u in unit:
        v0 = v0 - mem[u]
    mem[pad()] = v0
    if sd == 2:
        for i in range(2, n + 1):
            mem[(0, i)] = mem[(0, i)] - mem[(1, i - 1)]
    elif sd == 3:
        for i in range(2, n + 1):
            for j in range(n + 1 - i):
                mem[(0, i, j)] = mem[(0, i, j)] - mem[(1, i - 1, j)]
            mem[(0, 0, i)] = mem[(0, 0, i)] - mem[(0, 1, i - 1)] - mem[(1, 0, i - 1)]
    return mem


def ufc_map(sd, dtype=np.float64):
    """(A, b) of the UFC simplex onto the (-1, 1)^sd simplex."""
    return 2 * np.eye(sd, dtype=dtype), -np.ones(sd, dtype=dtype)


def tabulate(sd, degree, order, pts, A=None, b=None, scale=None, longdouble=False):
    """(ntab, ndof, npts): all derivatives up to ``order`` (<= 2) in mis() order of IntegratedLegendre(degree) on the cell
    that X = A x + b maps onto the (-1, 1)^sd simplex (default: the UFC simplex)."""
    dtype = np.longdouble if longdouble else np.float64
    if A is None:
        A, b = ufc_map(sd, dtype)
    if scale is None:
        scale = scales(sd, dtype)
    mem = c0_jets(sd, degree, expansion_jets(sd, degree, pts, A, b, dtype))
    rows = dof_table(sd, degree)
    npts = np.asarray(pts).reshape(-1, sd).shape[0]
    keys = [a for k in range(order + 1) for a in mis(sd, k)]
    out = np.zeros((len(keys), len(rows), npts), dtype=dtype)
    for r, (idx, dim) in enumerate(rows):
        jet = mem[idx] * scale[dim]
        for t, a in enumerate(keys):
            dirs = [d for d in range(sd) for _ in range(a[d])]
            out[t, r] = jet.v if not dirs else jet.g[dirs[0]] if len(dirs) == 1 else jet.h[dirs[0], dirs[1]]
    return out


def table_error(x, ref):
    """The project's norm: max |x - ref| / max(1, max |ref|)."""
    x, ref = np.asarray(x, dtype=np.longdouble), np.asarray(ref, dtype=np.longdouble)
    return float(np.max(np.abs(x - ref)) / max(1.0, float(np.max(np.abs(ref))))) if ref.size else 0.0
