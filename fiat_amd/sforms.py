"""The vector-valued members of the serendipity complex on quadrilaterals and hexahedra: BDMCE / BDMCF
(FIAT/brezzi_douglas_marini_cube.py) and the trimmed serendipity families (FIAT/Sminus.py, SminusCurl.py, SminusDiv.py).

None of them is a Ciarlet element: the basis is given by formula.  With, per direction of the flattened box, v0 and v1 the
first and last vertex coordinate, h = v1 - v0, lambda0 = (v1 - x) / h, lambda1 = (x - v0) / h, b = lambda0 lambda1 and
t = 2 x - (v0 + v1) (the reference's x_mid: not divided by h), every component of every basis function is zero or ONE term

    coefficient * prod_d f_d(x_d),    f_d in {lambda0, lambda1, L_j(t), b L_j(t)},  L_j Legendre, j <= degree.

The element is therefore a table of (coefficient, code per direction) per (dof, component) -- the *descriptor* built here
in plain Python -- and one data-driven HIP kernel (csrc/sforms.hpp, fx_sforms_tabulate_batch) evaluates it: no sympy, no
expansion set, no coefficient contraction.

Codes of the 1-D family at degree k (``ncodes(k)`` = 2 k + 4 of them):
    0  lambda0      1  lambda1      2 + j  L_j(t)      3 + k + j  b L_j(t)      (0 <= j <= k)
"""
import math
from fractions import Fraction

import numpy

from . import runtime
from .finite_element import FiniteElement
from .polynomial_set import mis
from .reference_element import flatten_reference_cube
from .serendipity import SerendipityDualSet, _flat, _unflatten

MAX_ORDER = 2


def ncodes(k):
    return 2 * k + 4


# ---- a term: coefficient times, per direction, lambda0^p lambda1^q prod L_j ------------------------------------------
class Term:
    """A product of the 1-D building blocks, kept per direction as (power of lambda0, power of lambda1, Legendre degrees).
    ``classify`` names the member of the 1-D family in every direction and fails if there is none."""

    def __init__(self, sd, coef=1, dirs=None):
        self.sd = sd
        self.coef = Fraction(coef)
        self.dirs = dirs if dirs is not None else tuple((0, 0, ()) for _ in range(sd))

    def __mul__(self, other):
        if isinstance(other, Term):
            dirs = tuple((a[0] + b[0], a[1] + b[1], tuple(sorted(a[2] + b[2]))) for a, b in zip(self.dirs, other.dirs))
            return Term(self.sd, self.coef * other.coef, dirs)
        return Term(self.sd, self.coef * Fraction(other), self.dirs)

    __rmul__ = __mul__

    def __neg__(self):
        return self * -1

    def __truediv__(self, n):
        return Term(self.sd, self.coef / Fraction(n), self.dirs)

    def classify(self, k):
        codes = []
        for d, (p, q, legs) in enumerate(self.dirs):
            legs = tuple(j for j in legs if j > 0)          # L_0 = 1
            if len(legs) > 1:
                raise ValueError(f"direction {d}: a product of Legendre polynomials {legs} is outside the 1-D family")
            j = legs[0] if legs else 0
            if j > k:
                raise ValueError(f"direction {d}: L_{j} beyond degree {k}")
            if (p, q) == (0, 0):
                codes.append(2 + j)
            elif (p, q) == (1, 1):
                codes.append(3 + k + j)
            elif (p, q) in ((1, 0), (0, 1)) and j == 0:
                codes.append(q)
            else:
                raise ValueError(f"direction {d}: lambda0^{p} lambda1^{q} L_{j} is outside the 1-D family")
        return float(self.coef), codes


class _Blocks:
    """lam(d, i), bub(d) = lambda0 lambda1 and P(d, j) = L_j on direction d of an sd-dimensional box."""

    def __init__(self, sd):
        self.sd = sd

    def _one(self, d, entry):
        return Term(self.sd, 1, tuple(entry if e == d else (0, 0, ()) for e in range(self.sd)))

    def lam(self, d, i):
        return self._one(d, (1 - i, i, ()))

    def bub(self, d):
        return self._one(d, (1, 1, ()))

    def P(self, d, j):
        if j < 0:
            raise ValueError("negative Legendre degree")
        return self._one(d, (0, 0, (j,)))


def _rot(rows):
    """(a0, a1) -> (-a1, a0): the H(div) partner of an H(curl) basis on the quadrilateral."""
    return [(None if a[1] is None else -a[1], a[0]) for a in rows]


# ---- the bases, as lists of rows of sd components (None: zero), in the reference's dof order --------------------------
def bdmce_rows(k):
    """BDMCE_k (FIAT/brezzi_douglas_marini_cube.py:140-213): per edge k lower-order tangential functions and one of degree
    k corrected by a bubble so that the curl stays of degree k - 1; then the interior functions."""
    B = _Blocks(2)
    X, Y = 0, 1
    c = Fraction(math.comb(2 * k, k), (k + 1) * math.comb(2 * k - 2, k - 1))
    rows = []
    for tang, norm in ((Y, X), (X, Y)):          # edges x = const (tangent y), then edges y = const (tangent x)
        for side in (0, 1):
            sgn = -1 if side == 0 else 1
            for j in range(k):
                f = -B.P(tang, j) * B.lam(norm, side)
                rows.append((None, f) if tang == Y else (f, None))
            top = -B.P(tang, k) * B.lam(norm, side)
            fix = c * sgn * B.P(tang, k - 1) * B.bub(tang)
            rows.append((fix, top) if tang == Y else (top, fix))
    for m in range(2, k + 1):
        for j in range(m - 1):
            rows.append((None, B.P(X, j) * B.P(Y, m - 2 - j) * B.bub(X)))
            rows.append((B.P(X, m - 2 - j) * B.P(Y, j) * B.bub(Y), None))
    return rows


def _trimmed_quad_edges(B, k):
    X, Y = 0, 1
    rows = []
    for side in (0, 1):
        rows += [(None, -B.P(Y, j) * B.lam(X, side)) for j in range(k)]
    for side in (0, 1):
        rows += [(-B.P(X, j) * B.lam(Y, side), None) for j in range(k)]
    return rows


def _trimmed_quad_tilde(B, k):
    X, Y = 0, 1
    rows = [(B.P(Y, k - 2) * B.bub(Y), None), (None, B.P(X, k - 2) * B.bub(X))]
    for j in range(1, k - 1):
        rows.append((B.P(X, j) * B.P(Y, k - j - 2) * B.bub(Y), -B.P(X, j - 1) * B.P(Y, k - j - 1) * B.bub(X)))
    return rows


def trimmed_quad_curl_rows(k):
    """S^-_k Lambda^1 on the quadrilateral as FIAT/Sminus.py:162-240 and FIAT/SminusCurl.py:355-433 list it (the two agree):
    the basis of TrimmedSerendipityEdge and TrimmedSerendipityCurl; TrimmedSerendipityFace is its rotation."""
    B = _Blocks(2)
    X, Y = 0, 1
    rows = _trimmed_quad_edges(B, k)
    if k >= 2:
        for m in range(2, k):
            for j in range(m - 1):
                f = B.P(X, j) * B.P(Y, m - 2 - j)
                rows.append((f * B.bub(Y), None))
                rows.append((None, f * B.bub(X)))
        rows += _trimmed_quad_tilde(B, k)
    return rows


def trimmed_quad_div_preimage_rows(k):
    """The H(curl) basis TrimmedSerendipityDiv rotates on the quadrilateral (FIAT/SminusDiv.py:234-321).  It differs from
    ``trimmed_quad_curl_rows`` in the lower-order interior functions: their order within a pair and which factor carries
    which degree (:307-314 against FIAT/Sminus.py:203-222), so SminusDiv is NOT SminusF from degree 3 on."""
    B = _Blocks(2)
    X, Y = 0, 1
    rows = _trimmed_quad_edges(B, k)
    if k >= 2:
        for m in range(2, k):
            for j in range(m - 1):
                rows.append((None, B.P(X, j) * B.P(Y, m - 2 - j) * B.bub(X)))
                rows.append((B.P(X, m - 2 - j) * B.P(Y, j) * B.bub(Y), None))
        rows += _trimmed_quad_tilde(B, k)
    return rows


def _hex_edge_rows(B, k):
    """The 12 edges in the hexahedron's numbering: along z, along y, along x (FIAT/SminusCurl.py:198-236)."""
    X, Y, Z = 0, 1, 2
    rows = []
    for i in (0, 1):
        for j in (0, 1):
            rows += [(None, None, B.P(Z, n) * B.lam(X, i) * B.lam(Y, j)) for n in range(k)]
    for i in (0, 1):
        for j in (0, 1):
            rows += [(None, B.P(Y, n) * B.lam(X, i) * B.lam(Z, j), None) for n in range(k)]
    for i in (0, 1):
        for j in (0, 1):
            rows += [(B.P(X, n) * B.lam(Y, i) * B.lam(Z, j), None, None) for n in range(k)]
    return rows


def _vec(sd, **comps):
    row = [None] * sd
    for name, term in comps.items():
        row[int(name[1:])] = term
    return tuple(row)


def _hex_face_tilde(B, k, n, side, u, v):
    face = B.lam(n, side)
    rows = [_vec(3, **{f"c{u}": B.P(v, k - 2) * face * B.bub(v)}), _vec(3, **{f"c{v}": B.P(u, k - 2) * face * B.bub(u)})]
    for j in range(1, k - 1):
        rows.append(_vec(3, **{f"c{u}": B.P(u, j) * B.P(v, k - j - 2) * face * B.bub(v),
                               f"c{v}": -B.P(u, j - 1) * B.P(v, k - j - 1) * face * B.bub(u)}))
    return rows


_HEX_FACES = [(0, 0, 1, 2), (0, 1, 1, 2), (1, 0, 0, 2), (1, 1, 0, 2), (2, 0, 0, 1), (2, 1, 0, 1)]   # normal, side, u, v


def trimmed_hex_curl_rows(k):
    """S^-_k Lambda^1 on the hexahedron as FIAT/SminusCurl.py:198-351 lists it, degrees 1-5."""
    B = _Blocks(3)
    X, Y, Z = 0, 1, 2
    rows = _hex_edge_rows(B, k)
    if k > 1:
        for n, side, u, v in _HEX_FACES:
            rows += _hex_face_tilde(B, k, n, side, u, v)
            face = B.lam(n, side)
            for m in range(2, k):
                for j in range(m - 1):
                    q = m - 2 - j
                    rows.append(_vec(3, **{f"c{u}": B.P(u, j) * B.P(v, q) * face * B.bub(v)}))
                    rows.append(_vec(3, **{f"c{v}": B.P(v, j) * B.P(u, q) * face * B.bub(u)}))
    if k > 3:
        if k > 5:
            raise NotImplementedError("TrimmedSerendipityCurl on the hexahedron from degree 6: the reference multiplies two "
                                      "Legendre polynomials in the same variable (outside the 1-D family)")
        bx, by, bz = B.bub(X), B.bub(Y), B.bub(Z)
        for m in range(4, k):
            for j in range(m - 3):
                for i in range(m - 3 - j):
                    f = B.P(X, j) * B.P(Y, i) * B.P(Z, m - 4 - j - i)
                    rows += [(f * by * bz, None, None), (None, f * bx * bz, None), (None, None, f * bx * by)]
        if k == 4:
            rows += [(by * bz, None, None), (None, bx * bz, None), (None, None, bx * by)]
        else:
            rows += [(B.P(Y, k - 4) * by * bz, None, None), (B.P(Z, k - 4) * by * bz, None, None),
                     (None, B.P(X, k - 4) * bx * bz, None), (None, B.P(Z, k - 4) * bx * bz, None),
                     (None, None, B.P(X, k - 4) * bx * by), (None, None, B.P(Y, k - 4) * bx * by)]
        for j in range(1, k - 3):
            rows.append((B.P(X, j) * B.P(Y, k - j - 4) * by * bz, -B.P(X, j - 1) * B.P(Y, k - j - 3) * bx * bz, None))
            rows.append((B.P(X, j) * B.P(Z, k - j - 4) * by * bz, None, -B.P(X, j - 1) * B.P(Z, k - j - 3) * bx * by))
    return rows


def trimmed_hex_edge_rows(k):
    """TrimmedSerendipityEdge on the hexahedron as FIAT/Sminus.py:243-356 lists it, degrees 1-3 (the lower-order face
    functions carry a factor L_q with q = k - j - 2 in a direction that already has a lambda: 1 only while k <= 3)."""
    B = _Blocks(3)
    rows = _hex_edge_rows(B, k)
    if k >= 2:
        for n, side, u, v in _HEX_FACES:
            rows += _hex_face_tilde(B, k, n, side, u, v)
            face = B.lam(n, side)
            w = u if n == 2 else n
            for j in range(1, k - 1):
                q = k - j - 2
                rows.append(_vec(3, **{f"c{u}": B.P(u, j) * B.P(v, q) * face * B.bub(v)}))
                rows.append(_vec(3, **{f"c{v}": B.P(v, j) * B.P(w, q) * face * B.bub(u)}))
    return rows


def trimmed_hex_div_rows(k):
    """S^-_k Lambda^2 on the hexahedron as FIAT/SminusDiv.py:180-230 lists it, degrees 1-5."""
    B = _Blocks(3)
    X, Y, Z = 0, 1, 2
    bx, by, bz = B.bub(X), B.bub(Y), B.bub(Z)
    rows = []
    for n, (u, v), sgn in ((X, (Y, Z), -1), (Y, (X, Z), 1), (Z, (X, Y), -1)):
        for side in (0, 1):
            for i in range(k):
                for j in range(k - i):
                    rows.append(_vec(3, **{f"c{n}": sgn * B.P(u, j) * B.P(v, i) * B.lam(n, side)}))
    if k > 1:
        for m in range(2, k):
            for j in range(m - 1):
                for i in range(m - 1 - j):
                    f = B.P(X, j) * B.P(Y, i) * B.P(Z, m - 2 - j - i)
                    rows += [(None, None, -f * bz), (None, -f * by, None), (-f * bx, None, None)]
        rows += [(None, None, B.P(Z, k - 2) * bz), (None, B.P(Y, k - 2) * by, None), (B.P(X, k - 2) * bx, None, None)]
        rows += [(B.P(X, k - j - 2) * B.P(Y, j) * bx, B.P(X, k - j - 1) * B.P(Y, j - 1) * by, None) for j in range(1, k - 1)]
        rows += [(B.P(X, k - j - 2) * B.P(Z, j) * bx, None, B.P(X, k - j - 1) * B.P(Z, j - 1) * bz) for j in range(1, k - 1)]
        rows += [(None, B.P(Y, k - j - 2) * B.P(Z, j) * by, B.P(Y, k - j - 1) * B.P(Z, j - 1) * bz) for j in range(1, k - 1)]
        for i in range(1, k - 2):
            for l in range(1, k - 1 - i):
                j = k - 2 - i - l
                rows.append((-B.P(X, j) * B.P(Y, i) * B.P(Z, l) * bx, B.P(X, j + 1) * B.P(Y, i - 1) * B.P(Z, l) * by,
                             -B.P(X, j + 1) * B.P(Y, i) * B.P(Z, l - 1) * bz))
    return rows


FAMILIES = ("BDMCE", "BDMCF", "SminusE", "SminusF", "SminusCurl", "SminusDiv")
# (family, sd) -> (largest degree, why not beyond)
MAX_DEGREE = {
    ("BDMCE", 2): 6, ("BDMCF", 2): 6, ("SminusE", 2): 6, ("SminusF", 2): 6, ("SminusCurl", 2): 6, ("SminusDiv", 2): 6,
    ("SminusDiv", 3): 5, ("SminusCurl", 3): 5, ("SminusE", 3): 3,
}
_WHY = {
    ("SminusE", 3): "from degree 4 the reference's dof count and its list of basis functions disagree",
    ("SminusCurl", 3): "at degree 6 the reference multiplies two Legendre polynomials in the same variable",
}

_descriptors = {}


def descriptor(family, sd, k):
    """(coef, codes) of ``family`` at degree k on the sd-dimensional box: coef (nrows, sd) float64, 0.0 where the component
    is zero; codes (nrows, sd, sd) int32, the code of direction d of component c of dof i at [i, c, d] (0 where the
    component is zero).  Rows in the reference's dof order.  Raises ValueError if a factor leaves the 1-D family."""
    key = (family, sd, k)
    if key in _descriptors:
        return _descriptors[key]
    if (family, sd) not in MAX_DEGREE:
        raise NotImplementedError(f"{family} in dimension {sd}")
    if k < 1:
        raise ValueError("the degree is positive")
    if k > MAX_DEGREE[family, sd]:
        why = _WHY.get((family, sd), "the kernel's 1-D tables are sized for this range")
        raise NotImplementedError(f"{family} of degree {k} in dimension {sd} (1..{MAX_DEGREE[family, sd]}): {why}")
    if sd == 2:
        rows = {"BDMCE": lambda: bdmce_rows(k), "BDMCF": lambda: _rot(bdmce_rows(k)),
                "SminusE": lambda: trimmed_quad_curl_rows(k), "SminusCurl": lambda: trimmed_quad_curl_rows(k),
                "SminusF": lambda: _rot(trimmed_quad_curl_rows(k)),
                "SminusDiv": lambda: _rot(trimmed_quad_div_preimage_rows(k))}[family]()
    else:
        rows = {"SminusE": trimmed_hex_edge_rows, "SminusCurl": trimmed_hex_curl_rows, "SminusDiv": trimmed_hex_div_rows}[family](k)
    coef = numpy.zeros((len(rows), sd), dtype=numpy.float64)
    codes = numpy.zeros((len(rows), sd, sd), dtype=numpy.int32)
    for i, row in enumerate(rows):
        if len(row) != sd:
            raise ValueError(f"dof {i}: {len(row)} components")
        for c, term in enumerate(row):
            if term is None:
                continue
            try:
                coef[i, c], codes[i, c] = term.classify(k)
            except ValueError as e:
                raise ValueError(f"{family} degree {k}, dof {i}, component {c}: {e}") from None
            if coef[i, c] == 0.0:
                raise ValueError(f"{family} degree {k}, dof {i}, component {c}: zero coefficient")
    coef.setflags(write=False)
    codes.setflags(write=False)
    _descriptors[key] = (coef, codes)
    return coef, codes


# ---- entity dofs on the flattened cell ---------------------------------------------------------------------------------
def _tri(n):
    return (n * (n + 1)) // 2


def flat_entity_ids(family, flat_el, k):
    """({dim: {entity: [dofs]}}, the reference's dof count) on the flattened cell.  The count is what the reference sizes
    its dual with; at degree 1 the trimmed quadrilateral elements count 5 but number and tabulate 4 functions."""
    sd = flat_el.get_spatial_dimension()
    topology = flat_el.get_topology()
    ids = {dim: {e: [] for e in topology[dim]} for dim in topology}
    cur = 0

    def give(dim, per_entity):
        nonlocal cur
        for e in sorted(topology[dim]):
            ids[dim][e] = list(range(cur, cur + per_entity))
            cur += per_entity

    if family in ("BDMCE", "BDMCF"):
        give(1, k + 1)
        give(2, 2 * _tri(k - 1))
        return ids, cur
    if sd == 2:
        give(1, k)
        inner = 2 * _tri(k - 2) + k
        if k >= 2:
            ids[2][0] = list(range(cur, cur + inner))
        return ids, cur + inner
    if family == "SminusDiv":
        give(2, _tri(k))
        inner = sum(3 * _tri(m - 1) for m in range(2, k))          # the lower-order interior functions
        if k > 1:
            inner += 3 * (k - 1)
        if k >= 4:
            inner += _tri(k - 1) - 2 * (k - 1) + 1
        give(3, inner)
        return ids, cur
    give(1, k)
    if family == "SminusCurl":
        if k > 1:
            give(2, k + sum(2 * (m - 1) for m in range(2, k)))
        inner = sum(3 * _tri(m - 3) for m in range(4, k)) + {4: 3, 5: 8}.get(k, 0)
        give(3, inner)
        return ids, cur
    if k >= 2:                                                      # SminusE on the hexahedron, degrees <= 3
        give(2, 2 * _tri(k - 2) + k)
    return ids, cur


# ---- the elements ------------------------------------------------------------------------------------------------------
class SFormElement(FiniteElement):
    """Common facade of the six classes: ``_family`` names the descriptor, ``_mapping_name`` the Piola map."""

    _family = None
    _mapping_name = None
    _hex = True

    def __init__(self, ref_el, degree):
        name = type(self).__name__
        if degree < 1:
            raise Exception(f"{name} elements only valid for k >= 1")
        flat_el = flatten_reference_cube(ref_el)
        sd = flat_el.get_spatial_dimension()
        if sd != 2 and not (self._hex and sd == 3):
            raise Exception(f"{name} elements only valid for dimension" + (" 2" if not self._hex else "s 2 and 3"))
        degree = int(degree)
        self._coef, self._codes = descriptor(self._family, sd, degree)        # NotImplementedError beyond the table
        self.flat_el = flat_el
        self.fdim = sd
        verts = numpy.asarray(flat_el.get_vertices(), dtype=numpy.float64)
        self._lo = numpy.ascontiguousarray(verts[0])
        self._hi = numpy.ascontiguousarray(verts[-1])
        self._flat_ids, count = flat_entity_ids(self._family, flat_el, degree)
        product = ref_el.get_dimension() != max(self._flat_ids)
        entity_ids = _unflatten(ref_el, self._flat_ids) if product else self._flat_ids
        formdegree = sd - 1 if self._family == "SminusDiv" else 1
        # (as in the reference the dual holds no functionals: ``count`` None nodes)
        super().__init__(ref_el, SerendipityDualSet([None] * count, ref_el, entity_ids), degree, formdegree,
                         self._mapping_name)
        self._tables = {}

    def degree(self):
        return self.get_order()

    def value_shape(self):
        return (self.fdim,)

    def num_rows(self):
        """Rows of a table: the number of basis functions listed (space_dimension() is the reference's dual count)."""
        return self._coef.shape[0]

    def dual_basis(self):
        raise NotImplementedError(f"dual_basis is not implemented for {type(self).__name__}")

    def get_coeffs(self):
        raise NotImplementedError(f"get_coeffs not implemented for {type(self).__name__}")

    def descriptor(self):
        return self._coef, self._codes

    def _table(self, ctx=None):
        """The term table on the device: uploaded once per element and device."""
        ctx = ctx or runtime.Context.get()
        if ctx not in self._tables:
            self._tables[ctx] = runtime.SFormsTable(self.fdim, self.order, self._coef, self._codes, ctx=ctx)
        return self._tables[ctx]

    def kernel(self, order, npts):
        """Kernel instance, output route, requests per item and image budget of a request shape (fx_sforms_kernel)."""
        return runtime.sforms_kernel(self.fdim, self.order, self.num_rows(), order, npts)

    def out_shape(self, order, nreq, npts):
        return (nreq, runtime.num_tables(self.fdim, order), self.num_rows(), self.fdim, npts)

    def tabulate(self, order, points, entity=None):
        """{alpha: (nrows, sd, npts)} of all derivatives up to ``order``; ``entity=(dim, id)``: the points are in the
        coordinates of that sub-entity of the element's cell."""
        points = numpy.asarray(points, dtype=float)
        if points.ndim != 2:
            raise ValueError("points must have shape (npts, dimension of the entity)")
        dev = self.tabulate_batch(order, points[None], entity=entity)
        out = runtime.fetch(dev)[0]
        keys = [a for k in range(order + 1) for a in mis(self.fdim, k)]
        return {a: numpy.ascontiguousarray(out[t]) for t, a in enumerate(keys)}

    def tabulate_batch(self, order, points, verts=None, out=None, stream=None, pushforward=False, entity=None):
        """points (nreq, npts, sd) -> device tensor (nreq, ntab, nrows, sd, npts), tables in mis() order.
        ``entity=(dim, id)``: points (nreq, npts, dim) on that sub-entity, mapped into the cell on the device
        (fx_map_points) before the same kernel runs.  ``verts`` must stay None (the families live on axis-aligned boxes: a
        bilinear cell is no affine image); ``pushforward`` changes nothing (the element's own cell)."""
        if verts is not None:
            raise NotImplementedError(f"{type(self).__name__} elements have no per-request cells")
        order = int(order)
        if order > MAX_ORDER:
            raise NotImplementedError(f"derivative order {order} > {MAX_ORDER}")
        if entity is not None and entity[0] != self.ref_el.get_dimension():
            points = runtime.map_points(*self._entity_affine(entity), points, stream=stream)
        return runtime.sforms_tabulate_batch(self._table(), self._lo, self._hi, order, points, out=out, stream=stream)

    def _entity_affine(self, entity):
        """(M, b) of x = M xi + b, from the cell's get_entity_transform."""
        dim, number = entity
        sd = self.fdim
        f = self.ref_el.get_entity_transform(dim, number)
        edim = sum(_flat(dim))
        b = numpy.asarray(f(numpy.zeros((1, edim))), dtype=float).reshape(sd)
        M = numpy.zeros((sd, edim))
        for i in range(edim):
            unit = numpy.zeros((1, edim))
            unit[0, i] = 1.0
            M[:, i] = numpy.asarray(f(unit), dtype=float).reshape(sd) - b
        return M, b
