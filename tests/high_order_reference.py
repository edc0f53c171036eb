"""Host references for derivative orders 7 and 8 (tests/test_high_order_host.py, tests/test_gpu_high_order.py and the generator
tests/golden/make_golden_high_order.py).  NumPy and the standard library only; imported by the tests, not a conftest.

- lagrange_exact_tables: equispaced Lagrange P_n on the UFC simplex in the MONOMIAL basis with exact rational coefficients
  (the classical product formula L_a = prod_i prod_{k < a_i} (n lambda_i - k) / (k + 1), expanded by polynomial multiplication
  over the integers), differentiated term by term and evaluated at the exact binary values of the points: the plain
  high-precision reference of the operation.  on_set_from_lagrange contracts it with the values of another basis of P_n at the
  lattice nodes (the coefficients of that basis in the Lagrange basis).
- chain_rule_matrices / chain_rule_apply: d^alpha_x from the tables with respect to the reference coordinates X, by the sum over
  ORDERED source directions (the formula of _chain_rule_tables in tests/test_gpu_round4.py), as one matrix per order and cell.
- the cases of tests/golden/high_order.npz, and the oracle's tables in the same layout."""
import itertools
import math
from fractions import Fraction

import numpy as np

LD = np.longdouble
TOL_VAL, TOL_DER = 1e-12, 1e-10          # the suite's standing tolerances
TOL_EXACT = 1e-13                        # fixture and oracle against the exact rational evaluation

# name -> (sd, degree, rebuilt on the physical cells) of the cases of tests/golden/high_order.npz
CASES = {"on10int": (1, 10, False), "p8tri": (2, 8, True), "rt8tri": (2, 8, False), "on8tet": (3, 8, False)}
MAX_ORDER = 8


def mis(sd, k):
    """Multi-indices of length sd and sum k, first entry descending (the order of the tables within one order)."""
    if sd == 1:
        return [(k,)]
    return [(a,) + rest for a in range(k, -1, -1) for rest in mis(sd - 1, k - a)]


def jet(sd, order):
    return [a for k in range(order + 1) for a in mis(sd, k)]


def firsts(sd, order):
    """firsts[k] .. firsts[k + 1]: the tables of order k."""
    return np.cumsum([0] + [len(mis(sd, k)) for k in range(order + 1)])


def ntables(sd, order):
    return math.comb(sd + order, sd)


def ufc_simplex(sd):
    return np.concatenate([np.zeros((1, sd)), np.eye(sd)])


def order_errors(got, want, sd, order):
    """Per order k: max|got - want| / max(1, max|want| over the tables of order k) -- the norm of every figure here."""
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    assert got.shape == want.shape, (got.shape, want.shape)
    f = firsts(sd, order)
    return [float(np.abs(got[f[k]:f[k + 1]] - want[f[k]:f[k + 1]]).max() / max(1.0, np.abs(want[f[k]:f[k + 1]]).max()))
            for k in range(order + 1)]


def assert_close(got, want, sd, order, tag, tol_val=TOL_VAL, tol_der=TOL_DER):
    errs = order_errors(got, want, sd, order)
    for k, err in enumerate(errs):
        assert err <= (tol_val if k == 0 else tol_der), (tag, "order", k, err)
    return errs


# ---------------------------------------------------------------------------------------------------------------------
# exact rational Lagrange


def lattice_numerators(sd, n):
    """Barycentric numerators (a_0, .., a_sd), sum n, of the nodes of Lagrange(UFC simplex, n) in the reference's order
    (vertices, edges, faces, interior: oracle.fiat_oracle.lagrange_nodes, pinned by tests/test_oracle_golden.py)."""
    from oracle import fiat_oracle as fo
    nodes, _ = fo.lagrange_nodes(fo.UFC_SIMPLEX[sd], n)
    x = np.asarray(nodes, dtype=float).reshape(len(nodes), sd)
    num = np.rint(x * n).astype(int)
    assert np.abs(x - num / n).max() < 1e-15 and len(nodes) == math.comb(n + sd, sd)
    return [(n - int(r.sum()),) + tuple(int(v) for v in r) for r in num]


def _poly_mul_linear(p, lin, sd):
    """p * (lin[0] + sum_d lin[d + 1] u_d); polynomials as {exponent tuple: int}."""
    out = {}
    for e, c in p.items():
        if lin[0]:
            out[e] = out.get(e, 0) + c * lin[0]
        for d in range(sd):
            if lin[d + 1]:
                e2 = e[:d] + (e[d] + 1,) + e[d + 1:]
                out[e2] = out.get(e2, 0) + c * lin[d + 1]
    return out


def lagrange_monomial_coefficients(sd, n):
    """(exps, C, den): L_i = sum_j C[j][i] u^exps[j] / den[i] with u = n x, C a matrix of Python ints.  From
    L_a = prod_i prod_{k < a_i} (n lambda_i - k) / (k + 1) with n lambda_0 = n - sum u_d, n lambda_d = u_d."""
    nodes = lattice_numerators(sd, n)
    exps = [e for k in range(n + 1) for e in mis(sd, k)]
    pos = {e: j for j, e in enumerate(exps)}
    C = np.zeros((len(exps), len(nodes)), dtype=object)
    den = []
    for i, a in enumerate(nodes):
        p = {(0,) * sd: 1}
        for v, ai in enumerate(a):
            for k in range(ai):
                lin = [n - k] + [-1] * sd if v == 0 else [-k] + [int(d == v - 1) for d in range(sd)]
                p = _poly_mul_linear(p, lin, sd)
        for e, c in p.items():
            C[pos[e], i] = c
        den.append(math.prod(math.factorial(ai) for ai in a))
    return exps, C, den


def lagrange_exact_tables(sd, n, order, pts, as_fractions=False):
    """Tables (ntab, ndof, npts) of equispaced Lagrange P_n on the UFC simplex, all derivatives of orders <= ``order`` in
    jet order, evaluated exactly at the binary values of ``pts`` (npts, sd).  Returned as (hi, lo) float64 arrays with
    hi + lo the exact value to ~1e-32 (hi alone: the correctly rounded double), or as Fractions."""
    exps, C, den = lagrange_monomial_coefficients(sd, n)
    pts = np.asarray(pts, dtype=float).reshape(-1, sd)
    alphas = jet(sd, order)
    E = np.array(exps, dtype=int)
    hi = np.zeros((len(alphas), C.shape[1], len(pts)))
    lo = np.zeros_like(hi)
    exact = [[[None] * len(pts) for _ in range(C.shape[1])] for _ in alphas] if as_fractions else None
    for p, x in enumerate(pts):
        fr = [Fraction(float(v)) * n for v in x]                       # u_d = n x_d, exactly
        q = 1
        for f in fr:
            q = q * f.denominator // math.gcd(q, f.denominator)
        U = [int(f * q) for f in fr]                                   # u_d = U_d / q
        pw = [[U[d] ** k for k in range(n + 1)] for d in range(sd)]
        qp = [q ** k for k in range(n + 1)]
        # d^alpha u^e = n^|alpha| prod_d e_d! / (e_d - alpha_d)! u_d^(e_d - alpha_d), times q^n to stay in the integers
        Mn = np.zeros((len(alphas), len(exps)), dtype=object)
        for t, al in enumerate(alphas):
            for j, e in enumerate(E):
                if any(e[d] < al[d] for d in range(sd)):
                    continue
                c = n ** sum(al)
                left = 0
                for d in range(sd):
                    c *= math.perm(int(e[d]), al[d]) * pw[d][e[d] - al[d]]
                    left += int(e[d]) - al[d]
                Mn[t, j] = c * qp[n - left]
        num = Mn.dot(C)                                                # (ntab, ndof) Python ints
        scale = qp[n]
        for t in range(len(alphas)):
            for i in range(C.shape[1]):
                v = Fraction(int(num[t, i]), den[i] * scale)
                h = v.numerator / v.denominator                        # int / int: correctly rounded
                hi[t, i, p] = h
                lo[t, i, p] = float(v - Fraction(h))
                if as_fractions:
                    exact[t][i][p] = v
    return exact if as_fractions else (hi, lo)


def on_set_from_lagrange(values_at_nodes, hi, lo):
    """Tables of another basis of P_n from the exact Lagrange tables: member i = sum_j values_at_nodes[i, j] L_j, contracted
    in long double (the coefficients are doubles; the exact tables enter as hi + lo)."""
    c = np.asarray(values_at_nodes, dtype=LD)
    t = np.asarray(hi, dtype=LD) + np.asarray(lo, dtype=LD)
    return np.einsum("ij,tjp->tip", c, t).astype(float)


# ---------------------------------------------------------------------------------------------------------------------
# chain rule


def cell_jacobian_inverse(verts, ref=None):
    """Kt[c, d] = dX_c / dx_d of the affine map from the reference cell ``ref`` (default: UFC) to ``verts``."""
    verts = np.asarray(verts, dtype=float)
    sd = verts.shape[1]
    ref = ufc_simplex(sd) if ref is None else np.asarray(ref, dtype=float)
    J = (verts[1:] - verts[0]).T @ np.linalg.inv((ref[1:] - ref[0]).T)            # dx / dX
    return np.linalg.inv(J)


_SOURCE_INDEX = {}


def _source_index(sd, k):
    """For every ordered tuple of k source directions (row-major over range(sd)^k): the table, within order k, of the
    multi-index that counts them."""
    if (sd, k) not in _SOURCE_INDEX:
        pos = {a: i for i, a in enumerate(mis(sd, k))}
        _SOURCE_INDEX[(sd, k)] = np.array([pos[tuple(src.count(c) for c in range(sd))]
                                           for src in itertools.product(range(sd), repeat=k)], dtype=np.int64)
    return _SOURCE_INDEX[(sd, k)]


def chain_rule_matrices(sd, order, Kt):
    """[M_0, .., M_order]: d^alpha_x = sum_beta M_k[alpha][beta] d^beta_X for |alpha| = k.  Brute force: alpha differentiates
    in the directions d_1 .. d_k, every ORDERED tuple of source directions (c_1 .. c_k) adds prod_m Kt[c_m, d_m] to the
    multi-index beta that counts the c_m -- no recursion over the orders."""
    Kt = np.asarray(Kt, dtype=float)
    out = [np.ones((1, 1))]
    for k in range(1, order + 1):
        idx = _source_index(sd, k)
        alphas = mis(sd, k)
        M = np.zeros((len(alphas), len(alphas)))
        for t, alpha in enumerate(alphas):
            dirs = [d for d, m in enumerate(alpha) for _ in range(m)]
            W = np.ones(())
            for d in dirs:                                             # outer product over the k positions of the tuple
                W = np.multiply.outer(W, Kt[:, d])
            M[t] = np.bincount(idx, weights=W.ravel(), minlength=len(alphas))
        out.append(M)
    return out


def chain_rule_apply(Ms, ref_tab, sd, order):
    """One contraction per order: ref_tab (ntab, ...) with respect to X -> the same shape with respect to x."""
    f = firsts(sd, order)
    ref_tab = np.asarray(ref_tab, dtype=float)
    return np.concatenate([np.tensordot(Ms[k], ref_tab[f[k]:f[k + 1]], axes=1) for k in range(order + 1)])


def chain_rule_tables(ref_tab, sd, order, verts):
    return chain_rule_apply(chain_rule_matrices(sd, order, cell_jacobian_inverse(verts)), ref_tab, sd, order)


# ---------------------------------------------------------------------------------------------------------------------
# the fixture


def truncate(tab8, sd, order):
    """The expectation at ``order`` <= 8 from the stored order-8 jets: their first C(sd + order, sd) tables."""
    return tab8[:ntables(sd, order)]


def oracle_tables(sd, n, coeffs, order, pts, scale, variant):
    """oracle.fiat_oracle on the UFC simplex: (ntab, rows, *value_shape, npts) at pts (npts, sd)."""
    from oracle import fiat_oracle as fo
    tab = fo.element_tabulate(fo.UFC_SIMPLEX[sd], n, np.asarray(coeffs, dtype=float), order, np.asarray(pts, dtype=float), scale, variant)
    return np.stack([tab[a] for a in fo.jet_indices(sd, order)])
