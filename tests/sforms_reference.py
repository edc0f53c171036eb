"""NumPy evaluation of the descriptors of fiat_amd/sforms.py (BDMCE / BDMCF and the trimmed serendipity families), for
batches too large for fixtures.  Checked against the reference's fixtures in tests/test_sforms_host.py.

On direction d of the flattened cell, v0 / v1 the first / last vertex coordinate, h = v1 - v0: lambda0 = (v1 - x) / h,
lambda1 = (x - v0) / h, b = lambda0 lambda1, t = 2 x - (v0 + v1); code 0 is lambda0, code 1 lambda1, code 2 + j is L_j(t),
code 3 + k + j is b L_j(t) (L_j Legendre, numpy.polynomial.legendre; 0 <= j <= k).  A (dof, component) is zero or
coefficient * prod_d f_code_d(x_d)."""
import math

import numpy as np
from numpy.polynomial import legendre as npleg


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
    """(order + 1, 2 k + 4, len(x)): the m-th derivative in x of the function of code c.  L_j^(m)(t) comes from NumPy's
    Legendre series (legder); b L_j by Leibniz with b' = -t / h^2, b'' = -2 / h^2; dt/dx = 2."""
    x = np.asarray(x, dtype=float)
    h = v1 - v0
    out = np.zeros((order + 1, 2 * k + 4, len(x)))
    out[0, 0], out[0, 1] = (v1 - x) / h, (x - v0) / h
    if order >= 1:
        out[1, 0], out[1, 1] = -1.0 / h, 1.0 / h
    t = 2.0 * x - (v0 + v1)
    bd = [out[0, 0] * out[0, 1], -t / h ** 2, np.full_like(x, -2.0 / h ** 2)]
    L = np.zeros((order + 1, k + 1, len(x)))          # d^m L_j / dt^m
    for j in range(k + 1):
        c = np.zeros(j + 1)
        c[j] = 1.0
        for m in range(order + 1):
            L[m, j] = npleg.legval(t, npleg.legder(c, m)) if m <= j else 0.0
    for m in range(order + 1):
        out[m, 2:3 + k] = 2.0 ** m * L[m]
        for i in range(min(m, 2) + 1):
            out[m, 3 + k:] += math.comb(m, i) * bd[i] * 2.0 ** (m - i) * L[m - i]
    return out


def tabulate(coef, codes, k, order, pts, lo=None, hi=None):
    """Descriptor (coef (nrows, sd), codes (nrows, sd, sd)) of degree k; pts (..., npts, sd) -> (..., ntab, nrows, sd, npts)
    on the box [lo, hi] (default: the unit box)."""
    coef, codes = np.asarray(coef, dtype=float), np.asarray(codes)
    nrows, sd = coef.shape
    pts = np.asarray(pts, dtype=float)
    lo = np.zeros(sd) if lo is None else np.asarray(lo, dtype=float)
    hi = np.ones(sd) if hi is None else np.asarray(hi, dtype=float)
    lead, npts = pts.shape[:-2], pts.shape[-2]
    flat = pts.reshape(-1, sd)
    F = [line_functions(k, order, flat[:, d], lo[d], hi[d]) for d in range(sd)]
    alphas = mis(sd, order)
    out = np.zeros((len(alphas), nrows, sd, flat.shape[0]))
    nz = coef != 0.0
    for t, alpha in enumerate(alphas):
        v = coef[..., None] * np.ones(flat.shape[0])
        for d in range(sd):
            v = v * F[d][alpha[d]][codes[:, :, d]]
        out[t] = np.where(nz[..., None], v, 0.0)
    out = out.reshape(len(alphas), nrows, sd, *lead, npts)
    return np.moveaxis(out, (0, 1, 2), (-4, -3, -2)) if lead else out


def rel_err(got, ref):
    """The project's norm: max |x - ref| / max(1, max |ref|)."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.max(np.abs(got - ref)) / max(1.0, float(np.max(np.abs(ref))))) if ref.size else 0.0
