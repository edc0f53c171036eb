"""NumPy restatement of the multilinear (Q1) cell map of ``fiat_amd.cellmap`` (csrc/cellmap.hpp): the shape functions and
their derivatives, x, J, det J and the second derivatives of the map, and the three maps applied to reference tables.
Imported by tests/test_cellmap_host.py and tests/test_gpu_cellmap.py; NumPy only, not a conftest.

    xi_d = (X_d - lo_d) / (hi_d - lo_d),  N_i = prod_d (bit_d(i) ? xi_d : 1 - xi_d)  (bit SD-1-d of i: last coordinate fastest)
    x = sum_i N_i v_i,  J_ad = dx_a / dX_d,  G = J^-1,  (d_e J)_ad = d2 x_a / dX_d dX_e
    affine:         out_0 = Phi,   out_{1+d} = sum_e d_e Phi G_ed
    covariant:      M = G^T,       contravariant: M = J / det J (signed)
    phi = M Phi,    d phi / dx_d = sum_e G_ed (d_e M Phi + M d_e Phi),  d_e G = -G d_e J G,  d_e det J = det J tr(G d_e J)"""
import itertools

import numpy as np

AFFINE, COVARIANT, CONTRAVARIANT = 0, 1, 2
MAPPINGS = {"affine": AFFINE, "covariant piola": COVARIANT, "contravariant piola": CONTRAVARIANT}
VALUES, DERIVATIVES = 1e-12, 1e-10          # the project's bars, in the norm of ``rel``


def bits(sd):
    return np.array(list(itertools.product((0, 1), repeat=sd)))          # vertex i -> (bit of coordinate 0, 1[, 2])


def unit_corners(sd, lo=None, hi=None):
    """The vertices of the box [lo, hi] in the order of get_vertices(): the last coordinate fastest."""
    lo = np.zeros(sd) if lo is None else np.asarray(lo, dtype=float)
    hi = np.ones(sd) if hi is None else np.asarray(hi, dtype=float)
    return np.where(bits(sd) == 1, hi, lo)


def shape_functions(sd, xi):
    """xi (..., sd) -> N (..., 2^sd), dN (..., 2^sd, sd), d2N (..., 2^sd, sd, sd), derivatives with respect to xi."""
    xi = np.asarray(xi)
    B = bits(sd)
    f = np.where(B == 1, xi[..., None, :], 1 - xi[..., None, :])       # (..., 2^sd, sd)
    s = np.where(B == 1, 1.0, -1.0)
    N = f.prod(-1)
    dN = np.empty(f.shape, dtype=f.dtype)
    d2N = np.zeros(f.shape + (sd,), dtype=f.dtype)
    for e in range(sd):
        dN[..., e] = s[:, e] * np.delete(f, e, axis=-1).prod(-1)
        for h in range(sd):
            if h != e:
                d2N[..., e, h] = s[:, e] * s[:, h] * np.delete(f, [e, h], axis=-1).prod(-1)
    return N, dN, d2N


def geometry(lo, hi, X, corners):
    """X (nreq, npts, sd) in the box [lo, hi], corners (nreq, 2^sd, sd) -> x (nreq, npts, sd), J (nreq, npts, sd, sd),
    detJ (nreq, npts), H (nreq, npts, sd, sd, sd) with H[..., a, d, e] = d2 x_a / dX_d dX_e."""
    X, corners = np.asarray(X), np.asarray(corners)
    lo, hi = np.asarray(lo, dtype=float), np.asarray(hi, dtype=float)
    sd = X.shape[-1]
    ih = 1.0 / (hi - lo)
    N, dN, d2N = shape_functions(sd, (X - lo) / (hi - lo))
    x = np.einsum("rpi,ria->rpa", N, corners)
    J = np.einsum("rpid,ria->rpad", dN * ih, corners)
    H = np.einsum("rpide,ria->rpade", d2N * ih[:, None] * ih[None, :], corners)
    return x, J, np.linalg.det(J), H


def piola(mapping, J, H):
    """M (nreq, npts, c, k) and dM (nreq, npts, e, c, k) = dM / dX_e."""
    G = np.linalg.inv(J)
    det = np.linalg.det(J)
    GdJ = np.einsum("rpia,rpade->rpeid", G, H)                           # G d_e J
    if mapping == COVARIANT:
        M = np.swapaxes(G, -1, -2)
        dM = -np.einsum("rpekd,rpdc->rpeck", GdJ, G)                    # (d_e G)[k][c]
    elif mapping == CONTRAVARIANT:
        M = J / det[..., None, None]
        tr = np.einsum("rpeii->rpe", GdJ)
        dM = (np.einsum("rpcke->rpeck", H) - J[:, :, None] * tr[..., None, None]) / det[..., None, None, None]
    else:
        raise ValueError(mapping)
    return M, dM


def apply(lo, hi, X, corners, tab, mapping=AFFINE):
    """Reference tables tab (nreq, ntab, ndof, [sd,] npts), ntab 1 or 1 + sd, tabulated at X -> the physical tables."""
    tab = np.asarray(tab)
    sd = np.asarray(X).shape[-1]
    order = 0 if tab.shape[1] == 1 else 1
    assert tab.shape[1] == 1 + sd * order
    _, J, _, H = geometry(lo, hi, X, corners)
    G = np.linalg.inv(J)
    out = np.empty_like(tab)
    if mapping == AFFINE:
        out[:, 0] = tab[:, 0]
        if order:
            out[:, 1:] = np.einsum("re...p,rped->rd...p", tab[:, 1:], G)
        return out
    assert tab.ndim == 5 and tab.shape[3] == sd
    M, dM = piola(mapping, J, H)
    out[:, 0] = np.einsum("rpck,rikp->ricp", M, tab[:, 0])
    if order:
        dref = np.einsum("rpeck,rikp->reicp", dM, tab[:, 0]) + np.einsum("rpck,reikp->reicp", M, tab[:, 1:])
        out[:, 1:] = np.einsum("reicp,rped->rdicp", dref, G)
    return out


def perturbed_cells(rng, nreq, sd, lo=None, hi=None, amount=0.15):
    """The box plus U(-amount, amount) per corner coordinate, scaled by the box's edges: det J of the map from the unit box
    stays >= 0.39 for amount 0.15 (2 000 seeded cells, corners and interior points)."""
    base = unit_corners(sd, lo, hi)
    edge = base.max(0) - base.min(0)
    return base + rng.uniform(-amount, amount, size=(nreq,) + base.shape) * edge


def box_points(rng, nreq, npts, lo, hi):
    lo, hi = np.asarray(lo, dtype=float), np.asarray(hi, dtype=float)
    return lo + rng.uniform(0.0, 1.0, size=(nreq, npts, len(lo))) * (hi - lo)


def rel(got, ref):
    """max|got - ref| / max(1, max|ref|)."""
    got, ref = np.asarray(got, dtype=float), np.asarray(ref, dtype=float)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / max(1.0, np.abs(ref).max())) if ref.size else 0.0


def errors(got, ref):
    """(values, derivatives) in the norm of ``rel``, tables on axis 1."""
    got, ref = np.asarray(got), np.asarray(ref)
    return rel(got[:, :1], ref[:, :1]), (rel(got[:, 1:], ref[:, 1:]) if ref.shape[1] > 1 else 0.0)
