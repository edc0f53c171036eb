"""TEST INFRASTRUCTURE -- NumPy restatement of the fused evaluation kernel (fiat_amd/csrc/evaluate.hpp), in the kernel's own
order of operations: fold (bubble: coeffs . T, columns in the order of the walk), transform (w = A'^T c), walk (the
Dubiner recurrence depth first, every member multiplied into the accumulators as it appears), Piola matrix.  Built on
oracle/fiat_oracle.py (recurrence coefficients, member numbering, C0 basis, cell maps); ``longdouble=True`` runs everything
after the fold in extended precision."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import fiat_oracle as fo  # noqa: E402

VARIANTS = {0: None, 1: "bubble", 2: "dual"}
MAXK, MAXORDER, MAXRHS = 6, 2, 8              # the instance set of evaluate.hpp
LDS_BYTES, RB, GRID_PER_CU = 16 * 1024, 4, 32


def jet(sd, order):
    return fo.jet_indices(sd, order)


def error(got, ref):
    """The project's norm: max |x - ref| / max(1, max |ref|)."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.max(np.abs(got - ref)) / max(1.0, float(np.max(np.abs(ref))))) if ref.size else 0.0


def errors(got, ref):
    """(values, derivatives) of results (ntab, ...)."""
    return error(got[:1], ref[:1]), (error(got[1:], ref[1:]) if ref.shape[0] > 1 else 0.0)


def walk_members(sd, n):
    """Lattice indices in the order of the walk: p slowest, then q, then r."""
    if sd == 1:
        return [(p,) for p in range(n + 1)]
    if sd == 2:
        return [(p, q) for p in range(n + 1) for q in range(n - p + 1)]
    return [(p, q, r) for p in range(n + 1) for q in range(n - p + 1) for r in range(n - p - q + 1)]


def walk_order(sd, n):
    return [fo.member_index(i) for i in walk_members(sd, n)]


def _level_norm2(variant, codim, idx):
    """norm2 applied to the member with index ``idx`` (length codim + 1) when codimension codim is complete
    (FIAT/expansions.py:251-266)."""
    d = codim + 1
    if variant is not None:
        shift = 1 if variant == "dual" else 0
        p = idx[-1] + shift
        al = 2 * (sum(idx[:-1]) + d * shift) - 1
        num, den = (2 * d + 1), 2 * d                      # (0.5 + d) / d
        if p > 0 and p + al > 0:
            num, den = num * (p + al) * (2 * p + al), den * p
        return num, den
    return 2 * sum(idx) + d, d


def _tail_norm(variant, sd, codim, idx, T):
    w = T(1)
    for c in range(codim, sd):
        num, den = _level_norm2(variant, c, idx[:c + 1])
        w = w * np.sqrt(T(num) / T(den))
    return w


def step_table(sd, n, variant, scale, T=np.float64):
    """(phi0, coef[nexp][3]): the steps m_dst = (A fa - B fb) m_cur - C fb^2 m_prv with every member in its final
    normalisation (csrc/plan.hpp build_program), coef[k] for the member at walk position k."""
    scale = T(scale)
    if variant == "bubble":
        scale = -scale
    members = walk_members(sd, n)
    pos = {m: k for k, m in enumerate(members)}
    coef = np.zeros((len(members), 3), dtype=T)
    beta = 1 if variant == "dual" else 0
    pad = lambda idx: tuple(idx) + (0,) * (sd - len(idx))     # noqa: E731
    lam = lambda codim, idx: _tail_norm(variant, sd, codim, pad(idx), T)     # noqa: E731
    for codim in range(sd):
        for sub in fo.simplex_lattice(0, n, codim):
            s = sum(sub)
            if variant == "bubble":
                alpha = 2 * s
                a = b = T(-0.5)
            else:
                alpha = 2 * s + codim + ((1 + codim) if variant == "dual" else 0)
                a = T(0.5) * (alpha + beta) + 1
                b = T(0.5) * (alpha - beta)
            ln = n - s
            lams = [lam(codim, sub + (i,)) for i in range(ln + 1)]
            coef[pos[pad(sub + (1,))]] = (a * lams[1] / lams[0], b * lams[1] / lams[0], 0)
            for i in range(1, ln):
                if variant == "bubble":
                    a, b, c = fo.integrated_jacobi_abc(T(alpha), T(beta), i)
                else:
                    a, b, c = fo.jacobi_abc(T(alpha), T(beta), i)
                coef[pos[pad(sub + (i + 1,))]] = (a * lams[i + 1] / lams[i], b * lams[i + 1] / lams[i], c * lams[i + 1] / lams[i - 1])
    phi0 = scale * _tail_norm(variant, sd, 0, (0,) * sd, T)
    return phi0, coef


def c0_matrix(sd, n):
    """T with C0_basis(phi) = T phi (FIAT/expansions.py:270-322)."""
    nexp = math.comb(n + sd, sd)
    return fo.c0_basis(sd, n, [np.eye(nexp)])[0]


def fold(sd, n, variant, coeffs):
    """A'[ndof][vdim][nexp] over the raw recurrence, columns in the order of the walk."""
    nexp = math.comb(n + sd, sd)
    C = np.asarray(coeffs, dtype=float).reshape(len(coeffs), -1, nexp)
    if variant == "bubble":
        C = C @ c0_matrix(sd, n)
    return np.ascontiguousarray(C[..., walk_order(sd, n)])


def cell_map(verts, T=np.float64):
    """(A, b): the simplex ``verts`` onto the (-1, 1)^sd simplex."""
    verts = np.asarray(verts, dtype=T)
    sd = verts.shape[1]
    E = (verts[1:] - verts[0]).T
    import edge_reference
    A = 2 * edge_reference._inverse(E)
    return A, -1 - A @ verts[0]


def _step(codim, sd, order, cur, prv, abc, fa, fb, dfa, dfb):
    """Jets are lists [v, g[sd], h[d1 <= d2]] of arrays over the points."""
    A, B, C = abc
    last = codim == sd - 1
    f = A * fa + B if last else A * fa - B * fb
    g = -C * np.ones_like(fa) if last else -C * (fb * fb)
    nw = [cur[0] * f + prv[0] * g]
    if order >= 1:
        df = [A * dfa[d] if last else A * dfa[d] - B * dfb[d] for d in range(sd)]
        dg = [0 * fa if last else (-2 * C) * fb * dfb[d] for d in range(sd)]
        nw.append([cur[1][d] * f + cur[0] * df[d] + prv[1][d] * g + prv[0] * dg[d] for d in range(sd)])
    if order >= 2:
        hs, h = [], 0
        for d1 in range(sd):
            for d2 in range(d1, sd):
                t = cur[2][h] * f + cur[1][d1] * df[d2] + cur[1][d2] * df[d1] + prv[2][h] * g
                if not last:
                    t = t + prv[1][d1] * dg[d2] + prv[1][d2] * dg[d1] + prv[0] * ((-2 * C) * dfb[d1] * dfb[d2])
                hs.append(t)
                h += 1
        nw.append(hs)
    return nw


def walk(sd, n, order, phi0, coef, w, A, b, pts):
    """acc (ntab, vdim, npts) = sum_k w[v][k] D^t member_k(pts): w (vdim, nexp) in the order of the walk, X = A x + b."""
    T = coef.dtype.type
    pts = np.asarray(pts, dtype=T)
    npts = len(pts)
    X = [pts @ A[i] + b[i] for i in range(sd)] + [np.full(npts, T(-1))] * 2
    J = [A[i] for i in range(sd)] + [np.zeros(sd, dtype=T)] * 2
    fa, fb, dfa, dfb = [], [], [], []
    for c in range(sd):
        if c == sd - 1:
            fb.append(np.full(npts, T(-1)))
            fa.append(X[c])
        else:
            fb.append(T(0.5) * (X[c + 1] + X[c + 2]))
            fa.append(X[c] + (fb[c] + 1))
        dfb.append([T(0) if c == sd - 1 else T(0.5) * (J[c + 1][d] + J[c + 2][d]) for d in range(sd)])
        dfa.append([J[c][d] + dfb[c][d] for d in range(sd)])
    nh = sd * (sd + 1) // 2
    ntab = math.comb(sd + order, sd)
    acc = np.zeros((ntab, w.shape[0], npts), dtype=T)
    zero = np.zeros(npts, dtype=T)
    const = [np.full(npts, T(phi0))] + ([[zero] * sd] if order >= 1 else []) + ([[zero] * nh] if order >= 2 else [])
    k = 0

    def accumulate(m):
        nonlocal k
        flat = [m[0]] + (list(m[1]) if order >= 1 else []) + (list(m[2]) if order >= 2 else [])
        for v in range(w.shape[0]):
            for t in range(ntab):
                acc[t, v] += w[v, k] * flat[t]
        k += 1

    def step(codim, cur, prv):
        return _step(codim, sd, order, cur, prv, coef[k], fa[codim], fb[codim], dfa[codim], dfb[codim])

    pc = pp = const
    for p in range(n + 1):
        if p > 0:
            pc, pp = step(0, pc, pp), pc
        if sd == 1:
            accumulate(pc)
            continue
        qc = qp = pc
        for q in range(n - p + 1):
            if q > 0:
                qc, qp = step(1, qc, qp), qc
            if sd == 2:
                accumulate(qc)
                continue
            rc = rp = qc
            for r in range(n - p - q + 1):
                if r > 0:
                    rc, rp = step(2, rc, rp), rc
                accumulate(rc)
    assert k == coef.shape[0]
    return acc


def piola_matrix(verts, cell, kind, T=np.float64):
    """J = E_req G with G = A0 / 2 of the element's own cell; 1: J^-T, 2: J / det J."""
    verts = np.asarray(verts, dtype=T)
    A0, _ = cell_map(cell, T)
    J = (verts[1:] - verts[0]).T @ (A0 / 2)
    import edge_reference
    sd = J.shape[0]
    Ji = edge_reference._inverse(J)
    det = J[0, 0] if sd == 1 else (J[0, 0] * J[1, 1] - J[0, 1] * J[1, 0] if sd == 2 else
                                    J[0, 0] * (J[1, 1] * J[2, 2] - J[1, 2] * J[2, 1]) - J[0, 1] * (J[1, 0] * J[2, 2] - J[1, 2] * J[2, 0])
                                    + J[0, 2] * (J[1, 0] * J[2, 1] - J[1, 1] * J[2, 0]))
    return Ji.T if kind == 1 else J / det


def evaluate(sd, n, variant, scale, coeffs, order, pts, dofs, cell=None, verts=None, mapping=0, value_shape=(), longdouble=False):
    """pts (npts, sd), dofs (nrhs, ndof) -> (ntab, nrhs, *value_shape, npts), one request.  ``cell``: the element's own cell
    (default: the UFC simplex); ``verts``: the request's cell (derivatives with respect to its coordinates); ``mapping`` 1 / 2:
    covariant / contravariant Piola map through ``verts``."""
    T = np.longdouble if longdouble else np.float64
    cell = fo.UFC_SIMPLEX[sd] if cell is None else np.asarray(cell, dtype=float)
    Ap = fold(sd, n, variant, coeffs).astype(T)                     # (ndof, vdim, nexp)
    phi0, coef = step_table(sd, n, variant, scale, T)
    A, b = cell_map(cell if verts is None else verts, T)
    dofs = np.asarray(dofs, dtype=T)
    out = []
    for c in dofs:
        w = np.zeros(Ap.shape[1:], dtype=T)
        for i in range(len(c)):                                      # the kernel's order: dofs ascending
            w += c[i] * Ap[i]
        acc = walk(sd, n, order, phi0, coef, w, A, b, pts)
        if mapping in (1, 2):
            acc = np.einsum("ab,tbp->tap", piola_matrix(verts, cell, mapping, T), acc)
        out.append(acc)
    res = np.stack(out, axis=1)                                      # (ntab, nrhs, vdim, npts)
    return res.reshape(res.shape[:2] + tuple(value_shape) + res.shape[-1:])


# ---- the item scheme (evaluate.hip make_plan), restated ---------------------------------------------------------------------

def _even(x):
    return (x + 1) & ~1


def lds_bytes(P, ndof, vn, image):
    return (_even(-(-P // RB) * RB * ndof) + _even(P * vn) + _even(image)) * 8


def plan(sd, n, order, vdim, ndof, npts, nrhs=1):
    """(P, chunks) of a shape."""
    vn = vdim * math.comb(n + sd, sd)
    if npts > 64:
        return 1, -(-npts // 64)
    per = math.comb(sd + order, sd) * vdim * npts
    P = 64 // npts
    while P > 1 and lds_bytes(P, ndof, vn, P * per) > LDS_BYTES:
        P -= 1
    return P, 1


def kernel_name(sd, n, order, vdim, ndof, npts, nrhs=1):
    P, chunks = plan(sd, n, order, vdim, ndof, npts, nrhs)
    return f"fxk::eval_kernel<{sd},{order},{vdim}> degree={n} P={P} chunks={chunks}"


# ---- the stand-alone walk program (tools/evaluate_walk_host.cpp) --------------------------------------------------------------

def write_walk_cases(path, cases):
    """``cases``: dicts with sd, n, variant (code), scale, order, vdim, mapping, cell (sd+1, sd), verts or None, coeffs
    (ndof, vdim, nexp), dofs (nrhs, ndof), pts (npts, sd), ref (ntab, nrhs, vdim, npts).  Plain text, one number per token."""
    with open(path, "w") as f:
        f.write(f"{len(cases)}\n")
        for c in cases:
            coeffs = np.asarray(c["coeffs"], dtype=float)
            ndof = coeffs.shape[0]
            dofs, pts = np.asarray(c["dofs"], dtype=float), np.asarray(c["pts"], dtype=float)
            has_verts = c.get("verts") is not None
            f.write(f"{c['sd']} {c['n']} {c['variant']} {c['order']} {c['vdim']} {c['mapping']} {ndof} {len(dofs)} {len(pts)} "
                    f"{int(has_verts)}\n")
            arrays = [[c["scale"]], c["cell"]] + ([c["verts"]] if has_verts else []) + [coeffs, dofs, pts, c["ref"]]
            for a in arrays:
                f.write(" ".join(float(x).hex() for x in np.asarray(a, dtype=float).ravel()) + "\n")
