"""Independent host references and helpers for the edge tests of the Bernstein (csrc/bernstein.hpp) and fused H(div) /
H(curl) (csrc/hdivcurl.hpp) kernels.  NumPy and the standard library only; imported by the tests, not a conftest.

- bernstein_reference: the Bernstein basis and its Cartesian derivatives from the definition, in np.longdouble, for the
  three sources of (lambda, G) of the kernel: the element's cell, per-request cells, one point set pushed to many cells;
  bernstein_exact: the same in fractions.Fraction from the exact binary values of the inputs (pins the long-double one).
- line_lagrange_reference / hdivcurl_reference: 1-D Lagrange factors by the product formula, and the signed row-major
  blocks of the H(div) / H(curl) tensor-product elements built from them.
- bern_route / hdc_route: what the launchers (bernstein.hip, hdivcurl.hip) decide for a request shape, with the constants
  parsed from the sources, so the edge shapes follow the launchers.
- guarded_out / check_guarded: an ``out`` view inside a NaN-filled buffer with guard regions on both sides."""
import itertools
import math
import os
import re
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fiat_amd", "csrc")
LD = np.longdouble

# ---------------------------------------------------------------------------------------------------------------------
# constants of the kernels and launchers


def _parse_constants(path, names):
    """``constexpr int NAME = <integer expression>`` (also in a comma-separated declaration) -> {NAME: value}."""
    text = open(path).read()
    out = {}
    for name in names:
        m = re.search(r"\b" + name + r"\s*=\s*([0-9][0-9\s*+()-]*)[,;]", text)
        if m is None:
            raise KeyError(f"{name} not found in {os.path.basename(path)}")
        expr = m.group(1)
        assert re.fullmatch(r"[0-9\s*+()-]+", expr)
        out[name] = int(eval(expr, {"__builtins__": {}}))      # digits and + - * ( ) only
    return out


def constants():
    c = {}
    c.update(_parse_constants(os.path.join(CSRC, "bernstein.hpp"), ["BERN_MAXN", "BERN_SPEC_MAXN", "BERN_IMAGE_BYTES"]))
    c.update(_parse_constants(os.path.join(CSRC, "bernstein.hip"), ["BERN_MAX_ORDER", "BERN_MAX_ORDER_CELLS"]))
    c.update(_parse_constants(os.path.join(CSRC, "hdivcurl.hpp"), ["HDC_IMAGE_BYTES"]))
    c.update(_parse_constants(os.path.join(CSRC, "hdivcurl.hip"), ["HDC_MAXK_QUAD", "HDC_MAXK_HEX", "HDC_MAX_ORDER"]))
    return c


C = constants()
BERN_SPEC_ORDER = 2            # compile-time instances: orders 0..2 (bernstein.hip launch_n)
MI355X_CU = 256                # compute units of one MI355X: the GPU tests read the device, the host coverage check uses this

# ---------------------------------------------------------------------------------------------------------------------
# multi-indices


def multi_indices(m, n):
    """Multi-indices of length m and sum n, first entry descending, then the rest in the same order (the order of mis)."""
    if m == 1:
        return [(n,)]
    return [(a,) + rest for a in range(n, -1, -1) for rest in multi_indices(m - 1, n - a)]


def jet(sd, order):
    """Cartesian derivative multi-indices of the tables, order by order."""
    return [a for o in range(order + 1) for a in multi_indices(sd, o)]


def ntables(sd, order):
    return math.comb(sd + order, sd)


# ---------------------------------------------------------------------------------------------------------------------
# Bernstein


def ufc_simplex(sd):
    return np.concatenate([np.zeros((1, sd)), np.eye(sd)])


def _inverse(A):
    """Inverse of (..., sd, sd) matrices, sd <= 3, by cofactors in the array's own dtype (np.linalg has no long double)."""
    sd = A.shape[-1]
    if sd == 1:
        return 1 / A
    if sd == 2:
        det = A[..., 0, 0] * A[..., 1, 1] - A[..., 0, 1] * A[..., 1, 0]
        adj = np.stack([np.stack([A[..., 1, 1], -A[..., 0, 1]], -1), np.stack([-A[..., 1, 0], A[..., 0, 0]], -1)], -2)
        return adj / det[..., None, None]
    cof = np.empty_like(A)
    for i in range(3):
        for j in range(3):
            r = [k for k in range(3) if k != i]
            c = [k for k in range(3) if k != j]
            minor = A[..., r[0], c[0]] * A[..., r[1], c[1]] - A[..., r[0], c[1]] * A[..., r[1], c[0]]
            cof[..., i, j] = (-1) ** (i + j) * minor
    det = (A[..., 0, :] * cof[..., 0, :]).sum(-1)
    return np.swapaxes(cof, -1, -2) / det[..., None, None]


def barycentric(verts, pts):
    """verts (..., sd+1, sd), pts (..., npts, sd) -> lam (..., npts, sd+1), G (..., sd+1, sd) = d lambda / dx, long double."""
    verts, pts = np.asarray(verts, dtype=LD), np.asarray(pts, dtype=LD)
    E = _inverse(np.swapaxes(verts[..., 1:, :] - verts[..., :1, :], -1, -2))       # rows: d lambda_i / dx, i = 1..sd
    lr = np.einsum("...id,...pd->...pi", E, pts - verts[..., None, 0, :])
    lam = np.concatenate([1 - lr.sum(-1, keepdims=True), lr], -1)
    G = np.concatenate([-E.sum(-2, keepdims=True), E], -2)
    return lam, G


def _chain(alpha, G, one):
    """d^alpha / dx^alpha = prod_d (sum_i G[i][d] d/dlambda_i)^alpha_d as {beta: coefficient}, by multinomial expansion."""
    sd = len(alpha)
    terms = {(0,) * (sd + 1): one}
    for d in range(sd):
        new = {}
        for g in multi_indices(sd + 1, alpha[d]):
            m = math.factorial(alpha[d])
            c = one
            for i, gi in enumerate(g):
                m //= math.factorial(gi)
                for _ in range(gi):
                    c = c * G[..., i, d]
            for beta, cb in terms.items():
                key = tuple(b + x for b, x in zip(beta, g))
                new[key] = new.get(key, 0) + cb * c * m
        terms = new
    return terms


def bernstein_reference(sd, n, order, pts, verts=None, shared=False, cell=None):
    """Tables (nreq, ntab, ndof, npts) of the degree-n Bernstein basis, dofs in mis(sd+1, n) order, tables in mis order,
    in np.longdouble.  pts (nreq, npts, sd) on the element's cell ``cell`` (default: the UFC simplex) or, with ``verts``
    (nreq, sd+1, sd), in the request's cell; ``shared``: pts (npts, sd) on ``cell``, derivatives from verts[r]."""
    cell = ufc_simplex(sd) if cell is None else np.asarray(cell, dtype=float)
    pts = np.asarray(pts, dtype=float)
    if shared:
        assert verts is not None and pts.ndim == 2
        lam, _ = barycentric(cell, pts)
        _, G = barycentric(verts, np.zeros((len(verts), 1, sd)))
        lam = np.broadcast_to(lam, (len(verts),) + lam.shape)
    elif verts is not None:
        lam, G = barycentric(verts, pts)
    else:
        lam, G = barycentric(cell, pts)
        G = np.broadcast_to(G, (len(pts),) + G.shape)
    nreq, npts = lam.shape[0], lam.shape[1]
    ks = np.array(multi_indices(sd + 1, n), dtype=int)                 # (ndof, sd+1)
    pw = np.ones((n + 1, sd + 1, nreq, npts), dtype=LD)               # pw[e, i] = lam_i ** e, repeated products
    lamT = np.moveaxis(lam, -1, 0)
    for e in range(1, n + 1):
        pw[e] = pw[e - 1] * lamT
    fact = np.array([math.factorial(j) for j in range(n + 1)], dtype=LD)
    dB = {}                                                             # d^beta B_k, (ndof, nreq, npts)

    def dbeta(beta):
        if beta not in dB:
            e = ks - np.array(beta)
            ok = (e >= 0).all(1)
            ec = np.maximum(e, 0)
            v = np.full((len(ks), nreq, npts), fact[n], dtype=LD) / np.prod(fact[ec], axis=1)[:, None, None]
            for i in range(sd + 1):
                v = v * pw[ec[:, i], i]
            v[~ok] = 0
            dB[beta] = v
        return dB[beta]
    out = np.zeros((nreq, ntables(sd, order), len(ks), npts), dtype=LD)
    for t, alpha in enumerate(jet(sd, order)):
        for beta, c in _chain(alpha, G, np.ones(nreq, dtype=LD)).items():
            out[:, t] += c[:, None, None] * np.moveaxis(dbeta(beta), 1, 0)
    return out


def _exact_bary(verts, x):
    """Exact barycentric coordinates and G of one simplex (lists of Fractions)."""
    sd = len(x)
    A = [[verts[c + 1][r] - verts[0][r] for c in range(sd)] for r in range(sd)]
    # Gauss-Jordan inverse over the rationals
    M = [row[:] + [Fraction(int(i == j)) for j in range(sd)] for i, row in enumerate(A)]
    for c in range(sd):
        p = next(r for r in range(c, sd) if M[r][c] != 0)
        M[c], M[p] = M[p], M[c]
        piv = M[c][c]
        M[c] = [v / piv for v in M[c]]
        for r in range(sd):
            if r != c and M[r][c] != 0:
                f = M[r][c]
                M[r] = [a - f * b for a, b in zip(M[r], M[c])]
    E = [row[sd:] for row in M]
    lr = [sum(E[i][d] * (x[d] - verts[0][d]) for d in range(sd)) for i in range(sd)]
    lam = [1 - sum(lr)] + lr
    G = [[-sum(E[i][d] for i in range(sd)) for d in range(sd)]] + [[E[i][d] for d in range(sd)] for i in range(sd)]
    return lam, G


def bernstein_exact(sd, n, order, x, verts=None, shared=False, cell=None):
    """One point x (sd,) -> (ntab, ndof) exact Fractions, from the exact binary values of the inputs (same modes as
    bernstein_reference; ``verts`` one cell (sd+1, sd))."""
    F = lambda a: [[Fraction(float(v)) for v in row] for row in np.asarray(a, dtype=float)]    # noqa: E731
    cell = F(ufc_simplex(sd) if cell is None else cell)
    xs = [Fraction(float(v)) for v in np.asarray(x, dtype=float)]
    if verts is None:
        lam, G = _exact_bary(cell, xs)
    elif shared:
        lam, _ = _exact_bary(cell, xs)
        _, G = _exact_bary(F(verts), xs)
    else:
        lam, G = _exact_bary(F(verts), xs)
    Garr = np.array(G, dtype=object)
    ks = multi_indices(sd + 1, n)
    out = []
    for alpha in jet(sd, order):
        row = []
        terms = _chain(alpha, Garr, Fraction(1))
        for k in ks:
            s = Fraction(0)
            for beta, c in terms.items():
                e = [a - b for a, b in zip(k, beta)]
                if min(e) < 0:
                    continue
                v = Fraction(math.factorial(n))
                for i, ei in enumerate(e):
                    v = v / math.factorial(ei) * lam[i] ** ei
                s += c * v
            row.append(s)
        out.append(row)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# 1-D Lagrange and H(div) / H(curl)


def line_lagrange_reference(nodes, x, order):
    """(order+1, nn, npts) long double: basis i = prod_{j != i} (x - x_j) / (x_i - x_j); the k-th derivative is
    k! sum over the k-subsets T of the other nodes of prod_{j not in T} (x - x_j), over the same denominator."""
    nodes = [LD(v) for v in np.asarray(nodes, dtype=float)]
    x = np.asarray(x, dtype=float).astype(LD)
    nn = len(nodes)
    out = np.zeros((order + 1, nn, len(x)), dtype=LD)
    for i in range(nn):
        others = [nodes[j] for j in range(nn) if j != i]
        den = LD(1)
        for xj in others:
            den = den * (nodes[i] - xj)
        for k in range(order + 1):
            if k > len(others):
                continue
            s = np.zeros(len(x), dtype=LD)
            for T in itertools.combinations(range(len(others)), k):
                p = np.ones(len(x), dtype=LD)
                for j in range(len(others)):
                    if j not in T:
                        p = p * (x - others[j])
                s = s + p
            out[k, i] = LD(math.factorial(k)) * s / den
    return out


def _kind(kind):
    return {"div": 0, "curl": 1, 0: 0, 1: 1}[kind]


def hdivcurl_reference(kind, C_nodes, D_nodes, offsets, signs, sd, order, pts):
    """pts (nreq, npts, sd) -> (nreq, ntab, ndof, sd, npts) long double.  Block c (offsets[c] >= 0): dofs
    offsets[c] + row-major (i0, i1[, i2]) of prod_d F_d, F_d = C where (d == c) for H(div) (kind 0 / "div") and where
    (d != c) for H(curl), else D; sign signs[c]; component c only, every other component exactly zero."""
    kind = _kind(kind)
    pts = np.asarray(pts, dtype=float)
    nreq, npts = pts.shape[0], pts.shape[1]
    flat = pts.reshape(-1, sd)
    TC = [line_lagrange_reference(C_nodes, flat[:, d], order) for d in range(sd)]
    TD = [line_lagrange_reference(D_nodes, flat[:, d], order) for d in range(sd)]
    K = len(D_nodes)
    assert len(C_nodes) == K + 1
    nb = (K + 1) * K ** (sd - 1) if kind == 0 else K * (K + 1) ** (sd - 1)
    nblocks = sum(1 for o in offsets if o >= 0)
    alphas = jet(sd, order)
    out = np.zeros((len(alphas), nb * nblocks, sd, nreq * npts), dtype=LD)
    for c in range(sd):
        if offsets[c] < 0:
            continue
        fac = [TC[d] if (d == c) == (kind == 0) else TD[d] for d in range(sd)]
        for t, a in enumerate(alphas):
            prod = fac[0][a[0]]
            for d in range(1, sd):
                prod = (prod[:, None, :] * fac[d][a[d]][None, :, :]).reshape(-1, nreq * npts)
            out[t, offsets[c]:offsets[c] + nb, c] = signs[c] * prod
    return np.moveaxis(out.reshape(len(alphas), nb * nblocks, sd, nreq, npts), 3, 0)


def grid_points(grid):
    """Grid input (nreq, sd, q) -> points (nreq, q**sd, sd), row-major (j0, j1[, j2]) as the kernel reads them."""
    grid = np.asarray(grid)
    nreq, sd, q = grid.shape
    idx = np.stack(np.meshgrid(*[np.arange(q)] * sd, indexing="ij"), -1).reshape(-1, sd)
    return np.stack([grid[:, d, idx[:, d]] for d in range(sd)], -1)


# ---------------------------------------------------------------------------------------------------------------------
# route mirrors


def bern_coef_size(sd, order):
    return sum(math.comb(o + sd - 1, sd - 1) * math.comb(o + sd, sd) for o in range(order + 1))


def _items(P, npts, reqsize, nreq, image, gridcap, offset=0):
    nitems = -(-nreq // P)
    last = nreq - (nitems - 1) * P
    copies = set()
    if image:
        # item i starts offset + i * P * reqsize doubles past a 16-byte boundary; the image leaves by flush_block when the
        # item's size is even and its base 16-byte aligned, else by the scalar copy loop
        for i in ({0, 1, nitems - 1} & set(range(nitems))):
            total = (last if i == nitems - 1 else P) * reqsize
            copies.add("flush" if total % 2 == 0 and (offset + i * P * reqsize) % 2 == 0 else "scalar")
    return {"P": P, "nitems": nitems, "last": last, "last_partial": last < P, "reqsize": reqsize,
            "item_bytes": P * reqsize * 8, "image": bool(image), "gridcap": gridcap, "grid": max(1, min(nitems, gridcap)),
            "stride": nitems > gridcap, "chunks": -(-P * npts // 64), "partial_chunk": P == 1 and npts > 64 and npts % 64 != 0,
            "copies": copies}


def bern_route(sd, n, order, npts, cells, nreq, num_cu, offset=0):
    """What bernstein.hip decides: spec (compile-time instance) or generic, P, image or stream, items and grid."""
    ntab, ndof = ntables(sd, order), math.comb(n + sd, sd)
    reqsize = ntab * ndof * npts
    P = 64 // npts if npts <= 64 else 1
    spec = n <= C["BERN_SPEC_MAXN"] and order <= BERN_SPEC_ORDER
    if spec:
        image = P * reqsize * 8 <= C["BERN_IMAGE_BYTES"]
        gridcap = num_cu * 64
    else:
        csize = bern_coef_size(sd, order)
        if cells:
            P = max(1, min(P, C["BERN_IMAGE_BYTES"] // (csize * 8)))
        image = False
        gridcap = num_cu * 8
    r = _items(P, npts, reqsize, nreq, image, gridcap, offset)
    r.update(spec=spec, instance=("spec", sd, n, order) if spec else ("generic", sd), p_by_lds=not spec and cells and P < (64 // npts if npts <= 64 else 1))
    return r


def hdc_nb(sd, K, kind):
    return (K + 1) * K ** (sd - 1) if _kind(kind) == 0 else K * (K + 1) ** (sd - 1)


def hdc_route(sd, K, order, kind, nblocks, npts, nreq, num_cu, grid=False, offset=0):
    """What hdivcurl.hip decides for the fused kernel (npts = q**sd with grid input)."""
    ndof = nblocks * hdc_nb(sd, K, kind)
    reqsize = ntables(sd, order) * ndof * sd * npts
    P = 64 // npts if npts <= 64 else 1
    image = P * reqsize * 8 <= C["HDC_IMAGE_BYTES"]
    r = _items(P, npts, reqsize, nreq, image, num_cu * 64, offset)
    r.update(instance=(_kind(kind), sd, K, order, bool(grid)), ndof=ndof)
    return r


def hdc_instances():
    """Every fused instance: (kind, sd, K, order, grid)."""
    return [(kind, sd, K, order, grid) for kind in (0, 1) for sd in (2, 3)
            for K in range(1, (C["HDC_MAXK_QUAD"] if sd == 2 else C["HDC_MAXK_HEX"]) + 1)
            for order in range(C["HDC_MAX_ORDER"] + 1) for grid in (False, True)]


def bern_spec_instances():
    return [(sd, n, order) for sd in (1, 2, 3) for n in range(C["BERN_SPEC_MAXN"] + 1) for order in range(BERN_SPEC_ORDER + 1)]


def sample_requests(nreq, P, nitems_per_trip=None, k=24, seed=0):
    """A seeded sample of request indices with the first and last request and both sides of every item boundary that a
    small sample can hold (item boundaries near the start, the end and every grid-stride trip)."""
    rng = np.random.default_rng(seed)
    s = {0, nreq - 1}
    bounds = [P, 2 * P, nreq - nreq % P if nreq % P else nreq - P]
    if nitems_per_trip:
        trip = nitems_per_trip * P
        bounds += list(range(trip, nreq, trip))
    for b in bounds:
        s.update(x for x in (b - 1, b) if 0 <= x < nreq)
    s.update(int(x) for x in rng.choice(nreq, min(k, nreq), replace=False))
    return np.array(sorted(s))


# ---------------------------------------------------------------------------------------------------------------------
# guarded output

GUARD = 64                                  # doubles of guard on each side (a multiple of 16: keeps the 128-byte phase)
FILL_BITS = 0x7FF4DEADBEEF0A5A              # a quiet-bit-clear NaN with a payload no arithmetic produces
OFFSETS = (0, 1, 7, 8)                      # doubles: aligned, 8 mod 16 bytes, 56 bytes into a line, the middle of a line


def guarded_out(shape, offset_doubles, device):
    """(buf, out): buf filled with the FILL_BITS NaN; out a contiguous view of ``shape`` starting GUARD + offset doubles
    into buf (an allocation that starts on a 128-byte line), with at least GUARD doubles of guard after it."""
    import torch
    n = int(np.prod(shape))
    buf = torch.full((GUARD + offset_doubles + n + GUARD,), FILL_BITS, dtype=torch.int64, device=device).view(torch.float64)
    assert buf.data_ptr() % 128 == 0
    out = buf[GUARD + offset_doubles:GUARD + offset_doubles + n].view(shape)
    assert out.is_contiguous() and (out.data_ptr() - buf.data_ptr()) // 8 == GUARD + offset_doubles
    return buf, out


def check_guarded(buf, out):
    """Both guards bit-identical to the fill, no entry of out left at the fill, no NaN in out."""
    import torch
    start = (out.data_ptr() - buf.data_ptr()) // 8
    end = start + out.numel()
    bits = buf.view(torch.int64)
    assert bool((bits[:start] == FILL_BITS).all()), "a store before out"
    assert bool((bits[end:] == FILL_BITS).all()), "a store after out"
    body = bits[start:end]
    unwritten = int((body == FILL_BITS).sum())
    assert unwritten == 0, f"{unwritten} entries of out never written"
    assert not bool(torch.isnan(out).any()), "NaN in out"


def launched(call):
    """Names of the device kernels that ``call`` launches (the profiler's device-side records)."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        call()
        torch.cuda.synchronize()
    return {e.name for e in prof.events() if e.device_type.name == "CUDA" and "Memcpy" not in e.name and "Memset" not in e.name}


def launched_records(call, trace_path):
    """The device kernels that ``call`` launches, with where and when they ran: a list of
    ``{"name", "start", "end" (microseconds on the device's clock), "stream", "grid" (workgroups)}`` from the profiler's
    device-side records (its trace file, written to ``trace_path``: the Python event objects carry neither stream nor grid)."""
    import json
    import torch
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        call()
        torch.cuda.synchronize()
    prof.export_chrome_trace(str(trace_path))
    with open(trace_path) as f:
        events = json.load(f)["traceEvents"]
    out = []
    for e in events:
        if e.get("cat") != "kernel":
            continue
        args = e.get("args", {})
        out.append({"name": e["name"], "start": float(e["ts"]), "end": float(e["ts"]) + float(e["dur"]),
                    "stream": args.get("stream"), "grid": int(args["grid"][0])})
    return sorted(out, key=lambda r: r["start"])


def compare(call, shape, device):
    """call(out) for a fresh out and for guarded views at every offset."""
    import torch
    fresh = torch.empty(shape, dtype=torch.float64, device=device)
    call(fresh)
    torch.cuda.synchronize()
    for off in OFFSETS:
        buf, out = guarded_out(shape, off, device)
        call(out)
        torch.cuda.synchronize()
        check_guarded(buf, out)
        assert torch.equal(out, fresh), off
    return fresh


def rel_to_exact(approx, exact):
    """max |approx - exact| / max(1, max |exact|) over nested lists of long doubles and Fractions, computed exactly."""
    a = np.asarray(approx, dtype=LD).ravel()
    e = [x for row in exact for x in row] if isinstance(exact[0], list) else list(exact)
    assert len(a) == len(e)
    err = max(abs(Fraction(*v.as_integer_ratio()) - x) for v, x in zip(a, e))
    return float(err / max(Fraction(1), max(abs(x) for x in e)))


# ---------------------------------------------------------------------------------------------------------------------
# shape lists of the GPU edge tests (tests/test_gpu_bernstein_edges.py, test_gpu_hdivcurl_edges.py,
# test_gpu_guarded_out.py), kept here so that tests/test_edge_reference_host.py runs the same lists through the mirrors

POINT_COUNTS = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200]
IMAGE_SEARCH_MAX_POINTS = 4096          # point counts searched for the image edge (P = 1 beyond 64: one request in chunks)


def nreq_list(P):
    return sorted({x for x in (1, P - 1, P, P + 1, 3 * P + 2) if x >= 1})


def simplex_points(rng, shape, sd, lo=0.0):
    """Points of the UFC simplex (lo < 0: barycentric coordinates down to lo, outside the cell)."""
    e = rng.exponential(size=shape + (sd + 1,))
    lam = e / e.sum(-1, keepdims=True)
    lam = lam * (1 - (sd + 1) * lo) + lo
    return lam[..., 1:].copy()


def random_cells(rng, nreq, sd, flip=True):
    """Random affine images of the UFC simplex, every third one negatively oriented."""
    A = np.eye(sd) + 0.3 * rng.standard_normal((nreq, sd, sd))
    if flip:
        A[::3, :, 0] *= -1.0
    return np.einsum("vd,red->rve", ufc_simplex(sd), A) + rng.standard_normal((nreq, 1, sd))


def _image_edge(item_bytes, shapes, limit):
    """Shapes at the LDS image limit: exactly ``limit`` bytes (the two with the fewest points), each of them with one point
    more (above the limit, a partial last chunk), the smallest item above the limit; and among the shapes of at most 64
    points (P whole requests an item) the two largest items at or below the limit and the two smallest above it."""
    sized = [(item_bytes(s), s) for s in shapes]
    exact = sorted((s for b, s in sized if b == limit), key=lambda s: (s[-1], s))[:2]
    out = exact + [s[:-1] + (s[-1] + 1,) for s in exact if item_bytes(s[:-1] + (s[-1] + 1,)) > limit]
    out.append(min((b, s) for b, s in sized if b > limit)[1])
    small = [(b, s) for b, s in sized if s[-1] <= 64]
    out += [s for b, s in sorted((x for x in small if x[0] <= limit), key=lambda x: (-x[0], x[1]))[:2]]
    out += [s for b, s in sorted(x for x in small if x[0] > limit)[:2]]
    return list(dict.fromkeys(out))


# Bernstein: (sd, n, order, npts, nreq), the 63 compile-time instances at 7 points (P = 9: one idle lane), nreq = 2P + 1
BERN_CENSUS = [(sd, n, o, 7, 2 * 9 + 1) for sd, n, o in bern_spec_instances()]
# generic instance on the element's cell: (sd, n, order, npts, nreq)
BERN_GENERIC_OWN = [(sd, n, o, 3, 2 * 21 + 1) for sd in (1, 2, 3) for n in (7, 11, 16) for o in (0, 3, 5, 8) if o <= n] + \
                   [(sd, n, n, 5, 2 * 12 + 1) for sd in (1, 2, 3) for n in (3, 4)]
# generic instance with cells (mode "cells" / "shared"), orders 3-4; 1-4 points on tetrahedra at order 4: P set by the LDS
BERN_GENERIC_CELLS = [(sd, n, o, npts, mode) for sd in (1, 2, 3) for n, o in ((3, 3), (5, 4)) for npts in (1, 4, 9)
                      for mode in ("cells", "shared")] + [(3, 4, 4, npts, "cells") for npts in (2, 3)]
BERN_POINT_SHAPES = [(2, 3, 1), (2, 8, 2)]         # (sd, n, order): one compile-time, one generic
# (sd, n, order, npts) of the compile-time instances at BERN_IMAGE_BYTES (only single requests of more than 64 points meet
# it exactly)
BERN_IMAGE_EDGE = _image_edge(lambda s: bern_route(*s, False, 1, MI355X_CU)["item_bytes"],
                              [(sd, n, o, p) for sd, n, o in bern_spec_instances() for p in range(1, IMAGE_SEARCH_MAX_POINTS + 1)],
                              C["BERN_IMAGE_BYTES"])
# odd item totals: odd request size with odd P (every item odd, every second one off a 16-byte boundary) and with even P
# (whole items even and aligned, the partial last item odd)
BERN_ODD_SHAPES = [(1, 0, 0, 7), (1, 2, 0, 5), (2, 1, 0, 3), (1, 0, 0, 21), (1, 2, 0, 7)]


def bern_grid_stride_cases(num_cu):
    """(sd, n, order, npts, mode, nreq): items exceed the grid cap at least twice."""
    out = []
    for sd, n, o, npts, mode in [(1, 1, 0, 8, "own"), (1, 7, 3, 16, "own"), (1, 7, 3, 8, "cells")]:
        r = bern_route(sd, n, o, npts, mode != "own", 1, num_cu)
        out.append((sd, n, o, npts, mode, r["P"] * (2 * r["gridcap"] + 3) - 1))
    return out


def hdc_name(kind, sd, K, single=False):
    """Fixture-style name of the enriched family (or, ``single``, of one summand) of a fused instance."""
    if single:
        return {(0, 2): "sdiv", (1, 2): "scurl", (0, 3): "sdivz", (1, 3): "scurlz"}[(kind, sd)] + f"{K}d0"
    return {(0, 2): "rtcf", (1, 2): "rtce", (0, 3): "ncf", (1, 3): "nce"}[(kind, sd)] + f"{K}d0"


def hdc_descriptor_of(name):
    """(kind, sd, K, nblocks) of a fused element name, without building it."""
    fam = name[:-3]
    K = int(name[-3])
    kind = 0 if fam in ("rtcf", "ncf", "sdiv", "sdivz") else 1
    sd = 3 if fam in ("ncf", "nce", "sdivz", "scurlz") else 2
    nblocks = 1 if fam.startswith("s") else sd
    return kind, sd, K, nblocks


def hdc_route_of(name, order, npts, nreq, num_cu=MI355X_CU, grid=False, offset=0):
    kind, sd, K, nb = hdc_descriptor_of(name)
    return hdc_route(sd, K, order, kind, nb, npts, nreq, num_cu, grid=grid, offset=offset)


# H(div) / H(curl): (element name, order, grid, npts or q, nreq): the 84 fused instances on the enriched families, 9 points
# (P = 7, one idle lane) or q = 3 (hexahedra: 27 points, P = 2), nreq = 2P + 1; plus the single summands (one block, a
# nonzero offset on the hexahedra)
HDC_CENSUS = [(hdc_name(kind, sd, K), order, grid, 3 if grid else 9, 2 * (64 // (9 if sd == 2 or not grid else 27)) + 1)
              for kind, sd, K, order, grid in hdc_instances()] + \
             [(hdc_name(kind, sd, 2, True), order, grid, 3 if grid else 9, 15) for kind in (0, 1) for sd in (2, 3)
              for order in (0, 2) for grid in (False, True)]
HDC_POINT_ELEMENTS = [("rtcf2d0", 2), ("nce1d0", 1)]
HDC_GRID_Q = {2: [1, 7, 8, 9, 11, 64], 3: [1, 3, 4, 5, 7]}
HDC_GRID_ELEMENTS = {2: ("rtce2d0", 1), 3: ("ncf1d0", 1)}
# (name, order, npts) at HDC_IMAGE_BYTES, as for Bernstein
HDC_IMAGE_EDGE = _image_edge(lambda s: hdc_route_of(*s, 1)["item_bytes"],
                             [(hdc_name(kind, sd, K), order, p) for kind, sd, K, order, grid in hdc_instances() if not grid
                              for p in range(1, IMAGE_SEARCH_MAX_POINTS + 1)],
                             C["HDC_IMAGE_BYTES"])
# (name, order, npts, offset in doubles): every block has (K+1) K^(sd-1) or K (K+1)^(sd-1) dofs, an even number, so every
# item is an even number of doubles and the scalar copy loop runs only for an out that starts off a 16-byte boundary
HDC_OFFSET_SHAPES = [("sdiv1d0", 0, 1, 1), ("rtcf1d0", 0, 7, 7), ("scurlz1d0", 1, 9, 1), ("nce1d0", 0, 33, 7), ("rtcf2d0", 2, 64, 1)]


def hdc_grid_stride_cases(num_cu):
    """(name, order, npts, nreq): items exceed the grid cap at least twice."""
    out = []
    for name, order, npts in [("rtcf1d0", 0, 16), ("ncf1d0", 0, 9)]:
        r = hdc_route_of(name, order, npts, 1, num_cu)
        out.append((name, order, npts, r["P"] * (2 * r["gridcap"] + 3) - 1))
    return out


# guarded outputs of the two kernels: (sd, n, order, npts, nreq, mode) -- compile-time instance with image, with stream,
# generic; own cell, cells, shared -- and (name, order, grid, npts or q, nreq) of the fused kernel, image and stream
GUARD_BERN = [(2, 3, 1, 9, 20, "own"), (3, 6, 2, 64, 3, "own"), (3, 5, 2, 7, 19, "own"), (2, 9, 3, 11, 13, "own"),
              (3, 4, 3, 5, 30, "cells"), (2, 2, 1, 13, 9, "shared")]
GUARD_HDC = [("rtcf2d0", 1, False, 9, 15), ("nce2d0", 2, False, 33, 4), ("ncf1d0", 1, True, 3, 5), ("rtce3d0", 2, True, 11, 2),
             ("rtcf4d0", 2, False, 65, 3)]


# ---------------------------------------------------------------------------------------------------------------------
# the H(div) / H(curl) fixture


def hdivcurl_fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "hdivcurl.npz"))


def fixture_descriptor(name, fixture=None):
    """(sd, kind, C nodes, D nodes, offsets, signs) of a fixture element without building it (building an element needs
    the device, so the GPU tests pin hdivcurl.fused_descriptor against this): the nodes recorded with the fixture, each
    block's first dof read off the value table, the sign rule of the Hdiv / Hcurl wrappers (-1 on component 0 of H(div),
    else +1)."""
    GH = hdivcurl_fixture() if fixture is None else fixture
    tab, pts = GH[f"{name}_tab"], GH[f"{name}_pts"]
    sd = pts.shape[1]
    kind = 0 if name.startswith(("rtcf", "ncf", "sdiv")) else 1
    comps = [int(np.argmax(np.abs(tab[0, i]).max(-1))) for i in range(tab.shape[1])]
    offsets = tuple(comps.index(c) if c in comps else -1 for c in range(sd))
    signs = tuple((-1 if kind == 0 and c == 0 else 1) if offsets[c] >= 0 else 0 for c in range(sd))
    return sd, kind, GH[f"{name}_c"], GH[f"{name}_d"], offsets, signs


def rel(got, ref):
    """The suite's norm max|got - ref| / max(1, max|ref|) over whole arrays."""
    got, ref = np.asarray(got, dtype=float), np.asarray(ref, dtype=float)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return np.abs(got - ref).max() / max(1.0, np.abs(ref).max())
