"""TEST INFRASTRUCTURE -- ``evaluate_batch`` on per-request cells: the shared case lists and a closed-form oracle.  The host
test (tests/test_evaluate_host.py) and the GPU test (tests/test_gpu_evaluate_cells.py) build the same batches from here.

The oracle is the reference's own order-2 contraction on its reference cell (``{name}_ref`` of tests/golden/evaluate.npz, taken
at the points ``{name}_pts``: 12 on the interval, 13 on the triangle, 14 on the tetrahedron) pushed through closed formulas: for the affine cell x = B X + v0 the chain rule of the
derivatives through B^-1 (``make_golden_evaluate.chain``) and then J^-T or J / det J (``make_golden_evaluate.pushed``).  Nothing
of the kernel's recurrence, cell map, collapsed-coordinate gradients or Piola code is in it.  Orders 0 and 1 are the leading
1 and 1 + sd tables.

Conditions on the inputs (stated, not measured): cells from ``edge_reference.random_cells`` with fixed seeds, a cell dropped
from the draw when cond_2(B) > COND_MAX = 8, at most 10 % of a draw dropped, both orientations among the kept cells.  With
them the float64 restatement of elements built on the UFC cell stays a factor 50 inside the standing 1e-12 on values and
nearly 1e4 inside 1e-10 on derivatives (tests/test_evaluate_host.py prints the figure of every batch)."""
import math
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.join(HERE, "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import edge_reference as E  # noqa: E402
import evaluate_reference as R  # noqa: E402
import make_golden_evaluate as M  # noqa: E402

G = np.load(os.path.join(HERE, "golden", "evaluate.npz"))
STANDING = (1e-12, 1e-10)
FUSED = [n for n in M.CASES if n not in M.GENERAL_ONLY]
MAPPING_NAMES = {0: "affine", 1: "covariant piola", 2: "contravariant piola"}
COND_MAX = 8.0
NFIX = 13                                  # points of a request of the family cases


def meta(name):
    n, ndof, sd, vdim, mapping, variant = (int(x) for x in G[f"{name}_meta"])
    return {"n": n, "ndof": ndof, "sd": sd, "vdim": vdim, "mapping": mapping, "variant": variant,
            "scale": float(G[f"{name}_scale"][0]), "value_shape": tuple(G[f"{name}_ref"].shape[2:-1])}


def instance_of(name, order):
    m = meta(name)
    return (m["sd"], order, m["vdim"])


def plan(name, order, npts):
    """(P, chunks) of the launcher for this element and shape (evaluate_reference.plan restates evaluate.hip make_plan)."""
    m = meta(name)
    return R.plan(m["sd"], m["n"], order, m["vdim"], m["ndof"], npts)


def per_item(name, order, npts):
    P, chunks = plan(name, order, npts)
    return P if chunks == 1 else 1


def edge_matrices(verts):
    """B (nreq, sd, sd) with x = B X + v0: the columns are the edges v_i - v_0."""
    verts = np.asarray(verts, dtype=float)
    return np.swapaxes(verts[:, 1:] - verts[:, :1], 1, 2)


def cells(rng, nreq, sd, cond_max=COND_MAX):
    """``nreq`` cells of a seeded draw of ``random_cells`` (every third one negatively oriented), those with
    cond_2(B) > COND_MAX dropped.  At most 10 % of the draw may be dropped and the kept cells hold both orientations."""
    draw = max(200, nreq + nreq // 4 + 8)      # large enough that the 10 % bound is a statement about the distribution
    verts = E.random_cells(rng, draw, sd)
    B = edge_matrices(verts)
    keep = np.linalg.cond(B, 2) <= cond_max
    assert int((~keep).sum()) * 10 <= draw, (int((~keep).sum()), draw)
    kept = verts[keep]
    det = np.linalg.det(B[keep])
    assert (det > 0).any() and (det < 0).any()
    assert len(kept) >= nreq
    if nreq >= 4:                           # the requests themselves, not only the draw
        assert (det[:nreq] > 0).any() and (det[:nreq] < 0).any()
    return np.ascontiguousarray(kept[:nreq])


def point_indices(rng, nreq, npts, nfix):
    """Per request: a permutation prefix of the ``nfix`` fixture points (12 on the interval, 13 on the triangle, 14 on the
    tetrahedron), or above that a sample with replacement."""
    if npts <= nfix:
        return np.stack([rng.permutation(nfix)[:npts] for _ in range(nreq)]).reshape(nreq, npts)
    return rng.integers(0, nfix, size=(nreq, npts))


def rhs_of(r, j):
    """(fixture dof vector, exact scale) of right-hand side j of request r: the three vectors rotated by r, scaled by
    2^-(r % 4); right-hand sides beyond the third repeat them with a further 2^-(j // 3)."""
    return (r + j) % 3, 2.0 ** -(r % 4) * 2.0 ** -(j // 3)


def seed_of(name, order, npts, nreq, nrhs):
    return zlib.crc32(f"{name} {order} {npts} {nreq} {nrhs}".encode())


def batch(name, order, npts, nreq, nrhs=1, seed=None, own=False, cond_max=COND_MAX):
    """The inputs and the expected result of one call: ``pts`` (nreq, npts, sd) in the requests' cells, ``verts``
    (nreq, sd + 1, sd), ``dofs`` (nreq, nrhs, ndof), ``ref`` (nreq, ntab, nrhs, *value_shape, npts), ``B`` and ``idx``.
    ``own``: the element is built on the fixture's skewed cell ``{name}_verts`` (affine families); the oracle is then the
    reference's element built on that cell, ``{name}_pref``, chained through the map of that cell onto the request's."""
    m = meta(name)
    sd = m["sd"]
    rng = np.random.default_rng(seed_of(name, order, npts, nreq, nrhs) if seed is None else seed)
    verts = cells(rng, nreq, sd, cond_max)
    B = edge_matrices(verts)
    X = G[f"{name}_pts"]
    idx = point_indices(rng, nreq, npts, len(X))
    pts = np.einsum("rde,rpe->rpd", B, X[idx]) + verts[:, :1]
    base = G[f"{name}_dofs"]
    sel = np.array([[rhs_of(r, j)[0] for j in range(nrhs)] for r in range(nreq)]).reshape(nreq, nrhs)
    scl = np.array([[rhs_of(r, j)[1] for j in range(nrhs)] for r in range(nreq)]).reshape(nreq, nrhs)
    dofs = np.ascontiguousarray(base[sel] * scl[..., None])
    ntab = math.comb(sd + order, sd)
    mapping = MAPPING_NAMES[m["mapping"]]
    if own:
        assert mapping == "affine"
        table = G[f"{name}_pref"]
        B0inv = np.linalg.inv(edge_matrices(G[f"{name}_verts"][None])[0])
    else:
        table = G[f"{name}_ref"]
    ref = []
    for r in range(nreq):
        t = table[:, sel[r]][..., idx[r]]                                  # (ntab2, nrhs, *value_shape, npts)
        t = t * scl[r].reshape((1, nrhs) + (1,) * (t.ndim - 2))           # powers of two: exact
        Br = B[r] @ B0inv if own else B[r]
        ref.append(M.pushed(M.chain(t, Br), Br, mapping)[:ntab])
    return {"pts": np.ascontiguousarray(pts), "verts": verts, "dofs": dofs, "ref": np.stack(ref), "B": B, "idx": idx}


def restated(name, order, b, longdouble=False, own=False, coeffs=None):
    """The NumPy restatement of the kernel (evaluate_reference.evaluate) on a batch, request by request."""
    m = meta(name)
    kw = dict(cell=G[f"{name}_verts"]) if own else {}
    coeffs = G[f"{name}_coeffs"] if coeffs is None else coeffs
    return np.stack([R.evaluate(m["sd"], m["n"], R.VARIANTS[m["variant"]], m["scale"], coeffs, order, b["pts"][r], b["dofs"][r],
                                verts=b["verts"][r], mapping=m["mapping"], value_shape=m["value_shape"], longdouble=longdouble, **kw)
                     for r in range(len(b["pts"]))])


def worst(got, ref):
    """(values, derivatives): the worst request of a batch in the project's norm, every request compared."""
    got, ref = np.asarray(got, dtype=float), np.asarray(ref, dtype=float)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    e = [R.errors(got[r], ref[r]) for r in range(len(ref))]
    return (max(x[0] for x in e), max(x[1] for x in e)) if e else (0.0, 0.0)


# ---- the case lists: (name, order, npts, nreq, nrhs) ------------------------------------------------------------------------

# every family: order 2, the 13 points permuted, three whole items and a partial one
FAMILY_CASES = [(name, M.ORDER, NFIX, 3 * per_item(name, M.ORDER, NFIX) + 2, 1) for name in FUSED]
# every instance: one element per (sd, vdim) and one contravariant element per dimension at orders 0 and 1 (order 2: above)
INSTANCE_ELEMENTS = ("leg_int3", "lag_tri3", "ned_tri3", "lag_tet3", "ned_tet2", "rt_tri3", "rt_tet2")
INSTANCE_CASES = [(name, order, 7, 13, 1) for name in INSTANCE_ELEMENTS for order in (0, 1)]
# item shapes: one lane per request (P set by the LDS budget), a few points, the wave boundary, chunks with a partial last one
SHAPE_ELEMENTS = ("lag_tet3", "ned_tri3", "rt_tet2")
SHAPE_POINTS = (1, 5, 64, 65, 130)
SHAPE_CASES = [(name, M.ORDER, npts, nreq, 1) for name in SHAPE_ELEMENTS for npts in SHAPE_POINTS
               for nreq in E.nreq_list(per_item(name, M.ORDER, npts))]
# right-hand sides: whole requests with P = 2, chunks, P = 7; built with 8 right-hand sides, of which 1 and 3 are prefixes
RHS_CASES = [("lag_tet3", M.ORDER, 23, 5, 8), ("rt_tet2", M.ORDER, 70, 3, 8), ("ned_tri3", M.ORDER, 9, 16, 8)]
# output alignment: odd request size and odd P (item starts alternate in parity), and one chunked shape
ALIGN_CASES = [("lag_tri2", 0, 7, 20, 1), ("lag_tri2", 1, 70, 3, 1)]
# elements built on their own skewed cell, per-request cells on top
OWN_ELEMENTS = ("lag_tri3", "lag_tet4", "dg_tet3", "leg_int3")
OWN_CASES = [(name, order, 7, 13, 1) for name in OWN_ELEMENTS for order in (0, 1, 2)]

ALL_CASES = FAMILY_CASES + INSTANCE_CASES + SHAPE_CASES + RHS_CASES + ALIGN_CASES


def instances_with_cells():
    """The compile-time instances (sd, order, vdim) that the case lists run with per-request cells."""
    return {instance_of(c[0], c[1]) for c in ALL_CASES + OWN_CASES}


def walk_cell_cases(per_class=3):
    """Cases for tools/evaluate_walk_host.cpp: per (sd, vdim, mapping) ``per_class`` random cells of a batch, a negatively
    oriented one among them, at order 2 (the program runs orders 0..2 of each); and per dimension one element built on the
    fixture's own skewed cell with a request's cell on top."""
    out = []
    classes = {}
    for name in FUSED:
        m = meta(name)
        classes.setdefault((m["sd"], m["vdim"], m["mapping"]), name)
    for key, name in sorted(classes.items()):
        m = meta(name)
        b = batch(name, M.ORDER, 7, 8, nrhs=3)
        det = np.linalg.det(b["B"])
        picks = [int(np.argmax(det < 0))] + [r for r in range(8) if det[r] > 0][:per_class - 1]
        assert det[picks[0]] < 0 and len(picks) == per_class
        for r in picks:
            out.append(dict(sd=m["sd"], n=m["n"], variant=m["variant"], scale=m["scale"], order=M.ORDER, vdim=m["vdim"],
                            mapping=m["mapping"], cell=R.fo.UFC_SIMPLEX[m["sd"]], verts=b["verts"][r],
                            coeffs=G[f"{name}_coeffs"].reshape(m["ndof"], m["vdim"], -1), dofs=b["dofs"][r], pts=b["pts"][r],
                            ref=b["ref"][r]))
    for name in ("leg_int3", "lag_tri3", "lag_tet4"):
        m = meta(name)
        base = dict(sd=m["sd"], n=m["n"], variant=m["variant"], scale=m["scale"], order=M.ORDER, vdim=m["vdim"], mapping=0,
                    cell=G[f"{name}_verts"], coeffs=G[f"{name}_coeffs"].reshape(m["ndof"], m["vdim"], -1))
        out.append(dict(base, verts=None, dofs=G[f"{name}_dofs"], pts=G[f"{name}_ppts"], ref=G[f"{name}_pref"]))
        b = batch(name, M.ORDER, 7, 4, nrhs=3, own=True)
        r = int(np.argmax(np.linalg.det(b["B"]) < 0))
        out.append(dict(base, verts=b["verts"][r], dofs=b["dofs"][r], pts=b["pts"][r], ref=b["ref"][r]))
    return out
