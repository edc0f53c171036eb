"""Golden vectors of Serendipity, generated from the *unmodified reference* in the build container (minutes: the reference
differentiates sympy expressions):

    PYTHONPATH=oracle/restated_deps:/root/reference python -B tests/golden/make_golden_serendipity.py

Every entry is built by ``build(F, name)`` below, with F the reference's FIAT (here) or fiat_amd (the tests), so the two
sides construct the same element.  ``{name}_pts`` / ``{name}_tab``: tabulate(order, pts) stacked in mis() order, (ntab, ndof,
npts); ``{name}_meta``: [degree(), space dimension, form degree, order]; ``{name}_eids``: entity dofs as (dimension, entity,
dof) rows; ``{name}_upts``: unisolvent_pts; ``{name}_dual``: the dual nodes as a dense matrix, [i, j] = weight of node i at
unisolvent point j (0: no entry); ``ent_*``: entity= tabulations and their points.  Plain numbers only."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

# name -> (cell, degree, derivative order, store the dual)
CASES = {}
for _k in range(1, 7):
    CASES[f"q{_k}"] = ("quad", _k, 2, True)
    CASES[f"h{_k}"] = ("hex", _k, 2, True)
CASES["q7"] = ("quad", 7, 1, False)      # beyond the compile-time instances
CASES["q8"] = ("quad", 8, 1, False)
CASES["h7"] = ("hex", 7, 1, False)
CASES["q3o3"] = ("quad", 3, 3, False)    # third derivatives
CASES["h2o3"] = ("hex", 2, 3, False)
CASES["p3"] = ("prod", 3, 2, True)       # interval x interval, not flattened
CASES["b5"] = ("box", 5, 2, True)        # [-1, 1] x [0, 1]: the one non-unit box the reference can build (a product of lines)

ENTITIES = [("h3", 2, 1), ("h3", 2, 4), ("h4", 1, 5), ("h3", 1, 10), ("q4", 1, 2), ("q3", 1, 1), ("b5", 1, 0)]


def cell(F, kind):
    R = F.reference_element
    if kind == "quad":
        return R.UFCQuadrilateral()
    if kind == "hex":
        return R.UFCHexahedron()
    if kind == "prod":
        return R.TensorProductCell(R.UFCInterval(), R.UFCInterval())
    if kind == "box":
        return R.TensorProductCell(R.DefaultLine(), R.UFCInterval())
    raise ValueError(kind)


def build(F, name):
    kind, k = CASES[name][:2]
    from importlib import import_module
    return import_module(F.__name__ + ".serendipity").Serendipity(cell(F, kind), k)


def points(kind, rng):
    """Vertices, an edge and a face midpoint, seeded interior points, two points outside the cell."""
    if kind == "hex":
        special = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 1.0], [0.5, 1.0, 0.0], [0.5, 0.5, 1.0], [1.2, 0.4, -0.1], [-0.3, 1.1, 0.5]])
        return np.concatenate([special, rng.uniform(size=(4, 3))])
    special = np.array([[0.0, 0.0], [1.0, 1.0], [0.0, 0.5], [0.5, 0.5], [1.2, -0.1], [0.3, 1.25]])
    pts = np.concatenate([special, rng.uniform(size=(5, 2))])
    if kind == "box":
        pts[:, 0] = 2.0 * pts[:, 0] - 1.0
    return pts


def stack(tab, sd, order, mis):
    return np.stack([np.asarray(tab[a], dtype=float) for k in range(order + 1) for a in mis(sd, k)])


def flat_dim_code(d):
    """Entity dimension -> an integer: a product cell's tuple key as the digits of its flattened dimensions."""
    def flat(x):
        return sum((flat(y) for y in x), ()) if isinstance(x, tuple) else (x,)
    return int("".join(str(v) for v in flat(d))) if isinstance(d, tuple) else int(d)


def eids_rows(ids):
    return np.array([(flat_dim_code(d), e, i) for d in sorted(ids, key=repr) for e in sorted(ids[d]) for i in ids[d][e]],
                    dtype=np.int64).reshape(-1, 3)


def metadata(el):
    return np.array([el.degree(), el.space_dimension(), el.get_formdegree(), el.get_order()], dtype=np.int64)


def dual_matrix(el, upts):
    index = {tuple(float(x) for x in p): j for j, p in enumerate(upts)}
    W = np.zeros((el.space_dimension(), len(upts)))
    for i, node in enumerate(el.dual_basis()):
        for pt, entries in node.get_point_dict().items():
            for w, comp in entries:
                assert tuple(comp) == ()
                W[i, index[tuple(float(x) for x in pt)]] += w
    return W


def main():
    import FIAT
    from FIAT.polynomial_set import mis
    from FIAT.serendipity import unisolvent_pts
    rng = np.random.default_rng(2025)
    out, els = {}, {}
    for name, (kind, k, order, dual) in CASES.items():
        el = els[name] = build(FIAT, name)
        sd = el.get_reference_element().get_spatial_dimension()
        pts = points(kind, rng)
        out[f"{name}_pts"] = pts
        out[f"{name}_tab"] = stack(el.tabulate(order, pts), sd, order, mis)
        out[f"{name}_meta"] = metadata(el)
        out[f"{name}_eids"] = eids_rows(el.entity_dofs())
        upts = np.array(unisolvent_pts(cell(FIAT, kind), k), dtype=float)
        out[f"{name}_upts"] = upts
        if dual:
            out[f"{name}_dual"] = dual_matrix(el, upts)
        print(name, out[f"{name}_tab"].shape, flush=True)
    for name, dim, ent in ENTITIES:
        el = els[name]
        sd = el.get_reference_element().get_spatial_dimension()
        p = rng.uniform(size=(4, dim))
        key = ((1, 0), 0) if name == "b5" else (dim, ent)    # the product cell's own entity key: the edge y = 0
        out[f"ent_{name}_{dim}_{ent}_pts"] = p
        out[f"ent_{name}_{dim}_{ent}_tab"] = stack(el.tabulate(1, p, entity=key), sd, 1, mis)
    path = os.path.join(HERE, "serendipity.npz")
    np.savez_compressed(path, **out)
    print(len(out), "arrays ->", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
