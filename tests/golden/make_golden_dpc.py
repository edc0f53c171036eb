"""Golden vectors of DPC, generated from the *unmodified reference* in the build container (seconds):

    PYTHONPATH=oracle/restated_deps:/root/reference python -B tests/golden/make_golden_dpc.py

Every entry is built by ``build(F, name)`` below, with F the reference's FIAT (here) or fiat_amd (the tests), so the two
sides construct the same element.  ``{name}_pts`` / ``{name}_tab``: tabulate(order, pts) stacked in mis() order, (ntab, ndof,
npts) -- not for the product cells, whose ``tabulate`` raises a TypeError in the reference; ``{name}_meta``: [degree(), space
dimension, form degree, order]; ``{name}_eids`` / ``{name}_cids``: entity dofs and entity closure dofs as (dimension, entity,
dof) rows; ``{name}_nodes``: the points of the dual nodes, in node order; ``{name}_coeffs``: get_coeffs(); ``ent_*``:
entity= tabulations and their points; ``{name}_keyerror``: 1 where the reference's constructor raises a KeyError.  Plain
numbers only."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

# name -> (cell, degree, derivative order; None: no tables)
CASES = {}
for _k in range(0, 7):
    CASES[f"q{_k}"] = ("quad", _k, 2)
    CASES[f"h{_k}"] = ("hex", _k, 2)
CASES["q7"] = ("quad", 7, 1)         # beyond the direct kernel's degrees: the general route
CASES["h3o3"] = ("hex", 3, 3)        # third derivatives: the general route
CASES["p3"] = ("prod", 3, None)      # interval x interval, not flattened
# [-1, 1] x [0, 1] flattens to a hypercube that is not a UFC cell: the reference's hypercube_simplex_map has no entry for it
# and DPC raises a KeyError.  Recorded as such (``b2_keyerror`` = 1); there are no nodes or metadata to take.
RAISES = {"b2": ("box", 2)}

# (case, dimension, entity, derivative order)
ENTITIES = [("q3", 1, 2, 1), ("h2", 2, 3, 1)]


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
    kind, k = (CASES[name] if name in CASES else RAISES[name])[:2]
    from importlib import import_module
    return import_module(F.__name__ + ".discontinuous_pc").DPC(cell(F, kind), k)


def points(kind, rng):
    """The vertices, an edge and a face midpoint, seeded points in the cell, two points at most 0.2 outside it."""
    if kind == "hex":
        verts = np.array([[i, j, k] for i in (0.0, 1.0) for j in (0.0, 1.0) for k in (0.0, 1.0)])
        special = np.array([[0.5, 1.0, 0.0], [0.5, 0.5, 1.0], [1.2, 0.4, -0.1], [-0.15, 1.1, 0.5]])
        return np.concatenate([verts, special, rng.uniform(size=(6, 3))])
    verts = np.array([[i, j] for i in (0.0, 1.0) for j in (0.0, 1.0)])
    special = np.array([[0.0, 0.5], [0.5, 0.5], [1.2, -0.1], [0.3, 1.15]])
    return np.concatenate([verts, special, rng.uniform(size=(6, 2))])


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


def node_points(el):
    pts = []
    for node in el.dual_basis():
        (pt, entries), = node.get_point_dict().items()
        (w, comp), = entries
        assert w == 1.0 and tuple(comp) == ()
        pts.append([float(x) for x in pt])
    return np.array(pts, dtype=float)


def main():
    import FIAT
    from FIAT.polynomial_set import mis
    rng = np.random.default_rng(2026)
    out, els = {}, {}
    for name, (kind, k, order) in CASES.items():
        el = els[name] = build(FIAT, name)
        sd = el.get_reference_element().get_spatial_dimension()
        out[f"{name}_meta"] = metadata(el)
        out[f"{name}_eids"] = eids_rows(el.entity_dofs())
        out[f"{name}_cids"] = eids_rows(el.entity_closure_dofs())
        out[f"{name}_nodes"] = node_points(el)
        out[f"{name}_coeffs"] = np.asarray(el.get_coeffs(), dtype=float)
        assert set(el.mapping()) == {"affine"} and el.value_shape() == ()
        if order is not None:
            pts = points(kind, rng)
            out[f"{name}_pts"] = pts
            out[f"{name}_tab"] = stack(el.tabulate(order, pts), sd, order, mis)
        print(name, out[f"{name}_meta"], flush=True)
    for name in RAISES:
        try:
            build(FIAT, name)
            out[f"{name}_keyerror"] = np.array([0], dtype=np.int64)
        except KeyError:
            out[f"{name}_keyerror"] = np.array([1], dtype=np.int64)
        print(name, "KeyError:", out[f"{name}_keyerror"][0], flush=True)
    for name, dim, ent, order in ENTITIES:
        el = els[name]
        sd = el.get_reference_element().get_spatial_dimension()
        p = rng.uniform(size=(5, dim))
        out[f"ent_{name}_{dim}_{ent}_pts"] = p
        out[f"ent_{name}_{dim}_{ent}_tab"] = stack(el.tabulate(order, p, entity=(dim, ent)), sd, order, mis)
    path = os.path.join(HERE, "dpc.npz")
    np.savez_compressed(path, **out)
    print(len(out), "arrays ->", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
