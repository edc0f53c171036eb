"""Golden vectors of IntegratedLegendre, generated from the *unmodified reference* in the build container (seconds):

    PYTHONPATH=oracle/restated_deps:/root/reference python -B tests/golden/make_golden_hierarchical.py

Every element is built by ``build(F, name)`` below, with F the reference's FIAT (here) or fiat_amd (the tests), so the two
sides construct the same element.  Per case ``name`` (``int``/``tri``/``tet`` + degree [+ ``i2`` for variant "integral(2)"]):

``{name}_meta``     [degree(), space dimension, form degree, spatial dimension];
``{name}_eids``     entity dofs as (dimension, entity, dof) rows;
``{name}_cids``     entity closure dofs, the same way;
``{name}_coeffs``   get_coeffs();
``{name}_pts`` / ``_tab``  tabulate(order, pts) as (ntab, ndof, npts), tables in mis() order; the points are the cell's
                    vertices, one edge midpoint, the barycentre, six seeded interior points and two points up to 0.2 outside;
``{name}_order``    the order of that table: 2 for degrees 1-6, 1 for tri7, 3 for tet3o3 (both general-route cases);
``{name}_e_ent`` / ``_e_pts`` / ``_e_tab``  (tri3: edge 1; tet3: face 2) tabulate(1, pts, entity=ent), pts in the entity's
                    coordinates.
``raises_degree0``  1: IntegratedLegendre(cell, 0) raises ValueError; ``raises_text``: its message as bytes.
Plain float64, int64 and uint8 only."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

CELLS = {"int": "interval", "tri": "triangle", "tet": "tetrahedron"}
# name -> (cell, degree, variant, order)
CASES = {f"{c}{k}": (c, k, None, 2) for c in CELLS for k in range(1, 7)}
CASES["tri7"] = ("tri", 7, None, 1)
CASES["tet3o3"] = ("tet", 3, None, 3)
CASES["tri3i2"] = ("tri", 3, "integral(2)", 2)
ENTITY = {"tri3": (1, 1), "tet3": (2, 2)}


def cell(F, kind):
    R = F.reference_element
    return {"interval": R.UFCInterval, "triangle": R.UFCTriangle, "tetrahedron": R.UFCTetrahedron}[kind]()


def build(F, name):
    from importlib import import_module
    c, k, variant, _ = CASES[name]
    return import_module(F.__name__ + ".hierarchical").IntegratedLegendre(cell(F, CELLS[c]), k, variant)


def mis(sd, order):
    if sd == 1:
        return [(order,)]
    return [(order - i,) + rest for i in range(order + 1) for rest in mis(sd - 1, i)]


def ids_rows(ids):
    return np.array([(d, e, i) for d in sorted(ids) for e in sorted(ids[d]) for i in ids[d][e]], dtype=np.int64).reshape(-1, 3)


def cell_points(sd, rng):
    """Vertices, one edge midpoint, the barycentre, six seeded interior points, two points up to 0.2 outside the cell."""
    verts = np.vstack([np.zeros(sd), np.eye(sd)])
    e = rng.exponential(size=(6, sd + 1))
    inner = (e / e.sum(-1, keepdims=True))[:, 1:]
    outside = np.stack([np.concatenate([[-0.2], np.full(sd - 1, 0.3)]), np.full(sd, 1.0 / sd) + 0.2 / sd])
    return np.concatenate([verts, [0.5 * (verts[0] + verts[-1])], [verts.mean(axis=0)], inner, outside])


def table(el, order, pts, entity=None):
    sd = el.get_reference_element().get_spatial_dimension()
    tab = el.tabulate(order, [tuple(p) for p in pts], entity) if entity else el.tabulate(order, [tuple(p) for p in pts])
    return np.stack([np.asarray(tab[a], dtype=float) for k in range(order + 1) for a in mis(sd, k)])


def main():
    import FIAT
    rng = np.random.default_rng(2028)
    out = {}
    for name, (c, k, variant, order) in CASES.items():
        el = build(FIAT, name)
        sd = el.get_reference_element().get_spatial_dimension()
        out[f"{name}_meta"] = np.array([el.degree(), el.space_dimension(), el.get_formdegree(), sd], dtype=np.int64)
        out[f"{name}_eids"] = ids_rows(el.entity_dofs())
        out[f"{name}_cids"] = ids_rows(el.entity_closure_dofs())
        out[f"{name}_coeffs"] = np.asarray(el.get_coeffs(), dtype=float)
        pts = cell_points(sd, rng)
        out[f"{name}_pts"] = pts
        out[f"{name}_tab"] = table(el, order, pts)
        out[f"{name}_order"] = np.array([order], dtype=np.int64)
        if name in ENTITY:
            dim, number = ENTITY[name]
            epts = cell_points(dim, rng)[:-2]
            out[f"{name}_e_ent"] = np.array([dim, number], dtype=np.int64)
            out[f"{name}_e_pts"] = epts
            out[f"{name}_e_tab"] = table(el, 1, epts, (dim, number))
        print(name, out[f"{name}_meta"], out[f"{name}_tab"].shape, flush=True)
    from FIAT.hierarchical import IntegratedLegendre
    try:
        IntegratedLegendre(cell(FIAT, "triangle"), 0)
        out["raises_degree0"] = np.array([0], dtype=np.int64)
        out["raises_text"] = np.zeros(0, dtype=np.uint8)
    except ValueError as err:
        out["raises_degree0"] = np.array([1], dtype=np.int64)
        out["raises_text"] = np.frombuffer(str(err).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "hierarchical.npz")
    np.savez_compressed(path, **out)
    print(len(out), "arrays ->", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
