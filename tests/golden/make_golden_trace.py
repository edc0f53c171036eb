"""Golden vectors of HDivTrace and Legendre, generated from the *unmodified reference* in the build container (seconds):

    PYTHONPATH=oracle/restated_deps:/root/reference python -B tests/golden/make_golden_trace.py

Every element is built by ``build(F, name)`` below, with F the reference's FIAT (here) or fiat_amd (the tests), so the two
sides construct the same element.  Per case ``name``:

``{name}_meta``    [degree(), space dimension, form degree, spatial dimension];
``{name}_eids``    entity dofs as (dimension code, entity, dof) rows;
``{name}_facets``  the facets in dof-block order as (dimension code, entity) rows;
``{name}_nodes``   the points of the dual nodes, where all nodes are point evaluations;
``{name}_f{j}_pts`` / ``_tab``  tabulate(0, pts, entity=facet j): seeded points of the facet, its vertices, two points slightly
                   outside it; the table (ndof, npts);
``{name}_span_pts`` / ``_tab``  (simplices) tabulate(0, pts) over cell points that span all facets in one call;
``{name}_fail{n}_pts`` / ``_tab``  (simplices) calls that fail -- a vertex, an interior point, on the tetrahedron an edge
                   midpoint, each between two good points -- as the reference's all-NaN table;
``hex_raises``     1: HDivTrace on the UFC hexahedron raises NotImplementedError.

``leg_{cell}{k}_coeffs`` / ``_pts`` / ``_tab``: get_coeffs() and tabulate(0, pts) of Legendre on the interval ("int") and the
triangle ("tri"), degrees 0-4.  Plain float64 and int64 only."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

# name -> (cell, degree, variant)
CASES = {"int0": ("interval", 0, None)}
for _k in range(0, 8):
    CASES[f"tri{_k}"] = ("triangle", _k, None)
    CASES[f"tet{_k}"] = ("tetrahedron", _k, None)
for _k in range(1, 5):
    for _tag, _variant in (("s", "spectral"), ("i", "integral")):
        CASES[f"tri{_k}{_tag}"] = ("triangle", _k, _variant)
        CASES[f"tet{_k}{_tag}"] = ("tetrahedron", _k, _variant)
for _k in range(0, 5):
    CASES[f"quad{_k}"] = ("quadrilateral", _k, None)
CASES["prod22"] = ("product", (2, 2), None)
CASES["prod13"] = ("product", (1, 3), None)
CASES["prism21"] = ("prism", (2, 1), None)
SIMPLICES = ("interval", "triangle", "tetrahedron")
LEGENDRE = {f"leg_{c}{k}": (c, k) for c in ("int", "tri") for k in range(5)}


def cell(F, kind):
    R = F.reference_element
    return {"interval": lambda: R.UFCInterval(), "triangle": lambda: R.UFCTriangle(), "tetrahedron": lambda: R.UFCTetrahedron(),
            "quadrilateral": lambda: R.UFCQuadrilateral(), "hexahedron": lambda: R.UFCHexahedron(),
            "product": lambda: R.TensorProductCell(R.UFCInterval(), R.UFCInterval()),
            "prism": lambda: R.TensorProductCell(R.UFCTriangle(), R.UFCInterval())}[kind]()


def build(F, name):
    from importlib import import_module
    if name in LEGENDRE:
        c, k = LEGENDRE[name]
        return import_module(F.__name__ + ".hierarchical").Legendre(cell(F, {"int": "interval", "tri": "triangle"}[c]), k)
    kind, degree, variant = CASES[name]
    return import_module(F.__name__ + ".hdiv_trace").HDivTrace(cell(F, kind), degree, variant)


def flat(d):
    return sum((flat(y) for y in d), ()) if isinstance(d, tuple) else (d,)


def dim_code(d):
    """Entity dimension -> an integer: a product cell's tuple key as the digits of its flattened dimensions."""
    return int("".join(str(v) for v in flat(d))) if isinstance(d, tuple) else int(d)


def eids_rows(ids):
    return np.array([(dim_code(d), e, i) for d in sorted(ids, key=repr) for e in sorted(ids[d]) for i in ids[d][e]],
                    dtype=np.int64).reshape(-1, 3)


def facets_of(el):
    """The facets in dof-block order: by facet kind (sorted dimension keys), then by entity number."""
    ref_el = el.get_reference_element()
    top = ref_el.get_topology()
    fd = ref_el.get_spatial_dimension() - 1
    return [(d, e) for d in sorted(k for k in top if sum(flat(k)) == fd) for e in sorted(top[d])]


def facet_points(dims, rng):
    """Seeded points of a facet cell, its vertices and two points slightly outside it; ``dims``: the flattened factor
    dimensions of the facet (a simplex: one entry)."""
    dims = [d for d in dims if d > 0]
    if not dims:
        return np.zeros((3, 0))
    if dims == [1]:
        return np.concatenate([rng.uniform(size=(4, 1)), [[0.0], [1.0], [-0.05], [1.1]]])
    if dims == [2]:
        e = rng.exponential(size=(4, 3))
        return np.concatenate([(e / e.sum(-1, keepdims=True))[:, 1:], [[0, 0], [1, 0], [0, 1], [-0.05, 0.3], [0.6, 0.55]]])
    if dims == [1, 1]:
        return np.concatenate([rng.uniform(size=(4, 2)), [[0, 0], [1, 0], [0, 1], [1, 1], [-0.05, 0.3], [0.6, 1.1]]])
    raise ValueError(dims)


def node_points(el):
    pts = []
    for node in el.dual_basis():
        pd = node.get_point_dict()
        if len(pd) != 1:
            return None
        (pt, entries), = pd.items()
        (w, comp), = entries
        if w != 1.0 or tuple(comp) != ():
            return None
        pts.append([float(x) for x in pt])
    return np.array(pts, dtype=float).reshape(len(pts), -1)


def main():
    import FIAT
    rng = np.random.default_rng(2027)
    out = {}
    for name, (kind, degree, variant) in CASES.items():
        el = build(FIAT, name)
        ref_el = el.get_reference_element()
        sd = ref_el.get_spatial_dimension()
        out[f"{name}_meta"] = np.array([el.degree(), el.space_dimension(), el.get_formdegree(), sd], dtype=np.int64)
        out[f"{name}_eids"] = eids_rows(el.entity_dofs())
        facets = facets_of(el)
        out[f"{name}_facets"] = np.array([(dim_code(d), e) for d, e in facets], dtype=np.int64)
        assert set(el.mapping()) == {"affine"} and el.value_shape() == () and el.is_nodal()
        nodes = node_points(el)
        if nodes is not None:
            out[f"{name}_nodes"] = nodes
        evalkey = (0,) * sd
        for j, (d, e) in enumerate(facets):
            pts = facet_points(list(flat(d)), rng)
            tab = el.tabulate(0, [tuple(p) for p in pts], entity=(d, e))[evalkey]
            out[f"{name}_f{j}_pts"] = pts
            out[f"{name}_f{j}_tab"] = np.asarray(tab, dtype=float)
        if kind in SIMPLICES:
            good = []
            for j, (d, e) in enumerate(facets):
                fp = facet_points([d], rng)[:2]
                good.append(np.asarray(ref_el.get_entity_transform(d, e)(fp), dtype=float).reshape(len(fp), sd))
            span = np.concatenate(good)
            span = span[rng.permutation(len(span))]
            out[f"{name}_span_pts"] = span
            out[f"{name}_span_tab"] = np.asarray(el.tabulate(0, span)[evalkey], dtype=float)
            assert np.isfinite(out[f"{name}_span_tab"]).all()
            verts = np.asarray(ref_el.get_vertices(), dtype=float)
            bad = [verts[0], verts.mean(axis=0)]
            if sd == 3:
                bad.append(0.5 * (verts[1] + verts[2]))
            if sd == 1:
                bad = bad[1:]         # (a vertex of the interval is a facet)
            for n, b in enumerate(bad):
                pts = np.stack([span[0], b, span[1]])
                tab = np.asarray(el.tabulate(0, pts)[evalkey], dtype=float)
                assert np.isnan(tab).all()
                out[f"{name}_fail{n}_pts"] = pts
                out[f"{name}_fail{n}_tab"] = tab
        print(name, out[f"{name}_meta"], flush=True)
    try:
        from FIAT.hdiv_trace import HDivTrace
        HDivTrace(cell(FIAT, "hexahedron"), 1)
        out["hex_raises"] = np.array([0], dtype=np.int64)
    except NotImplementedError:
        out["hex_raises"] = np.array([1], dtype=np.int64)
    for name, (c, k) in LEGENDRE.items():
        el = build(FIAT, name)
        sd = el.get_reference_element().get_spatial_dimension()
        pts = facet_points([sd], rng)
        out[f"{name}_coeffs"] = np.asarray(el.get_coeffs(), dtype=float)
        out[f"{name}_pts"] = pts
        out[f"{name}_tab"] = np.asarray(el.tabulate(0, pts)[(0,) * sd], dtype=float)
        out[f"{name}_meta"] = np.array([el.degree(), el.space_dimension(), el.get_formdegree(), sd], dtype=np.int64)
        print(name, out[f"{name}_meta"], flush=True)
    path = os.path.join(HERE, "trace.npz")
    np.savez_compressed(path, **out)
    print(len(out), "arrays ->", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
