"""Golden vectors of Hdiv / Hcurl / EnrichedElement, generated from the *unmodified reference* in the build container:

    PYTHONPATH=oracle/restated_deps:/root/reference python -B tests/golden/make_golden_hdivcurl.py

Every entry is built by ``build(F, name)`` below, with F the reference's FIAT (here) or fiat_amd (the tests), so the two sides
compose the same element.  ``{name}_pts`` / ``{name}_tab``: tabulate(order, pts) stacked in mis() order, (ntab, ndof, sd,
npts) -- or (ntab, ndof, npts) for the scalar enriched element; ``{name}_meta``: [value size, mapping code, form degree
(-1: None), degree, space dimension]; ``{name}_eids`` / ``{name}_feids``: entity dofs as (dimension code, entity, dof) rows
of the product / the FlattenedDimensions numbering; ``{name}_dual``: class code of every dual node; ``{name}_c`` /
``{name}_d``: the 1-D nodes of C (K+1) and D (K) of the quad / hex families; ``ent_*``: entity= tabulations.  Plain
numbers only."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

MAPPINGS = ["affine", "contravariant piola", "covariant piola"]
DUAL_CLASSES = ["Functional", "PointEvaluation", "ComponentPointEvaluation"]


def _enrich(F, a, b, rev):
    return F.EnrichedElement(*((b, a) if rev else (a, b)))


def build(F, name):
    """name = family + k + variant (d: default, s: "spectral") + summand order (0, 1 reversed); or a prism / rotation /
    scalar case."""
    I = F.reference_element.UFCInterval()
    fam, k, var, rev = name[:-3], int(name[-3]), name[-2], int(name[-1])
    kw = {"variant": "spectral"} if var == "s" else {}
    T = F.TensorProductElement
    CG = lambda n: F.Lagrange(I, n, **kw)                 # noqa: E731
    DG = lambda n: F.DiscontinuousLagrange(I, n, **kw)    # noqa: E731
    if fam == "rtcf":
        return _enrich(F, F.Hdiv(T(CG(k), DG(k - 1))), F.Hdiv(T(DG(k - 1), CG(k))), rev)
    if fam == "rtce":   # Firedrake's order: component 1's block first
        return _enrich(F, F.Hcurl(T(CG(k), DG(k - 1))), F.Hcurl(T(DG(k - 1), CG(k))), rev)
    if fam == "ncf":
        return _enrich(F, F.Hdiv(T(build(F, f"rtcf{k}{var}0"), DG(k - 1))), F.Hdiv(T(T(DG(k - 1), DG(k - 1)), CG(k))), rev)
    if fam == "nce":
        return _enrich(F, F.Hcurl(T(build(F, f"rtce{k}{var}0"), CG(k))), F.Hcurl(T(T(CG(k), CG(k)), DG(k - 1))), rev)
    if fam == "sdiv":    # single summands
        return F.Hdiv(T(CG(k), DG(k - 1)))
    if fam == "scurl":
        return F.Hcurl(T(CG(k), DG(k - 1)))
    if fam == "sdivz":
        return F.Hdiv(T(T(DG(k - 1), DG(k - 1)), CG(k)))
    if fam == "scurlz":
        return F.Hcurl(T(T(CG(k), CG(k)), DG(k - 1)))
    Tri = F.ufc_simplex(2)
    if fam == "pdiv":    # prisms
        return _enrich(F, F.Hdiv(T(F.RaviartThomas(Tri, k), DG(k - 1))), F.Hdiv(T(F.DiscontinuousLagrange(Tri, k - 1), CG(k))), rev)
    if fam == "pcurl":
        return _enrich(F, F.Hcurl(T(F.Nedelec(Tri, k), CG(k))), F.Hcurl(T(F.Lagrange(Tri, k), DG(k - 1))), rev)
    if fam == "rotdiv":
        return F.Hdiv(T(F.Nedelec(Tri, k), DG(k - 1)))
    if fam == "rotcurl":
        return F.Hcurl(T(F.RaviartThomas(Tri, k), CG(k)))
    if fam == "scal":
        return F.EnrichedElement(F.Lagrange(Tri, 1), F.DiscontinuousLagrange(Tri, 0))
    raise ValueError(name)


# (name, cell kind, orders) -- quad / hex families k = 1..3 (orders 0..3 for k <= 2), both variants, both summand orders
QUADHEX = []
for _k in (1, 2, 3):
    for _fam in ("rtcf", "rtce", "ncf", "nce"):
        for _var in ("d", "s"):
            for _rev in (0, 1):
                if _fam in ("ncf", "nce") and (_var, _rev) != ("d", 0) and _k != 2:
                    continue
                QUADHEX.append(f"{_fam}{_k}{_var}{_rev}")
QUADHEX += ["sdiv2d0", "scurl2d0", "sdivz2d0", "scurlz2d0", "sdiv1d0", "scurlz1s0"]
OTHERS = ["pdiv1d0", "pdiv2d0", "pcurl1d0", "pcurl2d0", "pdiv1d1", "rotdiv1d0", "rotdiv2d0", "rotcurl1d0", "rotcurl2d0", "scal1d0"]


def is_hex(name):
    return name.startswith(("ncf", "nce", "sdivz", "scurlz"))


def max_order(name):
    k = int(name[-3])
    return 3 if k <= 2 else 2


def points(sd, rng, cell):
    if cell == "prism":
        e = rng.exponential(size=(4, 3))
        tri = (e / e.sum(-1, keepdims=True))[:, 1:]
        z = rng.uniform(size=(4, 1))
        inside = np.concatenate([tri, z], axis=1)
        special = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 1.0], [0.5, 0.5, 0.3], [0.6, 0.6, 1.2]])
        return np.concatenate([inside, special])
    inside = rng.uniform(size=(4, sd))
    if sd == 2:
        special = np.array([[0.0, 0.0], [1.0, 1.0], [0.0, 0.5], [0.3, 1.0], [1.2, -0.1]])
    else:
        special = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [0.5, 0.0, 0.0], [0.0, 0.4, 1.0], [1.1, 0.5, -0.2]])
    return np.concatenate([inside, special])


def stack(tab, sd, order, mis):
    return np.stack([np.asarray(tab[a], dtype=float) for k in range(order + 1) for a in mis(sd, k)])


def flat_dim_code(d):
    """Product entity dimension (nested tuple) -> an integer code: digits of the flattened dimensions."""
    def flat(x):
        return sum((flat(y) for y in x), ()) if isinstance(x, tuple) else (x,)
    return int("".join(str(v) for v in flat(d))) if isinstance(d, tuple) else int(d)


def eids_rows(ids):
    return np.array([(flat_dim_code(d), e, i) for d in sorted(ids, key=repr) for e in sorted(ids[d]) for i in ids[d][e]],
                    dtype=np.int64).reshape(-1, 3)


def metadata(el):
    fd = el.get_formdegree()
    vs = el.value_shape()
    return np.array([int(np.prod(vs)) if vs else 1, MAPPINGS.index(el.mapping()[0]), -1 if fd is None else fd, el.degree(),
                     el.space_dimension()], dtype=np.int64)


def dual_codes(el):
    return np.array([DUAL_CLASSES.index(type(n).__name__) if type(n).__name__ in DUAL_CLASSES else 9
                     for n in el.dual_basis()], dtype=np.int64)


def main():
    import FIAT
    from FIAT.polynomial_set import mis
    from FIAT.tensor_product import FlattenedDimensions
    rng = np.random.default_rng(2024)
    out = {}
    for name in QUADHEX + OTHERS:
        el = build(FIAT, name)
        sd = el.get_reference_element().get_spatial_dimension()
        cell = "prism" if name in OTHERS and not name.startswith("scal") else ("tri" if name.startswith("scal") else "box")
        if cell == "tri":
            e = rng.exponential(size=(5, 3))
            pts = (e / e.sum(-1, keepdims=True))[:, 1:]
        else:
            pts = points(sd, rng, cell)
        if name.startswith("nce3"):
            pts = pts[[0, 5, 8]]
        order = max_order(name) if name in QUADHEX else 2
        out[f"{name}_pts"] = pts
        out[f"{name}_tab"] = stack(el.tabulate(order, pts), sd, order, mis)
        out[f"{name}_meta"] = metadata(el)
        out[f"{name}_eids"] = eids_rows(el.entity_dofs())
        out[f"{name}_dual"] = dual_codes(el)
        if name in QUADHEX:
            out[f"{name}_feids"] = eids_rows(FlattenedDimensions(el).entity_dofs())
            k, var = int(name[-3]), name[-2]
            kw = {"variant": "spectral"} if var == "s" else {}
            I = FIAT.reference_element.UFCInterval()
            out[f"{name}_c"] = np.array([list(n.get_point_dict())[0][0] for n in FIAT.Lagrange(I, k, **kw).dual_basis()])
            out[f"{name}_d"] = np.array([list(n.get_point_dict())[0][0]
                                         for n in FIAT.DiscontinuousLagrange(I, k - 1, **kw).dual_basis()])
    # entity=: quadrilateral facets (flattened and product ids), a face and an edge of the hexahedron
    q = rng.uniform(size=(4, 1))
    f2 = rng.uniform(size=(4, 2))
    quad, hexa = build(FIAT, "rtcf2d0"), build(FIAT, "ncf2d0")
    out["ent_p1"], out["ent_p2"] = q, f2
    for e in range(4):
        out[f"ent_rtcf_flat_e{e}"] = stack(FlattenedDimensions(quad).tabulate(1, q, entity=(1, e)), 2, 1, mis)
    out["ent_rtcf_prod_10_1"] = stack(quad.tabulate(1, q, entity=((1, 0), 1)), 2, 1, mis)
    out["ent_ncf_flat_f1"] = stack(FlattenedDimensions(hexa).tabulate(1, f2, entity=(2, 1)), 3, 1, mis)
    out["ent_ncf_flat_e4"] = stack(FlattenedDimensions(hexa).tabulate(1, q, entity=(1, 4)), 3, 1, mis)
    out["ent_ncf_prod_f"] = stack(hexa.tabulate(1, f2, entity=(((1, 0), 1), 1)), 3, 1, mis)
    nce = build(FIAT, "nce1d0")
    out["ent_nce_flat_f3"] = stack(FlattenedDimensions(nce).tabulate(2, f2, entity=(2, 3)), 3, 2, mis)
    path = os.path.join(HERE, "hdivcurl.npz")
    np.savez_compressed(path, **out)
    print(len(out), "arrays ->", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
