"""Golden vectors of BDMCE / BDMCF and the trimmed serendipity families, generated from the *unmodified reference* in the
build container (minutes: the Sminus* classes evaluate sympy expressions with evalf, point by point):

    PYTHONPATH=oracle/restated_deps:/root/reference python -B tests/golden/make_golden_sforms.py

Every entry is built by ``build(F, name)`` below, with F the reference's FIAT (here) or fiat_amd (the tests), so the two
sides construct the same element.  ``{name}_pts`` / ``{name}_tab``: tabulate(order, pts) stacked in mis() order, (ntab,
nrows, sd, npts); ``{name}_meta``: [degree(), space_dimension(), form degree, order, value_shape()[0], len(mapping()),
mapping code (0 covariant, 1 contravariant Piola)]; ``{name}_eids`` / ``{name}_cids``: entity dofs / entity closure dofs as
(dimension, entity, dof) rows; ``ent_*``: entity= tabulations and their points.  Plain numbers only."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

CLASSES = {
    "bdmce": ("brezzi_douglas_marini_cube", "BrezziDouglasMariniCubeEdge"),
    "bdmcf": ("brezzi_douglas_marini_cube", "BrezziDouglasMariniCubeFace"),
    "sme": ("Sminus", "TrimmedSerendipityEdge"),
    "smf": ("Sminus", "TrimmedSerendipityFace"),
    "smc": ("SminusCurl", "TrimmedSerendipityCurl"),
    "smd": ("SminusDiv", "TrimmedSerendipityDiv"),
}
HEX_DEGREES = {"smd": range(1, 6), "smc": range(1, 6), "sme": range(1, 4)}

# name -> (class key, cell, degree, derivative order)
CASES = {}
for _c in CLASSES:
    for _k in range(1, 7):
        CASES[f"{_c}_q{_k}"] = (_c, "quad", _k, 2 if _k <= 4 else 1)
for _c, _ks in HEX_DEGREES.items():
    for _k in _ks:
        CASES[f"{_c}_h{_k}"] = (_c, "hex", _k, 2 if _k <= 2 else 1)
CASES["smc_p2"] = ("smc", "prod", 2, 2)        # interval x interval, not flattened
CASES["bdmcf_b2"] = ("bdmcf", "box", 2, 2)     # [-1, 1] x [0, 1]: t = 2 x - (v0 + v1) and h != 1
CASES["smd_b3"] = ("smd", "box", 3, 2)

# (case, entity key, dimension of the entity)
ENTITIES = [("smf_q3", (1, 2), 1), ("bdmce_q2", (1, 1), 1), ("smd_h2", (2, 3), 2), ("smc_h3", (1, 6), 1), ("sme_h2", (2, 0), 2),
            ("smc_p2", ((1, 0), 1), 1), ("bdmcf_b2", ((0, 1), 0), 1)]


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
    c, kind, k = CASES[name][:3]
    from importlib import import_module
    module, cls = CLASSES[c]
    return getattr(import_module(F.__name__ + "." + module), cls)(cell(F, kind), k)


def ent_name(case, key):
    def flat(x):
        return sum((flat(y) for y in x), ()) if isinstance(x, tuple) else (x,)
    return f"ent_{case}_" + "".join(str(v) for v in flat(key[0])) + f"_{key[1]}"


def points(kind, k, rng):
    """A vertex or two, an edge midpoint, two points outside the cell, seeded interior points (5 for the large hexahedral
    cases)."""
    if kind == "hex":
        special = np.array([[0.0, 0.0, 0.0], [0.5, 1.0, 0.0], [1.2, 0.4, -0.1], [-0.3, 1.1, 0.5]])
        if k <= 2:
            special = np.concatenate([special, [[1.0, 0.0, 1.0]]])
        return np.concatenate([special, rng.uniform(size=(1 if k > 2 else 2, 3))])
    special = np.array([[0.0, 0.0], [1.0, 1.0], [0.0, 0.5], [1.2, -0.1], [0.3, 1.25]])
    pts = np.concatenate([special, rng.uniform(size=(2, 2))])
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
    mapping = el.mapping()
    assert len(set(mapping)) == 1
    code = {"covariant piola": 0, "contravariant piola": 1}[mapping[0]]
    (vdim,) = el.value_shape()
    return np.array([el.degree(), el.space_dimension(), el.get_formdegree(), el.get_order(), vdim, len(mapping), code], dtype=np.int64)


def main():
    import FIAT
    from FIAT.polynomial_set import mis
    rng = np.random.default_rng(2026)
    out, els = {}, {}
    for name, (c, kind, k, order) in CASES.items():
        el = els[name] = build(FIAT, name)
        sd = el.get_reference_element().get_spatial_dimension()
        pts = points(kind, k, rng)
        out[f"{name}_pts"] = pts
        out[f"{name}_tab"] = stack(el.tabulate(order, pts), sd, order, mis)
        out[f"{name}_meta"] = metadata(el)
        out[f"{name}_eids"] = eids_rows(el.entity_dofs())
        out[f"{name}_cids"] = eids_rows(el.entity_closure_dofs())
        print(name, out[f"{name}_tab"].shape, flush=True)
    for name, key, edim in ENTITIES:
        el = els[name]
        sd = el.get_reference_element().get_spatial_dimension()
        p = rng.uniform(size=(3, edim))
        out[ent_name(name, key) + "_pts"] = p
        out[ent_name(name, key) + "_tab"] = stack(el.tabulate(1, p, entity=key), sd, 1, mis)
        print(ent_name(name, key), flush=True)
    path = os.path.join(HERE, "sforms.npz")
    np.savez_compressed(path, **out)
    print(len(out), "arrays ->", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
