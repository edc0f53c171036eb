"""Golden vectors of ``evaluate_batch``, generated from the *unmodified reference* in the build container (seconds):

    PYTHONPATH=oracle/restated_deps:/root/reference python -B tests/golden/make_golden_evaluate.py

Every element is built by ``build(F, name)`` below, with F the reference's FIAT (here) or fiat_amd (the tests), so the two
sides construct the same element.  Per case ``name`` (family + cell + degree):

``{name}_meta``     [degree(), space dimension, spatial dimension, number of components, mapping code (FX_MAP_*), variant of
                    the expansion set (0 default, 1 bubble, 2 dual)];
``{name}_scale``    get_scale(degree()) of the expansion set;
``{name}_coeffs``   get_coeffs();
``{name}_pts``      the 13 points of ``make_golden_hierarchical.cell_points``: the vertices (where the Duffy coordinates
                    collapse), an edge midpoint, the barycentre, six seeded interior points, two points outside the cell;
``{name}_dofs``     seeded dof vectors (3, ndof), uniform in [-1, 1];
``{name}_ref``      (ntab, 3, *value_shape, npts): the reference's own tabulate(2, pts) contracted with the dofs, tables in
                    mis() order;
``{name}_verts``    one seeded skewed physical cell (edges of length about 0.05);
``{name}_ppts`` / ``_pref``  the images of the points in that cell and the same contraction there: for the affine families the
                    reference's element built ON that cell, for the Piola families the reference-cell tables pushed forward by
                    the formula (chain rule through the affine map, then J^-T Phi / J Phi / det J / J^-T Phi J^-1).
Plain float64 and int64 only."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden_hierarchical import cell_points, mis  # noqa: E402

SD = {"int": 1, "tri": 2, "tet": 3}
MAPPINGS = {"affine": 0, "covariant piola": 1, "contravariant piola": 2, "double covariant piola": 3}
# name -> (class, cell, degree)
CASES = {}
for _k in (1, 2, 3, 6):
    CASES[f"lag_tri{_k}"] = ("Lagrange", "tri", _k)
for _k in (1, 3, 4, 6):
    CASES[f"lag_tet{_k}"] = ("Lagrange", "tet", _k)
CASES.update({
    "dg_tri2": ("DiscontinuousLagrange", "tri", 2), "dg_tet3": ("DiscontinuousLagrange", "tet", 3),
    "leg_int3": ("Legendre", "int", 3), "ileg_int4": ("IntegratedLegendre", "int", 4),
    "ned_tet1": ("Nedelec", "tet", 1), "ned_tet2": ("Nedelec", "tet", 2), "ned_tri3": ("Nedelec", "tri", 3),
    "rt_tet2": ("RaviartThomas", "tet", 2), "rt_tri3": ("RaviartThomas", "tri", 3),
    "bdm_tet2": ("BrezziDouglasMarini", "tet", 2), "ned2_tri2": ("NedelecSecondKind", "tri", 2),
    "regge_tri1": ("Regge", "tri", 1), "lag_tri7": ("Lagrange", "tri", 7),
})
GENERAL_ONLY = ("regge_tri1", "lag_tri7")
ORDER = 2
NRHS = 3


def physical_cell(F, sd, verts):
    base = F.ufc_simplex(sd)
    return F.reference_element.UFCSimplex(base.get_shape(), tuple(map(tuple, np.asarray(verts, dtype=float))), base.get_topology())


def build(F, name, verts=None):
    cls, c, k = CASES[name]
    sd = SD[c]
    cell = F.ufc_simplex(sd) if verts is None else physical_cell(F, sd, verts)
    return getattr(F, cls)(cell, k)


def contracted(el, pts, dofs):
    """(ntab, nrhs, *value_shape, npts) from the element's own tabulate."""
    sd = el.get_reference_element().get_spatial_dimension()
    tab = el.tabulate(ORDER, [tuple(p) for p in pts])
    stack = np.stack([np.asarray(tab[a], dtype=float) for k in range(ORDER + 1) for a in mis(sd, k)])
    return np.einsum("ji,ti...->tj...", dofs, stack)


def chain(res, B):
    """Derivatives with respect to x = B X + v0 of tables (ntab, ..., npts) taken with respect to X."""
    sd = B.shape[0]
    Bi = np.linalg.inv(B)
    out = [res[0]]
    g = res[1:1 + sd]
    out += [sum(Bi[e, d] * g[e] for e in range(sd)) for d in range(sd)]
    second = mis(sd, 2)
    pos = {a: 1 + sd + i for i, a in enumerate(second)}

    def ref_h(e1, e2):
        a = [0] * sd
        a[e1] += 1
        a[e2] += 1
        return res[pos[tuple(a)]]

    for a in second:
        d = [i for i, m in enumerate(a) for _ in range(m)]
        out.append(sum(Bi[e1, d[0]] * Bi[e2, d[1]] * ref_h(e1, e2) for e1 in range(sd) for e2 in range(sd)))
    return np.stack(out)


def pushed(res, B, mapping):
    """The Piola map of the cell x = B X + v0 applied to the components of (ntab, nrhs, *value_shape, npts)."""
    if mapping == "affine":
        return res
    if mapping == "covariant piola":
        return np.einsum("ab,tjbp->tjap", np.linalg.inv(B).T, res)
    if mapping == "contravariant piola":
        return np.einsum("ab,tjbp->tjap", B / np.linalg.det(B), res)
    assert mapping == "double covariant piola"
    M = np.linalg.inv(B).T
    return np.einsum("ab,tjbcp,dc->tjadp", M, res, M)


def skewed_cell(sd, rng):
    B = 0.05 * (np.eye(sd) + 0.3 * rng.standard_normal((sd, sd)))
    if np.linalg.det(B) < 0:
        B[:, 0] *= -1
    v0 = rng.standard_normal(sd)
    return np.vstack([v0, v0 + B.T])


def main():
    import FIAT
    rng = np.random.default_rng(2031)
    out = {}
    for name, (cls, c, k) in CASES.items():
        sd = SD[c]
        el = build(FIAT, name)
        mapping = el.mapping()[0]
        vs = tuple(el.value_shape())
        pts = cell_points(sd, rng)
        dofs = rng.uniform(-1.0, 1.0, size=(NRHS, el.space_dimension()))
        verts = skewed_cell(sd, rng)
        B = (verts[1:] - verts[0]).T
        ppts = pts @ B.T + verts[0]
        es = el.get_nodal_basis().get_expansion_set()
        out[f"{name}_meta"] = np.array([el.degree(), el.space_dimension(), sd, int(np.prod(vs, dtype=int)), MAPPINGS[mapping],
                                        {None: 0, "bubble": 1, "dual": 2}[es.variant]], dtype=np.int64)
        out[f"{name}_scale"] = np.array([float(es.get_scale(el.degree()))])
        out[f"{name}_coeffs"] = np.asarray(el.get_coeffs(), dtype=float)
        out[f"{name}_pts"] = pts
        out[f"{name}_dofs"] = dofs
        out[f"{name}_ref"] = contracted(el, pts, dofs)
        out[f"{name}_verts"] = verts
        out[f"{name}_ppts"] = ppts
        if mapping == "affine":
            out[f"{name}_pref"] = contracted(build(FIAT, name, verts), ppts, dofs)
        else:
            out[f"{name}_pref"] = pushed(chain(out[f"{name}_ref"], B), B, mapping)
        print(name, out[f"{name}_meta"], mapping, out[f"{name}_ref"].shape, float(np.abs(out[f"{name}_pref"]).max()), flush=True)
    path = os.path.join(HERE, "evaluate.npz")
    np.savez_compressed(path, **out)
    print(len(out), "arrays ->", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
