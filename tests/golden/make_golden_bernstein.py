"""Golden vectors of the Bernstein element, generated from the *unmodified reference* in the build container:

    PYTHONPATH=oracle/restated_deps:/root/reference OMP_NUM_THREADS=1 python -B tests/golden/make_golden_bernstein.py

``tab_s{sd}_n{n}``: Bernstein(ufc_simplex(sd), n).tabulate(3, pts_s{sd}) stacked in mis() order (orders 0..3), at points
inside the cell, exactly on its vertices and edges, and outside it; ``hi_*``: degree 10 on the tetrahedron and 16 on the
triangle, order 1; ``ent_*``: entity= tabulations; ``phys_*``: the element the reference builds on a physical simplex
(one of the two per dimension negatively oriented) at physical points, order 2; ``d2_*``: P3 triangle at
create_quadrature(T, 3), order 2; ``eids_*``: entity_ids as (dim, entity, dof) rows; ``lat_*`` / ``dualw_*``: the GLL
lattice and the pointwise-dual weights (node x lattice point).  Plain numbers only.  The reference's tables where the
derivative order equals the degree (>= 2) are stored as it returns them (1 instead of n!): the tests correct them."""
import os

import numpy as np

import FIAT
from FIAT.polynomial_set import mis
from FIAT.quadrature_schemes import create_quadrature
from FIAT.reference_element import UFCSimplex, make_lattice

HERE = os.path.dirname(os.path.abspath(__file__))


def stack(tab, sd, order):
    return np.stack([np.asarray(tab[a], dtype=float) for k in range(order + 1) for a in mis(sd, k)])


def physical(sd, verts):
    ref = FIAT.ufc_simplex(sd)
    return UFCSimplex(ref.get_shape(), tuple(map(tuple, verts)), ref.get_topology())


def points(sd, rng, ninside):
    ref = np.array(FIAT.ufc_simplex(sd).get_vertices(), dtype=float)
    e = rng.exponential(size=(ninside, sd + 1))
    inside = (e / e.sum(-1, keepdims=True)) @ ref
    edges = np.array([0.25 * ref[0] + 0.75 * ref[1], 0.5 * ref[1] + 0.5 * ref[-1]])
    outside = np.array([np.full(sd, 0.7), np.full(sd, -0.2)])
    return np.concatenate([inside, ref, edges, outside])


def main():
    rng = np.random.default_rng(5005)
    out = {}
    for sd in (1, 2, 3):
        pts = points(sd, rng, 4)
        out[f"pts_s{sd}"] = pts
        for n in range(1, 7):   # (the reference cannot build degree 0: its dual set has no entity for k = 0)
            out[f"tab_s{sd}_n{n}"] = stack(FIAT.Bernstein(FIAT.ufc_simplex(sd), n).tabulate(3, pts), sd, 3)
        for n in range(1, 5):
            ids = FIAT.Bernstein(FIAT.ufc_simplex(sd), n).entity_dofs()
            out[f"eids_s{sd}_n{n}"] = np.array([(d, e, i) for d in sorted(ids) for e in sorted(ids[d]) for i in ids[d][e]],
                                               dtype=np.int64).reshape(-1, 3)
    for name, sd, n in (("tet10", 3, 10), ("tri16", 2, 16)):
        pts = points(sd, rng, 2)
        out[f"hi_{name}_pts"] = pts
        out[f"hi_{name}"] = stack(FIAT.Bernstein(FIAT.ufc_simplex(sd), n).tabulate(1, pts), sd, 1)
    # entity=: points on a reference sub-entity (a facet and an edge)
    for sd, dim, entity in ((2, 1, 0), (2, 1, 2), (3, 2, 1), (3, 1, 4), (3, 2, 3)):
        e = rng.exponential(size=(4, dim + 1))
        sub = np.array(FIAT.ufc_simplex(dim).get_vertices(), dtype=float)
        spts = (e / e.sum(-1, keepdims=True)) @ sub
        key = f"ent_s{sd}_d{dim}_e{entity}"
        out[key + "_pts"] = spts
        out[key] = stack(FIAT.Bernstein(FIAT.ufc_simplex(sd), 3).tabulate(2, spts, entity=(dim, entity)), sd, 2)
    # the element built on physical simplices, at physical points
    for sd in (1, 2, 3):
        ref = np.array(FIAT.ufc_simplex(sd).get_vertices(), dtype=float)
        A = np.eye(sd) + 0.25 * rng.standard_normal((2, sd, sd))
        A[-1, :, 0] *= -1.0
        verts = np.einsum("vd,red->rve", ref, A) + rng.standard_normal((2, 1, sd))
        e = rng.exponential(size=(2, 5, sd + 1))
        ppts = np.einsum("rpv,rvd->rpd", e / e.sum(-1, keepdims=True), verts)
        out[f"phys_s{sd}_verts"], out[f"phys_s{sd}_pts"] = verts, ppts
        for n in (2, 4):
            for r in range(2):
                out[f"phys_s{sd}_n{n}_r{r}"] = stack(FIAT.Bernstein(physical(sd, verts[r]), n).tabulate(2, ppts[r]), sd, 2)
    # the reference's second-derivative test: P3 triangle at the degree-3 rule, order 2
    T = FIAT.ufc_simplex(2)
    qpts = np.array(create_quadrature(T, 3).get_points(), dtype=float)
    out["d2_pts"], out["d2_tab"] = qpts, stack(FIAT.Bernstein(T, 3).tabulate(2, qpts), 2, 2)
    # GLL lattice and pointwise-dual weights
    for name, sd, n in (("p2tri", 2, 2), ("p3tri", 2, 3), ("p2tet", 3, 2)):
        cell = FIAT.ufc_simplex(sd)
        lat = np.array(make_lattice(cell.get_vertices(), n, variant="gll"), dtype=float)
        index = {tuple(p): j for j, p in enumerate(lat)}
        W = np.zeros((len(lat), len(lat)))
        for i, node in enumerate(FIAT.Bernstein(cell, n).dual_basis()):
            for pt, wcs in node.get_point_dict().items():
                for w, _ in wcs:
                    W[i, index[tuple(pt)]] += w
        out[f"lat_{name}"], out[f"dualw_{name}"] = lat, W
    path = os.path.join(HERE, "bernstein.npz")
    np.savez_compressed(path, **out)
    print(len(out), "arrays ->", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
