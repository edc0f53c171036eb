"""Host side of the edge tests (no GPU): the references of tests/edge_reference.py against the reference's fixtures
(tests/golden/bernstein.npz, hdivcurl.npz) and against exact rational arithmetic, the constants and route mirrors against
the launchers, and the coverage of the GPU edge tests' shape lists: together they must reach every route category."""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import edge_reference as R  # noqa: E402
import make_golden_hdivcurl as M  # noqa: E402

GB = np.load(os.path.join(HERE, "golden", "bernstein.npz"))
GH = R.hdivcurl_fixture()
rel = R.rel


def corrected(tab, sd, n, order):
    tab = np.array(tab, dtype=float)
    t = 0
    for o in range(order + 1):
        for _ in R.multi_indices(sd, o):
            if o == n and n >= 2:
                tab[t] *= math.factorial(n)
            t += 1
    return tab


def test_ordering_is_mis():
    from fiat_amd.polynomial_set import mis
    for m in (1, 2, 3, 4):
        for n in range(0, 9):
            assert R.multi_indices(m, n) == [tuple(a) for a in mis(m, n)]


# ---- Bernstein reference against the fixtures -----------------------------------------------------------------------

@pytest.mark.parametrize("sd", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6])
def test_bernstein_fixture(sd, n):
    ref = R.bernstein_reference(sd, n, 3, GB[f"pts_s{sd}"][None])[0]
    assert rel(ref, corrected(GB[f"tab_s{sd}_n{n}"], sd, n, 3)) <= 1e-13


@pytest.mark.parametrize("name,sd,n", [("tet10", 3, 10), ("tri16", 2, 16)])
def test_bernstein_fixture_high_degree(name, sd, n):
    assert rel(R.bernstein_reference(sd, n, 1, GB[f"hi_{name}_pts"][None])[0], GB[f"hi_{name}"]) <= 1e-13


@pytest.mark.parametrize("sd", [1, 2, 3])
@pytest.mark.parametrize("n", [2, 4])
def test_bernstein_fixture_physical_cells(sd, n):
    verts, pts = GB[f"phys_s{sd}_verts"], GB[f"phys_s{sd}_pts"]
    ref = R.bernstein_reference(sd, n, 2, pts, verts=verts)
    for r in range(len(verts)):
        assert rel(ref[r], corrected(GB[f"phys_s{sd}_n{n}_r{r}"], sd, n, 2)) <= 1e-13


def test_bernstein_fixture_second_derivatives():
    assert rel(R.bernstein_reference(2, 3, 2, GB["d2_pts"][None])[0], GB["d2_tab"]) <= 1e-13


def test_bernstein_shared_equals_per_request_cells():
    rng = np.random.default_rng(1)
    verts = R.random_cells(rng, 4, 3)
    ref_pts = R.simplex_points(rng, (6,), 3)
    phys = np.einsum("pv,rvd->rpd", np.concatenate([1 - ref_pts.sum(-1, keepdims=True), ref_pts], -1), verts)
    a = R.bernstein_reference(3, 4, 3, ref_pts, verts=verts, shared=True)
    b = R.bernstein_reference(3, 4, 3, phys, verts=verts)
    assert rel(a, b) <= 1e-15


# ---- long double against exact rationals ------------------------------------------------------------------------------

EXACT = [(1, 3, 3, "own"), (1, 16, 8, "own"), (2, 8, 8, "own"), (2, 16, 3, "cells"), (3, 3, 3, "own"), (3, 8, 4, "cells"),
         (3, 16, 1, "own"), (3, 4, 4, "shared"), (2, 5, 4, "cells")]


@pytest.mark.parametrize("sd,n,order,mode", EXACT)
def test_long_double_equals_fraction(sd, n, order, mode):
    rng = np.random.default_rng(sd * 100 + n)
    verts = R.random_cells(rng, 1, sd)[0] if mode != "own" else None
    if verts is not None and mode == "cells":
        verts = verts.copy()
        verts[[0, 1]] = verts[[1, 0]]                    # a negatively oriented cell
    for k in range(2):
        x = R.simplex_points(rng, (1,), sd, -0.1)[0]
        if mode == "cells":
            x = verts[0] + (verts[1:] - verts[0]).T @ x
        ld = R.bernstein_reference(sd, n, order, x[None] if mode == "shared" else x[None, None],
                                   verts=None if verts is None else verts[None], shared=mode == "shared")[0, :, :, 0]
        ex = R.bernstein_exact(sd, n, order, x, verts=verts, shared=mode == "shared")
        assert R.rel_to_exact(ld, ex) <= 1e-15, (k, R.rel_to_exact(ld, ex))


def test_line_lagrange_equals_fraction():
    from fractions import Fraction
    nodes = np.array([0.0, 1.0, 1 / 3, 2 / 3, 0.1])
    x = np.array([-0.1, 0.37, 1.1])
    ld = R.line_lagrange_reference(nodes, x, 4)
    N = [Fraction(float(v)) for v in nodes]
    for j, xj in enumerate(x):
        X = Fraction(float(xj))
        for i in range(len(N)):
            # exact polynomial coefficients by repeated multiplication, then derivatives
            coef = [Fraction(1)]
            den = Fraction(1)
            for m, nm in enumerate(N):
                if m == i:
                    continue
                coef = [a - nm * b for a, b in zip([Fraction(0)] + coef, coef + [Fraction(0)])]
                den *= N[i] - nm
            for k in range(5):
                d = sum(c * math.perm(p, k) * X ** (p - k) for p, c in enumerate(coef) if p >= k) / den
                assert abs(Fraction(*ld[k, i, j].as_integer_ratio()) - d) <= Fraction(1, 10 ** 15) * max(1, abs(d))


# ---- H(div) / H(curl) reference against the fixture, through the descriptor --------------------------------------------

@pytest.mark.parametrize("name", M.QUADHEX)
def test_hdivcurl_fixture(name):
    sd, kind, cn, dn, offsets, signs = R.fixture_descriptor(name, GH)
    pts = GH[f"{name}_pts"]
    ref = R.hdivcurl_reference(kind, cn, dn, offsets, signs, sd, M.max_order(name), pts[None])[0]
    tab = GH[f"{name}_tab"]
    assert rel(ref[0], tab[0]) <= 1e-13
    assert rel(ref, tab) <= 1e-12
    nz = ref != 0
    assert np.array_equal(nz.any(-1).any(0), (tab != 0).any(-1).any(0))      # the same nonzero component of every dof


def test_grid_points_row_major():
    g = np.arange(2 * 3 * 4, dtype=float).reshape(2, 3, 4)
    p = R.grid_points(g)
    assert p.shape == (2, 64, 3)
    assert np.array_equal(p[1, 4 * 4 * 1 + 4 * 2 + 3], [g[1, 0, 1], g[1, 1, 2], g[1, 2, 3]])


# ---- constants and mirrors --------------------------------------------------------------------------------------------

def test_constants():
    assert R.C == {"BERN_MAXN": 16, "BERN_SPEC_MAXN": 6, "BERN_IMAGE_BYTES": 48 * 1024, "BERN_MAX_ORDER": 8,
                   "BERN_MAX_ORDER_CELLS": 4, "HDC_IMAGE_BYTES": 40 * 1024, "HDC_MAXK_QUAD": 4, "HDC_MAXK_HEX": 3,
                   "HDC_MAX_ORDER": 2}
    assert len(R.bern_spec_instances()) == 63 and len(R.hdc_instances()) == 84


def test_mirrors_hand_checked():
    # P3 tetrahedra, order 1, 23 points: P = 2, 4 x 20 x 23 doubles a request, image of 29 440 B
    r = R.bern_route(3, 3, 1, 23, False, 1001, 256)
    assert (r["spec"], r["P"], r["reqsize"], r["image"], r["nitems"], r["last"]) == (True, 2, 1840, True, 501, 1)
    assert r["grid"] == 501 and not r["stride"] and r["copies"] == {"flush"}
    # generic, per-request cells, tetrahedra order 4: 798 coefficients a request, 48 KB hold 7
    r = R.bern_route(3, 4, 4, 1, True, 15, 256)
    assert (r["spec"], r["P"], r["image"], r["nitems"], r["gridcap"]) == (False, 7, False, 3, 2048) and r["p_by_lds"]
    # 65 points: one request in two chunks, the second partial
    r = R.bern_route(2, 3, 1, 65, False, 4, 256)
    assert (r["P"], r["chunks"], r["partial_chunk"], r["nitems"]) == (1, 2, True, 4)
    # odd request (7 doubles) with P = 9: every item odd
    assert R.bern_route(1, 0, 0, 7, False, 19, 256)["copies"] == {"scalar"}
    # H(div): RTCF2 on quadrilaterals, order 1, 9 points: 12 dofs, 3 x 12 x 2 x 9 doubles, P = 7, 36 288 B <= 40 KB
    r = R.hdc_route(2, 2, 1, 0, 2, 9, 15, 256)
    assert (r["P"], r["reqsize"], r["image"]) == (7, 648, True)
    assert not R.hdc_route(2, 2, 2, 0, 2, 9, 15, 256)["image"]            # order 2: 6 tables, 72 576 B
    r = R.hdc_route(2, 1, 0, 0, 2, 16, 10 ** 6, 256)
    assert r["stride"] and r["grid"] == 256 * 64 and r["copies"] == {"flush"}
    assert R.hdc_route(2, 1, 0, 0, 2, 16, 9, 256, offset=1)["copies"] == {"scalar"}


# ---- coverage of the GPU shape lists ----------------------------------------------------------------------------------

def _bern_routes():
    cu = R.MI355X_CU
    out = [R.bern_route(sd, n, o, p, False, q, cu) for sd, n, o, p, q in R.BERN_CENSUS + R.BERN_GENERIC_OWN]
    for sd, n, o, p, mode in R.BERN_GENERIC_CELLS:
        P = R.bern_route(sd, n, o, p, True, 1, cu)["P"]
        out.append(R.bern_route(sd, n, o, p, True, 3 * P + 2, cu))
    for sd, n, o in R.BERN_POINT_SHAPES:
        for p in R.POINT_COUNTS:
            for cells in (False, True):
                P = R.bern_route(sd, n, o, p, cells, 1, cu)["P"]
                out += [R.bern_route(sd, n, o, p, cells, q, cu) for q in R.nreq_list(P)]
    for sd, n, o, p in R.BERN_IMAGE_EDGE + R.BERN_ODD_SHAPES:
        P = R.bern_route(sd, n, o, p, False, 1, cu)["P"]
        out += [R.bern_route(sd, n, o, p, False, q, cu) for q in (P, 3 * P + 1)]
    out += [R.bern_route(sd, n, o, p, m != "own", q, cu) for sd, n, o, p, m, q in R.bern_grid_stride_cases(cu)]
    for sd, n, o, p, q, m in R.GUARD_BERN:
        out += [R.bern_route(sd, n, o, p, m != "own", q, cu, offset=off) for off in R.OFFSETS]
    return out


def _hdc_routes():
    cu = R.MI355X_CU
    out = []

    def add(name, order, npts, nreq, grid=False, offset=0):
        kind, sd, K, nb = R.hdc_descriptor_of(name)
        out.append(R.hdc_route(sd, K, order, kind, nb, npts ** sd if grid else npts, nreq, cu, grid=grid, offset=offset))
    for name, order, grid, npts, nreq in R.HDC_CENSUS:
        add(name, order, npts, nreq, grid)
    for name, order in R.HDC_POINT_ELEMENTS:
        for p in R.POINT_COUNTS:
            P = 64 // p if p <= 64 else 1
            for q in R.nreq_list(P):
                add(name, order, p, q)
    for sd, (name, order) in R.HDC_GRID_ELEMENTS.items():
        for qq in R.HDC_GRID_Q[sd]:
            p = qq ** sd
            P = 64 // p if p <= 64 else 1
            for q in R.nreq_list(P):
                add(name, order, qq, q, grid=True)
    for name, order, p in R.HDC_IMAGE_EDGE:
        P = 64 // p if p <= 64 else 1
        for q in (P, 3 * P + 1):
            add(name, order, p, q)
    for name, order, p, off in R.HDC_OFFSET_SHAPES:
        P = 64 // p if p <= 64 else 1
        for q in (P, 3 * P + 1):
            add(name, order, p, q, offset=off)
    for name, order, p, q in R.hdc_grid_stride_cases(cu):
        add(name, order, p, q)
    for name, order, grid, p, q in R.GUARD_HDC:
        for off in R.OFFSETS:
            add(name, order, p, q, grid=grid, offset=off)
    return out


def _categories(routes):
    cats = set()
    for r in routes:
        cats.add("image" if r["image"] else "stream")
        cats.add("P>1" if r["P"] > 1 else ("P=1 partial chunk" if r["partial_chunk"] else "P=1 one chunk"))
        cats.add("last partial" if r["last_partial"] else "last full")
        cats.add("stride" if r["stride"] else "no stride")
        cats.update(r["copies"])
    return cats


ALL = {"image", "stream", "P>1", "P=1 one chunk", "P=1 partial chunk", "last partial", "last full", "stride", "no stride",
       "flush", "scalar"}


def test_bernstein_shapes_cover_every_route():
    routes = _bern_routes()
    assert _categories(routes) == ALL, ALL - _categories(routes)
    instances = {r["instance"] for r in routes}
    assert {("spec",) + i for i in R.bern_spec_instances()} <= instances
    assert {("generic", sd) for sd in (1, 2, 3)} <= instances
    assert any(r["p_by_lds"] for r in routes)
    lim = R.C["BERN_IMAGE_BYTES"]
    assert any(r["item_bytes"] == lim and r["image"] for r in routes)                  # exactly at the LDS image limit
    assert any(r["spec"] and not r["image"] and r["partial_chunk"] and r["item_bytes"] - lim <= 1024 for r in routes)
    # the generic instance's own grid cap: crossed on the element's cell and with cells
    assert {r["instance"][0] for r in routes if r["stride"]} == {"spec", "generic"}


def test_hdivcurl_shapes_cover_every_route():
    routes = _hdc_routes()
    assert _categories(routes) == ALL, ALL - _categories(routes)
    assert {r["instance"] for r in routes} >= set(R.hdc_instances())
    lim = R.C["HDC_IMAGE_BYTES"]
    assert any(r["item_bytes"] == lim and r["image"] for r in routes)                  # exactly at the LDS image limit
    assert any(not r["image"] and r["item_bytes"] - lim <= 1024 for r in routes)
    assert any(r["instance"][4] and r["P"] == 1 and r["partial_chunk"] for r in routes)     # grid input, q**sd > 64
