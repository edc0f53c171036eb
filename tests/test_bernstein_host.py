"""Bernstein elements, host side (no GPU): the entity layout against the reference's fixture, the dof order, the fixture
itself against the formula restated here, and the new C ABI symbols of the built library."""
import math
import os

import numpy as np
import pytest

from fiat_amd import _lib, ufc_simplex
from fiat_amd.bernstein import bernstein_entity_ids
from fiat_amd.polynomial_set import mis

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "bernstein.npz"))


def formula(sd, n, order, pts):
    """Tables (ntab, ndof, npts) of the Bernstein basis on the UFC simplex, straight from the definition (the exact
    n!-scaled value where the derivative order equals the degree)."""
    pts = np.asarray(pts, dtype=float)
    lam = np.concatenate([1.0 - pts.sum(1, keepdims=True), pts], axis=1)          # (npts, sd+1)
    Gm = np.concatenate([-np.ones((1, sd)), np.eye(sd)])                           # d lambda_i / d x_d
    rows = []
    for o in range(order + 1):
        for alpha in mis(sd, o):
            dirs = [d for d, a in enumerate(alpha) for _ in range(a)]
            tab = np.zeros((math.comb(n + sd, sd), len(pts)))
            for i, ks in enumerate(mis(sd + 1, n)):
                for seq in np.ndindex(*(sd + 1,) * o):
                    beta = np.bincount(np.array(seq, dtype=int), minlength=sd + 1) if o else np.zeros(sd + 1, int)
                    e = np.array(ks) - beta
                    if (e < 0).any():
                        continue
                    w = np.prod([Gm[s, d] for s, d in zip(seq, dirs)])
                    c = math.factorial(n) / np.prod([math.factorial(int(x)) for x in e])
                    tab[i] += w * c * np.prod(lam ** e, axis=1)
            rows.append(tab)
    return np.stack(rows)


def reference_corrected(tab, sd, n, order):
    """The reference's tables with its order == degree entries scaled by n! (the deliberate deviation)."""
    tab = tab.copy()
    t = 0
    for o in range(order + 1):
        for _ in mis(sd, o):
            if o == n and n >= 2:
                tab[t] *= math.factorial(n)
            t += 1
    return tab


@pytest.mark.parametrize("sd", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_entity_ids_match_reference(sd, n):
    ids = bernstein_entity_ids(ufc_simplex(sd), n)
    rows = sorted((d, e, i) for d in ids for e in ids[d] for i in ids[d][e])
    assert rows == sorted(map(tuple, G[f"eids_s{sd}_n{n}"].tolist()))


def test_degree_zero_layout():
    ids = bernstein_entity_ids(ufc_simplex(2), 0)
    assert ids[2][0] == [0] and not any(ids[d][e] for d in (0, 1) for e in ids[d])


@pytest.mark.parametrize("sd", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 3, 6])
def test_dof_order_is_mis(sd, n):
    """At vertex v exactly the dof with ks = n e_v is 1: its position in the fixture's rows is its position in mis."""
    vals = G[f"tab_s{sd}_n{n}"][0][:, 4:4 + sd + 1]      # value table at the sd+1 vertex points
    ks = mis(sd + 1, n)
    for v in range(sd + 1):
        corner = tuple(n if i == v else 0 for i in range(sd + 1))
        expect = np.zeros(len(ks))
        expect[ks.index(corner)] = 1.0
        assert np.array_equal(vals[:, v], expect)


@pytest.mark.parametrize("sd", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 2, 4, 6])
def test_partition_of_unity_in_fixture(sd, n):
    tab = G[f"tab_s{sd}_n{n}"]
    inside = slice(0, 4 + sd + 1 + 2)                 # interior, vertices, edges (the last two points are outside)
    assert np.allclose(tab[0][:, inside].sum(0), 1.0, atol=1e-13)
    assert np.allclose(tab[1:1 + sd].sum(1), 0.0, atol=1e-11)


@pytest.mark.parametrize("sd,n", [(1, 2), (1, 3), (2, 2), (2, 3), (3, 2), (3, 3), (1, 5), (2, 4)])
def test_formula_matches_reference(sd, n):
    """The restated formula (used by the GPU tests) against the reference, with the order == degree correction."""
    ref = reference_corrected(G[f"tab_s{sd}_n{n}"], sd, n, 3)
    got = formula(sd, n, 3, G[f"pts_s{sd}"])
    assert np.abs(got - ref).max() <= 1e-10 * max(1.0, np.abs(ref).max())


def test_reference_order_equals_degree_deviation():
    """The reference returns 1 (not n!) where the order equals the degree: pinned here so the correction stays honest."""
    tab = G["tab_s1_n2"]
    assert np.allclose(tab[2][:, 0], [1.0, -2.0, 1.0])
    assert np.allclose(formula(1, 2, 2, G["pts_s1"][:1])[2][:, 0], [2.0, -4.0, 2.0])
    assert np.allclose(G["tab_s1_n3"][3][:, 0], [-1.0, 3.0, -3.0, 1.0])


def test_c_abi_symbols():
    for name in ("fx_bernstein_tabulate_batch", "fx_bernstein_tabulate_shared"):
        assert name in _lib.EXPORTS
        assert getattr(_lib.lib, name) is not None
    header = open(os.path.join(ROOT, "include", "fiat_amd.h")).read()
    assert "int fx_bernstein_tabulate_batch(" in header and "int fx_bernstein_tabulate_shared(" in header
    assert _lib.lib.fx_abi_version() == 2


def test_registry():
    import fiat_amd
    assert fiat_amd.supported_elements["Bernstein"] is fiat_amd.Bernstein
    assert not fiat_amd.Bernstein.is_nodal()
