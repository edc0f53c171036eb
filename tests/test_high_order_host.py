"""Derivative orders 7 and 8 without a GPU: the references the device tests of tests/test_gpu_high_order.py stand on.

1. The exact rational evaluation (tests/high_order_reference.py: equispaced Lagrange in the monomial basis, integer arithmetic,
   points as exact binary doubles) against tests/golden/high_order.npz, <= 1e-13: P8 on the triangle directly; the ON sets on
   the interval (degree 10) and the tetrahedron (degree 8) as the exact P10 / P8 tables contracted with the set's values at the
   lattice nodes.  The fixture is the unmodified reference's output, so this bounds the reference's own error.
2. oracle/fiat_oracle.py at orders 7 and 8 against every fixture array, <= 1e-13: the GPU tests use the oracle at points the
   fixture does not hold.
3. The chain-rule reference (one matrix per order and cell, brute force over ordered source directions) against the literal
   formula of tests/test_gpu_round4.py, and -- through the fixture's reference-cell arrays -- against the reference's Lagrange
   element built ON the physical cells, at the standing tolerances (1e-12 values, 1e-10 derivatives).
4. A NumPy restatement of table_mix_any_kernel with mix_any_order's index tables: as written it reproduces the reference's P8 on
   the physical cells; with CMAX 9 -> 8 for SD 2 or first[7] moved by one it misses the tolerance the device tests apply.

Every error is max|x - ref| / max(1, max|ref| over the tables of that order)."""
import itertools
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import high_order_reference as H  # noqa: E402

ORDER = H.MAX_ORDER


def _show(tag, errs):
    print(f"{tag}: worst {max(errs):.2e}  per order " + " ".join(f"{e:.1e}" for e in errs))


def _coeffs(golden, name):
    """(coefficients, scale, variant) of a fixture case for the oracle."""
    from oracle import fiat_oracle as fo
    sd, degree, _ = H.CASES[name]
    if name == "p8tri":
        return fo.lagrange_coeffs(fo.UFC_SIMPLEX[sd], degree)[0], 1, "bubble"
    if name == "rt8tri":
        return golden("high_order")["ho_rt8tri_coeffs"], None, None
    return np.eye(len(H.jet(sd, degree))), None, None


def test_exact_lagrange_is_nodal():
    """The helper itself: L_i(node_j) = delta_ij exactly, and the degree-8 derivatives of the vertex function of P8 are the
    closed form 8^8 / 8! * 8! (d^8 / dx^8 of prod_{k < 8} (8 x - k) / 8!)."""
    for sd, n in ((1, 10), (2, 8)):
        nodes = np.array(H.lattice_numerators(sd, n), dtype=float)[:, 1:]          # numerators: the nodes are these / n
        exps, C, den = H.lagrange_monomial_coefficients(sd, n)
        # u = n x is the numerator itself: integers throughout
        V = np.array([[int(np.prod([int(u) ** e for u, e in zip(row, ex)])) for ex in exps] for row in nodes.astype(int)], dtype=object)
        got = V.dot(C)
        want = np.zeros_like(got)
        for i in range(len(den)):
            want[i, i] = den[i]
        assert (got == want).all()
    tab = H.lagrange_exact_tables(2, 8, 8, np.array([[0.25, 0.125]]), as_fractions=True)
    first = int(H.firsts(2, 8)[8])
    assert tab[first][1][0] == Fraction(8 ** 8) and tab[first + 8][2][0] == Fraction(8 ** 8)     # vertices (1, 0) and (0, 1)


@pytest.mark.parametrize("name", ["on10int", "p8tri", "on8tet"])
def test_fixture_against_the_exact_rational_evaluation(golden, name):
    from oracle import fiat_oracle as fo
    g = golden("high_order")
    sd, degree, _ = H.CASES[name]
    values = None
    if name != "p8tri":        # the ON set's coefficients in the Lagrange basis: its values at the lattice nodes
        nodes = np.array(H.lattice_numerators(sd, degree), dtype=float)[:, 1:] / degree
        values = fo.expansion_tabulate(fo.UFC_SIMPLEX[sd], degree, nodes, 0)[(0,) * sd]
    for r in range(2):
        hi, lo = H.lagrange_exact_tables(sd, degree, ORDER, g[f"ho_{name}_refpts"][r])
        want = hi if values is None else H.on_set_from_lagrange(values, hi, lo)
        errs = H.order_errors(g[f"ho_{name}_o8_ref{r}"], want, sd, ORDER)
        _show(f"{name} cell {r}, fixture against exact", errs)
        assert max(errs) <= H.TOL_EXACT, (name, r, errs)


@pytest.mark.parametrize("name", list(H.CASES))
@pytest.mark.parametrize("order", [7, 8])
def test_oracle_at_orders_7_and_8_against_the_fixture(golden, name, order):
    g = golden("high_order")
    sd, degree, _ = H.CASES[name]
    coeffs, scale, variant = _coeffs(golden, name)
    for r in range(2):
        got = H.oracle_tables(sd, degree, coeffs, order, g[f"ho_{name}_refpts"][r], scale, variant)
        errs = H.order_errors(got, H.truncate(g[f"ho_{name}_o8_ref{r}"], sd, order), sd, order)
        _show(f"{name} cell {r} order {order}, oracle against fixture", errs)
        assert max(errs) <= H.TOL_EXACT, (name, r, errs)


def _chain_rule_tables_literal(ref_tab, sd, order, Kt):
    """The formula of _chain_rule_tables in tests/test_gpu_round4.py, term by term."""
    keys = H.jet(sd, order)
    pos = {a: i for i, a in enumerate(keys)}
    out = []
    for alpha in keys:
        dirs = [d for d, m in enumerate(alpha) for _ in range(m)]
        acc = 0.0
        for src in itertools.product(range(sd), repeat=len(dirs)):
            beta = tuple(src.count(c) for c in range(sd))
            acc = acc + float(np.prod([Kt[c, d] for c, d in zip(src, dirs)])) * ref_tab[pos[beta]]
        out.append(acc)
    return np.stack(out)


@pytest.mark.parametrize("sd,order", [(1, 8), (2, 5), (3, 4)])
def test_chain_rule_matrices_are_the_literal_sum(sd, order):
    rng = np.random.default_rng(sd)
    Kt = np.eye(sd) + 0.3 * rng.standard_normal((sd, sd))
    tab = rng.standard_normal((H.ntables(sd, order), 3, 2))
    got = H.chain_rule_apply(H.chain_rule_matrices(sd, order, Kt), tab, sd, order)
    want = _chain_rule_tables_literal(tab, sd, order, Kt)
    assert max(H.order_errors(got, want, sd, order)) <= 1e-14


@pytest.mark.parametrize("order", [7, 8])
def test_chain_rule_reference_against_elements_built_on_the_physical_cells(golden, order):
    """P8 triangle: the reference's element built on each physical cell (incl. the negatively oriented one) equals the chain rule
    applied to its reference-cell tables."""
    g = golden("high_order")
    for r in range(2):
        ref_tab = H.truncate(g[f"ho_p8tri_o8_ref{r}"], 2, order)
        got = H.chain_rule_tables(ref_tab, 2, order, g["ho_p8tri_verts"][r])
        errs = H.assert_close(got, H.truncate(g[f"ho_p8tri_o8_phys{r}"], 2, order), 2, order, ("p8tri", r))
        _show(f"p8tri cell {r} order {order}, chain rule against the element on the physical cell", errs)


def test_chain_rule_matrices_in_three_dimensions_compose():
    """Order 8 in 3-D (45 x 45, 6561 ordered tuples a row): the chain rule through two cells in a row is the chain rule of the
    composed map, M_k(K1 K2) = M_k(K2) M_k(K1)."""
    rng = np.random.default_rng(8)
    K1, K2 = (np.eye(3) + 0.2 * rng.standard_normal((3, 3)) for _ in range(2))
    A, B, AB = (H.chain_rule_matrices(3, ORDER, K) for K in (K1, K2, K1 @ K2))
    for k in range(ORDER + 1):
        assert np.abs(B[k] @ A[k] - AB[k]).max() <= 1e-12 * max(1.0, np.abs(AB[k]).max()), k


# ---- a NumPy restatement of table_mix_any_kernel<SD> with mix_any_order's index tables (csrc/table_kernels.hpp, csrc/api.hip) -----
def _mix_any_restatement(tab, sd, order, K, cmax, first_shift_at=None):
    """In place over the tables as the kernel does it: first[] / cnt[] per order, M_k from M_{k-1} through lead[] (first non-zero
    entry of alpha_t) and down[][] (alpha - e_c within the previous order), ``cmax`` tables of one order in registers.
    ``first_shift_at``: first[k] moved by one, the fault the device tests must catch."""
    mis = [H.mis(sd, k) for k in range(order + 1)]
    first, cnt, t = [0] * (order + 1), [1] * (order + 1), 1
    for k in range(1, order + 1):
        first[k], cnt[k] = t, len(mis[k])
        t += cnt[k]
    if first_shift_at is not None:
        first[first_shift_at] += 1

    def down(k, alpha, c):
        beta = list(alpha)
        beta[c] -= 1
        return mis[k - 1].index(tuple(beta))
    M = [np.ones((1, 1))]
    for k in range(1, order + 1):
        Mk = np.zeros((cnt[k], cnt[k]))
        for ti, alpha in enumerate(mis[k]):
            d = next(i for i, a in enumerate(alpha) if a)          # lead[]
            tp = down(k, alpha, d)
            for si, gamma in enumerate(mis[k]):
                Mk[ti, si] = sum(K[c, d] * (M[k - 1][tp, down(k, gamma, c)] if k > 1 else 1.0) for c in range(sd) if gamma[c] > 0)
        M.append(Mk)
    out = np.array(tab, dtype=float, copy=True)
    ntab = out.shape[0]
    for k in range(1, order + 1):
        regs = [out[first[k] + s].copy() if s < cnt[k] and first[k] + s < ntab else 0.0 for s in range(cmax)]
        for ti in range(cnt[k]):
            acc = 0.0
            for s in range(min(cmax, cnt[k])):
                acc = acc + M[k][ti, s] * regs[s]
            if first[k] + ti < ntab:                                # (the restatement stays inside its array; the kernel would not)
                out[first[k] + ti] = acc
    return out


@pytest.mark.parametrize("order", [7, 8])
def test_restated_mixing_kernel_and_the_faults_the_device_tests_catch(golden, order):
    """The kernel as written reproduces the reference's P8 triangle on the physical cells.  With CMAX 9 -> 8 for SD 2 (the ninth table
    of order 8 never enters the sum) or first[7] moved by one, the same comparison -- the one tests/test_gpu_high_order.py makes in
    test_cells_against_the_reference -- misses the 1e-10 tolerance by orders of magnitude at the order the fault touches."""
    g = golden("high_order")
    worst = {"as written": 0.0, "CMAX 8": 0.0, "first[7] + 1": 0.0}
    for r in range(2):
        ref_tab = H.truncate(g[f"ho_p8tri_o8_ref{r}"], 2, order)
        want = H.truncate(g[f"ho_p8tri_o8_phys{r}"], 2, order)
        K = H.cell_jacobian_inverse(g["ho_p8tri_verts"][r])
        for tag, kw in (("as written", dict(cmax=9)), ("CMAX 8", dict(cmax=8)), ("first[7] + 1", dict(cmax=9, first_shift_at=7))):
            errs = H.order_errors(_mix_any_restatement(ref_tab, 2, order, K, **kw), want, 2, order)
            worst[tag] = max(worst[tag], max(errs[1:]))
    print(f"order {order}: " + ", ".join(f"{k}: {v:.2e}" for k, v in worst.items()))
    assert worst["as written"] <= H.TOL_DER
    assert worst["first[7] + 1"] > 1e3 * H.TOL_DER
    if order == 8:
        assert worst["CMAX 8"] > 1e3 * H.TOL_DER
    else:
        assert worst["CMAX 8"] <= H.TOL_DER          # order 7 holds 8 tables: only order 8 fills the register file
