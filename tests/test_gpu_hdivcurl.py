"""Hdiv / Hcurl / EnrichedElement on the HIP path: the reference's tables (tests/golden/hdivcurl.npz) through tabulate and
tabulate_batch at 1e-12 for values and 1e-10 for derivatives, the route each element takes (fused kernel for the quad / hex
families at orders 0-2, general placement route otherwise), fused against general on random batches, grid input, the
façade's errors and metadata, and two full-size batches against the NumPy restatement of tests/test_hdivcurl_host.py."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import make_golden_hdivcurl as M  # noqa: E402

G = np.load(os.path.join(ROOT, "tests", "golden", "hdivcurl.npz"))
TOL_VAL, TOL_DER = 1e-12, 1e-10


def check_tables(got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape
    assert np.abs(got[0] - ref[0]).max() <= TOL_VAL * max(1.0, np.abs(ref[0]).max())
    if len(ref) > 1:
        assert np.abs(got[1:] - ref[1:]).max() <= TOL_DER * max(1.0, np.abs(ref[1:]).max())


def keys(sd, order):
    from fiat_amd.polynomial_set import mis
    return [a for k in range(order + 1) for a in mis(sd, k)]


def build(name):
    import fiat_amd
    return M.build(fiat_amd, name)


def order_of(name):
    return M.max_order(name) if name in M.QUADHEX else 2


@pytest.mark.parametrize("name", M.QUADHEX + M.OTHERS)
def test_parity_tabulate(name):
    el = build(name)
    pts = G[f"{name}_pts"]
    order = order_of(name)
    sd = pts.shape[1]
    tab = el.tabulate(order, pts)
    check_tables(np.stack([tab[a] for a in keys(sd, order)]), G[f"{name}_tab"])
    batch = el.tabulate_batch(order, pts[None]).cpu().numpy()[0]
    check_tables(batch, G[f"{name}_tab"])


@pytest.mark.parametrize("name", M.QUADHEX + M.OTHERS)
def test_metadata(name):
    from fiat_amd.tensor_product import FlattenedDimensions
    el = build(name)
    assert np.array_equal(M.metadata(el), G[f"{name}_meta"])
    assert np.array_equal(M.eids_rows(el.entity_dofs()), G[f"{name}_eids"])
    assert np.array_equal(M.dual_codes(el), G[f"{name}_dual"])
    if name in M.QUADHEX:
        assert np.array_equal(M.eids_rows(FlattenedDimensions(el).entity_dofs()), G[f"{name}_feids"])


def _no_general(monkeypatch):
    from fiat_amd import runtime

    def refuse(*args, **kwargs):
        raise AssertionError("the general route was taken")
    monkeypatch.setattr(runtime, "table_place", refuse)


@pytest.mark.parametrize("name", M.QUADHEX)
def test_fused_route(name, monkeypatch):
    el = build(name)
    pts = G[f"{name}_pts"]
    _no_general(monkeypatch)
    for order in (0, 1, 2):
        check_tables(el.tabulate_batch(order, pts[None]).cpu().numpy()[0], G[f"{name}_tab"][:len(keys(pts.shape[1], order))])


@pytest.mark.parametrize("name", ["pdiv1d0", "rotcurl1d0", "scal1d0", "rtcf1d0"])
def test_general_route(name, monkeypatch):
    from fiat_amd import runtime
    el = build(name)
    pts = G[f"{name}_pts"]
    order = 3 if name.startswith("rtcf") else 1
    calls = []
    real = runtime.table_place
    monkeypatch.setattr(runtime, "table_place", lambda *a, **k: calls.append(1) or real(*a, **k))
    out = el.tabulate_batch(order, pts[None]).cpu().numpy()[0]
    assert calls
    check_tables(out, G[f"{name}_tab"][:len(out)])


def test_entity_tabulation(monkeypatch):
    from fiat_amd.tensor_product import FlattenedDimensions
    quad, hexa, nce = build("rtcf2d0"), build("ncf2d0"), build("nce1d0")
    q, f2 = G["ent_p1"], G["ent_p2"]

    def stack(tab, sd, order):
        return np.stack([tab[a] for a in keys(sd, order)])
    for e in range(4):
        check_tables(stack(FlattenedDimensions(quad).tabulate(1, q, entity=(1, e)), 2, 1), G[f"ent_rtcf_flat_e{e}"])
    check_tables(stack(quad.tabulate(1, q, entity=((1, 0), 1)), 2, 1), G["ent_rtcf_prod_10_1"])
    check_tables(stack(FlattenedDimensions(hexa).tabulate(1, f2, entity=(2, 1)), 3, 1), G["ent_ncf_flat_f1"])
    check_tables(stack(FlattenedDimensions(hexa).tabulate(1, q, entity=(1, 4)), 3, 1), G["ent_ncf_flat_e4"])
    check_tables(stack(hexa.tabulate(1, f2, entity=(((1, 0), 1), 1)), 3, 1), G["ent_ncf_prod_f"])
    check_tables(stack(FlattenedDimensions(nce).tabulate(2, f2, entity=(2, 3)), 3, 2), G["ent_nce_flat_f3"])


@pytest.mark.parametrize("name,order", [("rtcf1d0", 0), ("rtcf2s1", 1), ("rtce3d0", 2), ("rtcf4", 1), ("rtce4", 2),
                                        ("ncf1d0", 2), ("ncf2d0", 1), ("nce2s1", 0), ("nce3d0", 1), ("sdivz2d0", 2)])
def test_fused_equals_general(name, order):
    """1 000 random requests: the fused kernel against the general route called directly; grid input against points."""
    import torch
    from fiat_amd import hdivcurl
    if name in ("rtcf4", "rtce4"):
        import fiat_amd
        from fiat_amd.reference_element import UFCInterval
        I, T = UFCInterval(), fiat_amd.TensorProductElement
        CG, DG = (lambda n: fiat_amd.Lagrange(I, n)), (lambda n: fiat_amd.DiscontinuousLagrange(I, n))
        W = fiat_amd.Hdiv if name == "rtcf4" else fiat_amd.Hcurl
        el = fiat_amd.EnrichedElement(W(T(CG(4), DG(3))), W(T(DG(3), CG(4))))
    else:
        el = build(name)
    sd = el.get_reference_element().get_spatial_dimension()
    rng = np.random.default_rng(7)
    q = 3
    grid = rng.uniform(-0.1, 1.1, size=(1000, sd, q))
    idx = np.stack(np.meshgrid(*[np.arange(q)] * sd, indexing="ij"), -1).reshape(-1, sd)
    pts = np.stack([grid[:, d, idx[:, d]] for d in range(sd)], -1)
    fused = el.tabulate_batch(order, pts)
    general = hdivcurl.tabulate_general(el, order, pts)
    torch.cuda.synchronize()
    diff = (fused - general).abs().max().item()
    assert diff <= 1e-12 * max(1.0, general.abs().max().item())
    g = el.tabulate_batch(order, torch.as_tensor(grid).cuda(), grid=True)
    assert torch.equal(g, fused)


def test_facade_errors():
    import fiat_amd
    from fiat_amd.reference_element import UFCInterval
    I, T = UFCInterval(), fiat_amd.TensorProductElement
    CG, DG = fiat_amd.Lagrange(I, 1), fiat_amd.DiscontinuousLagrange(I, 0)
    with pytest.raises(NotImplementedError):
        fiat_amd.Hdiv(CG)
    with pytest.raises(ValueError):
        fiat_amd.Hdiv(T(CG, CG))              # form degree 0, not sd - 1
    with pytest.raises(ValueError):
        fiat_amd.Hcurl(T(DG, DG))             # form degree 2, not 1
    with pytest.raises(ValueError):
        fiat_amd.EnrichedElement(fiat_amd.Hdiv(T(CG, DG)), fiat_amd.Hcurl(T(CG, DG)))     # mappings differ
    with pytest.raises(ValueError):
        fiat_amd.EnrichedElement(CG, fiat_amd.Lagrange(fiat_amd.ufc_simplex(2), 1))      # cells differ
    el = build("rtcf2d0")
    assert isinstance(el.elements()[0], fiat_amd.TensorProductElement)
    for call in (el.get_nodal_basis, el.get_coeffs, el.dmats):
        with pytest.raises(NotImplementedError):
            call()
    with pytest.raises(NotImplementedError):
        el.get_num_members(1)
    assert el.get_formdegree() == 1 and el.get_order() == 1


def test_rotated_second_factor_is_refused():
    """Hdiv(TPE(interval element, covariant element on a triangle)): the reference's branch uses an unset Asd."""
    import fiat_amd
    from fiat_amd.reference_element import UFCInterval
    el = fiat_amd.Hcurl(fiat_amd.TensorProductElement(fiat_amd.Lagrange(UFCInterval(), 1),
                                                      fiat_amd.RaviartThomas(fiat_amd.ufc_simplex(2), 1)))
    with pytest.raises(NotImplementedError):
        el.tabulate(0, [(0.2, 0.3, 0.1)])


def test_ncf_by_hand_over_enriched_factor():
    """TensorProductElement over an enriched factor: Hdiv(TPE(RTCF, DG)) summand by summand equals NCF's rows."""
    import fiat_amd
    from fiat_amd.reference_element import UFCInterval
    I, T = UFCInterval(), fiat_amd.TensorProductElement
    rtcf = build("rtcf2d0")
    prod = T(rtcf, fiat_amd.DiscontinuousLagrange(I, 1))
    assert prod.value_shape() == (2,) and prod.space_dimension() == 24
    top = fiat_amd.Hdiv(prod)
    ncf = fiat_amd.EnrichedElement(top, fiat_amd.Hdiv(T(T(fiat_amd.DiscontinuousLagrange(I, 1), fiat_amd.DiscontinuousLagrange(I, 1)),
                                                        fiat_amd.Lagrange(I, 2))))
    pts = G["ncf2d0_pts"]
    check_tables(ncf.tabulate_batch(2, pts[None]).cpu().numpy()[0], G["ncf2d0_tab"][:10])
    inner = prod.tabulate_batch(1, pts[None]).cpu().numpy()[0]          # the plain product: vector A x scalar B
    ref = G["ncf2d0_tab"][:4, :24, :2]
    check_tables(inner, ref)


def _restated(el_name, order, pts):
    from test_hdivcurl_host import blocks_from_reference, kind_of, restated
    tab = G[f"{el_name}_tab"]
    starts, _ = blocks_from_reference(tab, pts.shape[1])
    blocks = {c: (off, -1 if kind_of(el_name) == "div" and c == 0 else 1) for c, off in starts.items()}
    return restated(kind_of(el_name), G[f"{el_name}_c"], G[f"{el_name}_d"], blocks, pts.shape[1], order, pts)


@pytest.mark.parametrize("name,nreq,shape", [("ncf2d0", 40_000, "hex27"), ("rtcf2d0", 400_000, "quad9")])
def test_full_size(name, nreq, shape):
    import torch
    el = build(name)
    sd = 3 if shape == "hex27" else 2
    q = 3
    gp = np.array([0.5 - 0.5 * np.sqrt(0.6), 0.5, 0.5 + 0.5 * np.sqrt(0.6)])
    ref_pts = np.stack(np.meshgrid(*[gp] * sd, indexing="ij"), -1).reshape(-1, sd)
    rng = np.random.default_rng(3)
    shift = rng.uniform(-0.05, 0.05, size=(nreq, 1, sd))
    pts = torch.as_tensor(ref_pts[None] + shift).cuda()
    out = el.tabulate_batch(1, pts)
    torch.cuda.synchronize()
    assert not torch.isnan(out).any()
    # off-block components are exact zeros: every dof row has one component with nonzeros
    nz = (out != 0).any(dim=-1).any(dim=1)            # (nreq, ndof, sd)
    assert int(nz.sum(dim=-1).max()) == 1
    for r in rng.choice(nreq, 8, replace=False):
        got = out[r].cpu().numpy()
        want = _restated(name, 1, pts[r].cpu().numpy())
        assert np.abs(got - want).max() <= 1e-10 * max(1.0, np.abs(want).max())
    del out
