"""Fused H(div) / H(curl) kernel (csrc/hdivcurl.hpp, launcher hdivcurl.hip) at its tiling edges, against the long-double
product-formula reference of tests/edge_reference.py built from hdivcurl.fused_descriptor: all 84 instances (kind x
cell x K x order x points / grid), point counts and grid sizes around 64, items at the LDS image limit and above, odd item
sizes, grids that the items exceed, flipped block signs, exact zeros off the blocks; and the general placement route
(prisms, orders 3-4, a scalar enriched element) through a NaN-filled guarded output.  Norm max|x - ref| / max(1, max|ref|):
1e-12 values, 1e-10 derivatives.  The shape lists are those of tests/edge_reference.py, which
tests/test_edge_reference_host.py runs through the launcher mirror."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import edge_reference as R  # noqa: E402
import make_golden_hdivcurl as M  # noqa: E402

TOL_VAL, TOL_DER = 1e-12, 1e-10


# the shape lists live in edge_reference.py, where the host test runs them through the launcher mirror
name_of, descriptor_of, nreq_list = R.hdc_name, R.hdc_descriptor_of, R.nreq_list
CENSUS, POINT_COUNTS, POINT_ELEMENTS = R.HDC_CENSUS, R.POINT_COUNTS, R.HDC_POINT_ELEMENTS
GRID_Q, GRID_ELEMENTS, IMAGE_EDGE, OFFSET_SHAPES = R.HDC_GRID_Q, R.HDC_GRID_ELEMENTS, R.HDC_IMAGE_EDGE, R.HDC_OFFSET_SHAPES
grid_stride_cases = R.hdc_grid_stride_cases


# ---------------------------------------------------------------------------------------------------------------------

_ELS = {}


def element(name):
    import fiat_amd
    if name not in _ELS:
        _ELS[name] = M.build(fiat_amd, name)
    return _ELS[name]


def reference(el, order, pts):
    from fiat_amd import hdivcurl
    sd, kind, cn, dn, offsets, signs = hdivcurl.fused_descriptor(el)
    return R.hdivcurl_reference(kind, cn, dn, offsets, signs, sd, order, pts)


def rel_check(got, ref, what=""):
    got, ref = np.asarray(got, dtype=float), np.asarray(ref, dtype=float)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    for r in range(len(ref)):
        e0 = np.abs(got[r, 0] - ref[r, 0]).max() / max(1.0, np.abs(ref[r, 0]).max())
        assert e0 <= TOL_VAL, (what, r, "values", e0)
        if ref.shape[1] > 1:
            e1 = np.abs(got[r, 1:] - ref[r, 1:]).max() / max(1.0, np.abs(ref[r, 1:]).max())
            assert e1 <= TOL_DER, (what, r, "derivatives", e1)


def off_block_zeros(out, el):
    """Every component outside a dof's block is an exact zero (the block of each dof from the descriptor)."""
    import torch
    from fiat_amd import hdivcurl
    sd, kind, cn, dn, offsets, signs = hdivcurl.fused_descriptor(el)
    nb = R.hdc_nb(sd, len(dn), kind)
    for c in range(sd):
        if offsets[c] < 0:
            continue
        rows = out[:, :, offsets[c]:offsets[c] + nb]
        others = [e for e in range(sd) if e != c]
        assert bool((rows[:, :, :, others] == 0).all()), ("nonzero off-block component", c)
    assert bool(torch.isfinite(out).all())


def no_general(monkeypatch):
    from fiat_amd import runtime

    def refuse(*args, **kwargs):
        raise AssertionError("the general route was taken")
    monkeypatch.setattr(runtime, "table_place", refuse)


def run(name, order, npts, nreq, rng, grid=False, sample=None):
    """Fused tabulation of ``nreq`` requests (points in [-0.1, 1.1]; grid: npts = q per direction), ``sample`` against
    the reference, off-block zeros everywhere."""
    import torch
    el = element(name)
    sd = el.get_reference_element().get_spatial_dimension()
    if grid:
        g = rng.uniform(-0.1, 1.1, size=(nreq, sd, npts))
        out = el.tabulate_batch(order, torch.as_tensor(g).cuda(), grid=True)
        pts = R.grid_points(g)
    else:
        pts = rng.uniform(-0.1, 1.1, size=(nreq, npts, sd))
        out = el.tabulate_batch(order, pts)
    torch.cuda.synchronize()
    idx = np.arange(nreq) if sample is None else sample
    got = out[torch.as_tensor(idx, device=out.device)].cpu().numpy()
    rel_check(got, reference(el, order, pts[idx]), (name, order, npts, nreq, grid))
    off_block_zeros(out, el)
    return out


@pytest.mark.parametrize("name", M.QUADHEX)
def test_descriptor_and_reference_against_fixture(name):
    """hdivcurl.fused_descriptor of every quad / hex fixture element == the descriptor read off the fixture, and the
    reference built from it reproduces the reference's tables."""
    from fiat_amd import hdivcurl
    GH = R.hdivcurl_fixture()
    sd, kind, cn, dn, offsets, signs = hdivcurl.fused_descriptor(element(name))
    fsd, fkind, fcn, fdn, foffsets, fsigns = R.fixture_descriptor(name, GH)
    assert (sd, kind, tuple(offsets)) == (fsd, fkind, foffsets)
    assert tuple(s for s, o in zip(signs, offsets) if o >= 0) == tuple(s for s, o in zip(fsigns, foffsets) if o >= 0)
    assert np.array_equal(cn, fcn) and np.array_equal(dn, fdn)
    ref = R.hdivcurl_reference(kind, cn, dn, offsets, signs, sd, M.max_order(name), GH[f"{name}_pts"][None])[0]
    assert R.rel(ref, GH[f"{name}_tab"]) <= 1e-12


@pytest.mark.parametrize("name,order,grid,npts,nreq", CENSUS, ids=[f"{c[0]}-o{c[1]}-{'grid' if c[2] else 'pts'}" for c in CENSUS])
def test_instance_census(name, order, grid, npts, nreq, monkeypatch):
    no_general(monkeypatch)
    run(name, order, npts, nreq, np.random.default_rng(order * 7 + npts + len(name)), grid=grid)


@pytest.mark.parametrize("kind,sd", [(0, 2), (1, 2), (0, 3), (1, 3)])
def test_every_sign_pattern(kind, sd):
    """The runtime entry with every sign pattern of the blocks (the elements use -1 on component 0 of H(div) only)."""
    import itertools
    import torch
    from fiat_amd import hdivcurl, runtime
    el = element(name_of(kind, sd, 2))
    _, _, cn, dn, offsets, _ = hdivcurl.fused_descriptor(el)
    C, D = runtime.LineLagrange(cn), runtime.LineLagrange(dn)
    rng = np.random.default_rng(kind + sd)
    pts = rng.uniform(-0.1, 1.1, size=(5, 9, sd))
    for signs in itertools.product((1, -1), repeat=sd):
        out = runtime.hdivcurl_tabulate_batch(sd, kind, C, D, offsets, signs, 2, pts)
        torch.cuda.synchronize()
        rel_check(out.cpu().numpy(), R.hdivcurl_reference(kind, cn, dn, offsets, signs, sd, 2, pts), signs)


@pytest.mark.parametrize("npts", POINT_COUNTS)
@pytest.mark.parametrize("name,order", POINT_ELEMENTS)
def test_point_counts(name, order, npts, monkeypatch):
    no_general(monkeypatch)
    kind, sd, K, nb = descriptor_of(name)
    P = R.hdc_route(sd, K, order, kind, nb, npts, 1, R.MI355X_CU)["P"]
    for nreq in nreq_list(P):
        run(name, order, npts, nreq, np.random.default_rng(npts * 13 + nreq))


@pytest.mark.parametrize("sd,q", [(sd, q) for sd in (2, 3) for q in GRID_Q[sd]])
def test_grid_sizes(sd, q, monkeypatch):
    no_general(monkeypatch)
    name, order = GRID_ELEMENTS[sd]
    kind, _, K, nb = descriptor_of(name)
    P = R.hdc_route(sd, K, order, kind, nb, q ** sd, 1, R.MI355X_CU)["P"]
    for nreq in nreq_list(P):
        run(name, order, q, nreq, np.random.default_rng(q * 17 + nreq), grid=True)


@pytest.mark.parametrize("name,order,npts", IMAGE_EDGE)
def test_image_boundary(name, order, npts, monkeypatch):
    no_general(monkeypatch)
    kind, sd, K, nb = descriptor_of(name)
    P = R.hdc_route(sd, K, order, kind, nb, npts, 1, R.MI355X_CU)["P"]
    for nreq in (P, 3 * P + 1):
        run(name, order, npts, nreq, np.random.default_rng(npts + nreq))


@pytest.mark.parametrize("name,order,npts,offset", OFFSET_SHAPES)
def test_offset_out_takes_the_copy_loop(name, order, npts, offset, monkeypatch):
    """An out at an 8-byte offset: the image leaves through the scalar copy loop; guards untouched, every entry written,
    tables equal to a fresh out and to the reference."""
    import torch
    no_general(monkeypatch)
    kind, sd, K, nb = descriptor_of(name)
    P = R.hdc_route(sd, K, order, kind, nb, npts, 1, R.MI355X_CU)["P"]
    el = element(name)
    for nreq in (P, 3 * P + 1):
        pts = np.random.default_rng(npts + nreq).uniform(-0.1, 1.1, size=(nreq, npts, sd))
        fresh = el.tabulate_batch(order, pts)
        buf, out = R.guarded_out(tuple(fresh.shape), offset, fresh.device)
        el.tabulate_batch(order, pts, out=out)
        torch.cuda.synchronize()
        R.check_guarded(buf, out)
        assert torch.equal(out, fresh)
        rel_check(out.cpu().numpy(), reference(el, order, pts), (name, nreq))


def test_grid_stride(monkeypatch):
    import torch
    no_general(monkeypatch)
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    for name, order, npts, nreq in grid_stride_cases(num_cu):
        kind, sd, K, nb = descriptor_of(name)
        r = R.hdc_route(sd, K, order, kind, nb, npts, nreq, num_cu)
        assert r["nitems"] >= 2 * r["gridcap"]
        sample = R.sample_requests(nreq, r["P"], nitems_per_trip=r["grid"], k=16, seed=npts)
        out = run(name, order, npts, nreq, np.random.default_rng(nreq), sample=sample)
        del out


# ---------------------------------------------------------------------------------------------------------------------
# general route through a guarded output

GENERAL = [("pdiv1d0", 1), ("pcurl1d0", 2), ("rtcf2d0", 3), ("rtcf2d0", 4), ("scal1d0", 2)]


@pytest.mark.parametrize("npts", [1, 65, 129])
@pytest.mark.parametrize("name,order", GENERAL)
def test_general_route_guarded(name, order, npts):
    """table_place_kernel writes every row of the output only if the leaves tile them: a NaN-filled out catches a row
    that is never written; quadrilateral cases against the reference."""
    import torch
    from fiat_amd import hdivcurl
    el = element(name)
    sd = el.get_reference_element().get_spatial_dimension()
    rng = np.random.default_rng(npts + order)
    if name.startswith(("pdiv", "pcurl")):           # prisms: triangle x interval
        e = rng.exponential(size=(3, npts, 3))
        tri = (e / e.sum(-1, keepdims=True))[..., 1:]
        pts = np.concatenate([tri, rng.uniform(0, 1, size=(3, npts, 1))], -1)
    elif name.startswith("scal"):
        e = rng.exponential(size=(3, npts, 3))
        pts = (e / e.sum(-1, keepdims=True))[..., 1:].copy()
    else:
        pts = rng.uniform(-0.1, 1.1, size=(3, npts, sd))
    fresh = hdivcurl.tabulate_general(el, order, pts)
    for off in R.OFFSETS:
        buf, out = R.guarded_out(tuple(fresh.shape), off, fresh.device)
        hdivcurl.tabulate_general(el, order, pts, out=out)
        torch.cuda.synchronize()
        R.check_guarded(buf, out)
        assert torch.equal(out, fresh)
    if name.startswith("rtcf"):
        rel_check(fresh.cpu().numpy(), reference(el, order, pts), name)
