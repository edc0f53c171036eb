"""Every kernel that leaves its tables through store.hpp flush_block, and one shape per simplex kernel family, into an
``out`` view at 0, 1, 7 and 8 doubles past a 128-byte line inside a NaN-filled buffer (tests/edge_reference.py guarded_out):
the guards stay bit-identical, every entry of out is written, nothing is NaN, and the tables equal the same call into a
fresh tensor (the arithmetic is the same; only the store path differs)."""
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

BERN, HDC = R.GUARD_BERN, R.GUARD_HDC          # shape lists of edge_reference.py (the host test checks their routes)
launched, compare = R.launched, R.compare      # (shared with tests/test_gpu_instances.py)


def only_kernel(names, family):
    """Exactly one kernel of the call is of ``family`` (a name such as "fxk::tensor_small_kernel")."""
    hits = [n for n in names if family + "<" in n]
    assert len(hits) == 1, (family, sorted(names))


def pts_simplex(rng, nreq, npts, sd):
    e = rng.exponential(size=(nreq, npts, sd + 1))
    return (e / e.sum(-1, keepdims=True))[..., 1:].copy()


cells = R.random_cells


@pytest.mark.parametrize("sd,n,order,npts,nreq,mode", BERN)
def test_bernstein(sd, n, order, npts, nreq, mode):
    import torch
    from fiat_amd import Bernstein, ufc_simplex
    el = Bernstein(ufc_simplex(sd), n)
    rng = np.random.default_rng(npts + nreq)
    dev = torch.device("cuda", torch.cuda.current_device())
    shape = el.out_shape(order, nreq, npts)
    if mode == "own":
        pts = pts_simplex(rng, nreq, npts, sd)
        got = compare(lambda o: el.tabulate_batch(order, pts, out=o), shape, dev)
        ref = R.bernstein_reference(sd, n, order, pts)
    elif mode == "cells":
        verts = cells(rng, nreq, sd)
        pts = np.einsum("rpv,rvd->rpd", np.concatenate([1 - (x := pts_simplex(rng, nreq, npts, sd)).sum(-1, keepdims=True), x], -1), verts)
        got = compare(lambda o: el.tabulate_batch(order, pts, verts=verts, out=o), shape, dev)
        ref = R.bernstein_reference(sd, n, order, pts, verts=verts)
    else:
        verts = cells(rng, nreq, sd)
        pts = pts_simplex(rng, 1, npts, sd)[0]
        got = compare(lambda o: el.tabulate_cells(order, pts, verts, out=o), shape, dev)
        ref = R.bernstein_reference(sd, n, order, pts, verts=verts, shared=True)
    got = got.cpu().numpy()
    ref = np.asarray(ref, dtype=float)
    assert np.abs(got - ref).max() <= 1e-10 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("name,order,grid,npts,nreq", HDC)
def test_hdivcurl_fused(name, order, grid, npts, nreq, monkeypatch):
    import torch
    import fiat_amd
    from fiat_amd import hdivcurl, runtime

    def refuse(*args, **kwargs):
        raise AssertionError("the general route was taken")
    monkeypatch.setattr(runtime, "table_place", refuse)
    el = M.build(fiat_amd, name)
    sd = el.get_reference_element().get_spatial_dimension()
    rng = np.random.default_rng(npts + nreq)
    if grid:
        g = torch.as_tensor(rng.uniform(-0.1, 1.1, size=(nreq, sd, npts))).cuda()
        shape = tuple(el.tabulate_batch(order, g, grid=True).shape)
        got = compare(lambda o: el.tabulate_batch(order, g, grid=True, out=o), shape, g.device)
        pts = R.grid_points(g.cpu().numpy())
    else:
        pts = rng.uniform(-0.1, 1.1, size=(nreq, npts, sd))
        shape = tuple(el.tabulate_batch(order, pts).shape)
        got = compare(lambda o: el.tabulate_batch(order, pts, out=o), shape, torch.device("cuda", torch.cuda.current_device()))
    sd_, kind, cn, dn, offsets, signs = hdivcurl.fused_descriptor(el)
    ref = np.asarray(R.hdivcurl_reference(kind, cn, dn, offsets, signs, sd, order, pts), dtype=float)
    assert np.abs(got.cpu().numpy() - ref).max() <= 1e-10 * max(1.0, np.abs(ref).max())


def test_general_placement():
    import torch
    import fiat_amd
    from fiat_amd import hdivcurl
    el = M.build(fiat_amd, "pdiv1d0")
    rng = np.random.default_rng(3)
    e = rng.exponential(size=(4, 17, 3))
    pts = np.concatenate([(e / e.sum(-1, keepdims=True))[..., 1:], rng.uniform(0, 1, size=(4, 17, 1))], -1)
    shape = tuple(hdivcurl.tabulate_general(el, 1, pts).shape)
    compare(lambda o: hdivcurl.tabulate_general(el, 1, pts, out=o), shape, torch.device("cuda", torch.cuda.current_device()))


# degree -> (factors, order, points) with a lane-local tensor instance: Q1-Q3 on quadrilaterals, Q1 and (values) Q2 on
# hexahedra; 8 points make every request an even number of doubles (the flush_block branch), 9 points on quadrilaterals
# an odd one where the node count is odd (the copy loop)
TENSOR_SMALL = {1: [(2, 1, 8), (2, 1, 9), (3, 1, 8)], 2: [(2, 1, 8), (2, 1, 9), (3, 0, 8)], 3: [(2, 1, 8), (2, 1, 9)]}


@pytest.mark.parametrize("deg", [1, 2, 3])
def test_tensor_small(deg):
    """Tensor-product Lagrange factors of degree ``deg`` on the lane-local tensor kernel (tensor_small.hpp)."""
    import torch
    from fiat_amd import runtime
    L = runtime.LineLagrange(np.linspace(0.0, 1.0, deg + 1))
    rng = np.random.default_rng(deg)
    for nf, order, npts in TENSOR_SMALL[deg]:
        pts = rng.uniform(0, 1, size=(37, npts, nf))
        total = R.ntables(nf, order) * (deg + 1) ** nf * npts
        assert npts == 9 or total % 2 == 0
        only_kernel(launched(lambda: runtime.tensor_tabulate_batch([L] * nf, order, pts)), "fxk::tensor_small_kernel")
        shape = tuple(runtime.tensor_tabulate_batch([L] * nf, order, pts).shape)
        compare(lambda o: runtime.tensor_tabulate_batch([L] * nf, order, pts, out=o), shape,
                torch.device("cuda", torch.cuda.current_device()))


def test_prism_small():
    import torch
    import fiat_amd
    from fiat_amd import runtime
    tri = fiat_amd.Lagrange(fiat_amd.ufc_simplex(2), 2).device_polyset()
    line = runtime.LineLagrange(np.array([0.0, 1.0, 0.5]))
    rng = np.random.default_rng(5)
    e = rng.exponential(size=(29, 7, 3))
    pts = np.concatenate([(e / e.sum(-1, keepdims=True))[..., 1:], rng.uniform(0, 1, size=(29, 7, 1))], -1)
    res = runtime.prism_tabulate_batch(tri, line, 1, pts)
    assert res is not None and int(np.prod(res.shape[1:])) % 2 == 0          # an even request: the flush_block branch
    only_kernel(launched(lambda: runtime.prism_tabulate_batch(tri, line, 1, pts)), "fxk::prism_small_kernel")
    compare(lambda o: runtime.prism_tabulate_batch(tri, line, 1, pts, out=o), tuple(res.shape),
            torch.device("cuda", torch.cuda.current_device()))


def test_macro_small():
    import torch
    import fiat_amd
    el = fiat_amd.Lagrange(fiat_amd.ufc_simplex(2), 2, "equispaced,alfeld")
    ps = el.device_polyset()
    nreq, npts = 41, 7
    assert ps.kernel_name(1, nreq, npts) == "fxk::tabulate_macro_small", ps.kernel_name(1, nreq, npts)
    pts = pts_simplex(np.random.default_rng(8), nreq, npts, 2)
    compare(lambda o: ps.tabulate_batch(1, pts, out=o), ps.out_shape(1, nreq, npts),
            torch.device("cuda", torch.cuda.current_device()))


def _polyset(golden, which):
    """The P3 tetrahedron of the policy tests, or the DG P6 tetrahedron of the cooperative kernel's registry."""
    from fiat_amd import runtime
    g = golden("elements")
    if which == "dg6":
        return runtime.SimplexPolySet(3, 6, coeffs=g["c4_dg6tet_q6_coeffs"])
    return runtime.SimplexPolySet(3, 3, variant="bubble", scale=1, coeffs=g["c2_p3tet_q6_coeffs"])


# (policy, order, nreq, npts, cells, kernel name) on the P3 tetrahedron (the cooperative kernel: DG P6)
SIMPLEX = [((), 1, 257, 23, False, "fxk::tabulate_simplex_pair"),
           (("kernel_stream",), 1, 257, 23, False, "fxk::tabulate_simplex_stream"),
           (("kernel_image",), 1, 257, 23, False, "fxk::tabulate_simplex_fixed"),
           (("no_fixed", "no_stacked", "no_wg"), 1, 257, 23, False, "fxk::tabulate_simplex_coop"),
           (("no_fixed", "no_stacked", "no_coop", "no_small"), 1, 257, 23, False, "fxk::tabulate_simplex_kernel"),
           ((), 1, 1000, 7, False, "fxk::tabulate_simplex_kernel"),
           ((), 1, 1000, 40, False, "fxk::tabulate_simplex_stacked"),
           ((), 1, 1000, 130, False, "fxk::tabulate_simplex_stacked"),
           ((), 2, 1000, 23, True, "fxk::tabulate_simplex_stacked"),
           ((), 1, 1000, 100, False, "fxk::tabulate_simplex_wg")]


@pytest.mark.parametrize("policy,order,nreq,npts,has_cells,kernel", SIMPLEX, ids=[f"{s[5].split('_')[-1]}-{s[3]}pt" for s in SIMPLEX])
def test_simplex_kernels(policy, order, nreq, npts, has_cells, kernel, golden, kernel_policy):
    import torch
    ps = _polyset(golden, "dg6" if kernel.endswith("coop") else "p3")
    kernel_policy(*policy)
    assert ps.kernel_name(order, nreq, npts, has_verts=has_cells) == kernel
    rng = np.random.default_rng(npts + order)
    pts = pts_simplex(rng, nreq, npts, 3)
    verts = cells(rng, nreq, 3) if has_cells else None
    compare(lambda o: ps.tabulate_batch(order, pts, verts=verts, out=o), ps.out_shape(order, nreq, npts),
            torch.device("cuda", torch.cuda.current_device()))


@pytest.mark.parametrize("family,sd,degree,npts,order,nreq,kernel", [
    ("Lagrange", 2, 5, 12, 0, 515, "fxk::tabulate_simplex_small"),
    ("Lagrange", 2, 5, 7, 0, 515, "fxk::tabulate_simplex_small"),
    ("Lagrange", 3, 5, 14, 0, 517, "fxk::tabulate_simplex_wg")])
def test_simplex_small_and_grouped_wg(family, sd, degree, npts, order, nreq, kernel):
    import torch
    import fiat_amd as fa
    el = getattr(fa, family)(fa.ufc_simplex(sd), degree)
    ps = el.device_polyset()
    assert ps.kernel_name(order, nreq, npts) == kernel
    if kernel.endswith("small"):
        # simplex_small.hpp flushes through flush_block for an even request (21 x 12 doubles) and copies odd ones (21 x 7)
        reqsize = int(np.prod(ps.out_shape(order, 1, npts)[1:]))
        assert reqsize % 2 == (npts % 2)
    if kernel.endswith("wg"):
        assert ps.kernel_name(order, nreq, npts, instance=True).endswith("x9")          # several requests per workgroup
    pts = pts_simplex(np.random.default_rng(npts), nreq, npts, sd)
    compare(lambda o: ps.tabulate_batch(order, pts, out=o), ps.out_shape(order, nreq, npts),
            torch.device("cuda", torch.cuda.current_device()))


SHARED = {(): "fxk::shared_points_wave_kernel", ("no_shared_wave",): "fxk::shared_points_reg_kernel",
          ("no_shared_reg", "no_shared_wave"): "fxk::shared_points_kernel"}


@pytest.mark.parametrize("policy", list(SHARED))
def test_batch_shared_kernels(policy, kernel_policy):
    """The three kernels behind tabulate_batch_shared (wave per request, register-resident, one workgroup per request)."""
    import torch
    import fiat_amd as fa
    el = fa.Lagrange(fa.ufc_simplex(3), 3)
    ps = el.device_polyset()
    kernel_policy(*policy)
    rng = np.random.default_rng(len(policy))
    ref_pts = pts_simplex(rng, 1, 23, 3)[0]
    verts = cells(rng, 301, 3)
    only_kernel(launched(lambda: ps.tabulate_batch_shared(1, ref_pts, verts)), SHARED[policy])
    compare(lambda o: ps.tabulate_batch_shared(1, ref_pts, verts, out=o), ps.out_shape(1, 301, 23),
            torch.device("cuda", torch.cuda.current_device()))
