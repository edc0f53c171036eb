"""``tabulate_on_cells``, host side (no GPU): the NumPy restatement of the Q1 cell map (tests/cellmap_reference.py) against the
reference's fixture (tests/golden/cellmap.npz), against central differences and against the div / curl identities; the host
entries of libfiat_amd_cellmap.so; and the companion library itself -- its symbols, header, code object, kernel set, scratch
and recorded resource usage -- with the kernel set and exports of libfiat_amd.so left as they were."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import cellmap_reference as R  # noqa: E402
import make_golden_cellmap as M  # noqa: E402

from fiat_amd import _lib  # noqa: E402

G = np.load(os.path.join(HERE, "golden", "cellmap.npz"))
COMPANION = os.path.join(ROOT, "fiat_amd", "csrc", "libfiat_amd_cellmap.so")
needs_llvm = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/clang-offload-bundler"),
                                reason="needs the LLVM tools of ROCm")
MAPS = (R.AFFINE, R.COVARIANT, R.CONTRAVARIANT)


# ---- the restatement against the fixture --------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [n for n, (_, mp) in M.CASES.items() if mp == "affine"])
def test_restatement_scalar_cases_against_fixture(name):
    """The unit-cell tables (the box tables with the box's constant chain rule undone) mapped onto the box's own vertices are
    the reference's tables of the element built on the box."""
    lo, hi, tab = G[f"{name}_lo"], G[f"{name}_hi"], G[f"{name}_tab"]
    sd = len(lo)
    unit = tab.copy()
    unit[1:] *= (hi - lo)[:, None, None]
    got = R.apply(np.zeros(sd), np.ones(sd), G[f"{name}_X"][None], R.unit_corners(sd, lo, hi)[None], unit[None])
    e0, e1 = R.errors(got, tab[None])
    print(f"{name}: values {e0:.2e} derivatives {e1:.2e}")
    assert e0 <= R.VALUES and e1 <= R.DERIVATIVES


@pytest.mark.parametrize("name", [n for n, (_, mp) in M.CASES.items() if mp != "affine"])
def test_restatement_vector_cases_against_fixture(name):
    """The reference's field on the box pushed to the fixture's cell: the restatement against the generator's own formulas."""
    mapping = R.MAPPINGS[M.CASES[name][1]]
    got = R.apply(G[f"{name}_lo"], G[f"{name}_hi"], G[f"{name}_x"][None], G[f"{name}_corners"][None], G[f"{name}_tab"][None], mapping)
    e0, e1 = R.errors(got, G[f"{name}_pushed"][None])
    print(f"{name}: values {e0:.2e} derivatives {e1:.2e}")
    assert e0 <= R.VALUES and e1 <= R.DERIVATIVES
    # the fixture can tell the mistakes apart: no Piola map at all, and the gradient M d_e Phi G without the d_e M terms
    lo, hi, x, V, tab = (G[f"{name}_{k}"] for k in ("lo", "hi", "x", "corners", "tab"))
    assert R.rel(R.apply(lo, hi, x[None], V[None], tab[None]), G[f"{name}_pushed"][None]) > 1e-2
    _, J, _, H = R.geometry(lo, hi, x[None], V[None])
    Mp, _ = R.piola(mapping, J, H)
    dropped = np.einsum("rpck,reikp,rped->rdicp", Mp, tab[None][:, 1:], np.linalg.inv(J))
    assert R.rel(dropped, G[f"{name}_pushed"][None][:, 1:]) > 1e-2


# ---- the restatement against central differences ------------------------------------------------------------------------

def quadratic_field(rng, sd):
    """A seeded quadratic vector field on the reference box and its gradient: Phi(X) (..., sd), dPhi(X) (..., sd, sd)[c, e]."""
    A, B, C = rng.standard_normal((sd, sd, sd)), rng.standard_normal((sd, sd)), rng.standard_normal(sd)
    phi = lambda X: np.einsum("cab,...a,...b->...c", A, X, X) + np.einsum("ca,...a->...c", B, X) + C               # noqa: E731
    dphi = lambda X: np.einsum("cab,...b->...ca", A, X) + np.einsum("cab,...a->...cb", A, X) + B                    # noqa: E731
    return phi, dphi


def field_tables(phi, dphi, X):
    """One dof: (nreq, 1 + sd, 1, sd, npts) reference tables of the field at X (nreq, npts, sd)."""
    v = np.moveaxis(phi(X), -1, 1)[:, None, None]                      # (nreq, 1, 1, sd, npts)
    d = np.moveaxis(dphi(X), (-1, -2), (1, 2))[:, :, None]             # (nreq, sd[e], 1, sd[c], npts)
    return np.concatenate([v, d], axis=1)


@pytest.mark.parametrize("sd", [2, 3])
@pytest.mark.parametrize("mapping", MAPS)
def test_restatement_against_central_differences(sd, mapping):
    """d phi / dx from the formulas against (phi(X + h e) - phi(X - h e)) / 2h chained through G, h = 1e-6 in reference
    coordinates, seeded quadratic fields on 40 perturbed cells (det J >= 0.39): bound 1e-7 (the differences' own truncation
    and rounding; 4e-10 measured)."""
    rng = np.random.default_rng(100 * sd + mapping)
    phi, dphi = quadratic_field(rng, sd)
    nreq, npts, h = 40, 5, 1e-6
    lo, hi = np.zeros(sd), np.ones(sd)
    V = R.perturbed_cells(rng, nreq, sd)
    X = rng.uniform(0.1, 0.9, size=(nreq, npts, sd))
    assert R.geometry(lo, hi, X, V)[2].min() >= 0.39
    got = R.apply(lo, hi, X, V, field_tables(phi, dphi, X), mapping)

    def value(Y):
        return R.apply(lo, hi, Y, V, field_tables(phi, dphi, Y)[:, :1], mapping)[:, 0]          # (nreq, 1, sd, npts)
    fd = np.stack([(value(X + h * np.eye(sd)[e]) - value(X - h * np.eye(sd)[e])) / (2 * h) for e in range(sd)], 1)
    Ginv = np.linalg.inv(R.geometry(lo, hi, X, V)[1])
    fd = np.einsum("reicp,rped->rdicp", fd, Ginv)
    err = np.abs(got[:, 1:] - fd).max()
    print(f"sd {sd} mapping {mapping}: {err:.2e}")
    assert err <= 1e-7


@pytest.mark.parametrize("sd", [2, 3])
def test_div_and_curl_identities(sd):
    """div_x (J Phi / det J) = div_X Phi / det J and curl_x (J^-T Phi) = J curl_X Phi / det J (the scalar curl_X Phi / det J
    in two dimensions), to 1e-13.  (Both also hold for M d_e Phi G alone -- a trace and an antisymmetric part are blind to the
    d_e M terms; the fixture and the central differences are what sees those.)"""
    rng = np.random.default_rng(7 + sd)
    phi, dphi = quadratic_field(rng, sd)
    lo, hi = np.zeros(sd), np.ones(sd)
    V = R.perturbed_cells(rng, 30, sd)
    X = rng.uniform(0.0, 1.0, size=(30, 6, sd))
    ref = field_tables(phi, dphi, X)
    _, J, det, _ = R.geometry(lo, hi, X, V)
    gX = np.swapaxes(np.moveaxis(ref[:, 1:, 0], 3, 1), 2, 3)          # [r, p, c, e] = d Phi_c / dX_e
    con = R.apply(lo, hi, X, V, ref, R.CONTRAVARIANT)
    gx = np.swapaxes(np.moveaxis(con[:, 1:, 0], 3, 1), 2, 3)           # [r, p, c, d]
    div_err = np.abs(np.trace(gx, axis1=2, axis2=3) - np.trace(gX, axis1=2, axis2=3) / det).max()
    cov = R.apply(lo, hi, X, V, ref, R.COVARIANT)
    gx = np.swapaxes(np.moveaxis(cov[:, 1:, 0], 3, 1), 2, 3)
    if sd == 2:
        curl_err = np.abs((gx[..., 1, 0] - gx[..., 0, 1]) - (gX[..., 1, 0] - gX[..., 0, 1]) / det).max()
    else:
        curl = lambda g: np.stack([g[..., 2, 1] - g[..., 1, 2], g[..., 0, 2] - g[..., 2, 0], g[..., 1, 0] - g[..., 0, 1]], -1)  # noqa: E731
        curl_err = np.abs(curl(gx) - np.einsum("rpab,rpb->rpa", J, curl(gX)) / det[..., None]).max()
    print(f"sd {sd}: div {div_err:.2e} curl {curl_err:.2e}")
    assert div_err <= 1e-13 and curl_err <= 1e-13


@pytest.mark.parametrize("sd", [2, 3])
@pytest.mark.parametrize("mapping", MAPS)
def test_identity_corners_change_nothing(sd, mapping):
    """The box's own vertices as corners: x = X, J = I, and the tables come back unchanged, to 1e-15."""
    rng = np.random.default_rng(sd)
    lo, hi = np.array([0.2, -1.0, 1.0])[:sd], np.array([0.7, 0.5, 3.0])[:sd]
    X = R.box_points(rng, 3, 8, lo, hi)
    tab = rng.standard_normal((3, 1 + sd, 5, sd, 8))
    corners = np.broadcast_to(R.unit_corners(sd, lo, hi), (3, 2 ** sd, sd))
    got = R.apply(lo, hi, X, corners, tab, mapping)
    err = R.rel(got, tab)
    print(f"sd {sd} mapping {mapping}: {err:.2e}")
    assert err <= 1e-15
    x, J, det, H = R.geometry(lo, hi, X, corners)
    assert np.abs(x - X).max() <= 1e-15 and np.abs(J - np.eye(sd)).max() <= 1e-15
    # the second derivatives of the map are exactly zero here; each is a sum of 2^sd terms v_i s s' / (h_d h_e) prod f that
    # cancel, so rounding leaves at most 2^sd eps max|v| / min(h)^2 (3.6e-15 for this quadrilateral, 2.1e-14 for the hexahedron)
    hbound = 2 ** sd * np.finfo(float).eps * np.abs(corners).max() / (hi - lo).min() ** 2
    print(f"max |H| {np.abs(H).max():.2e} (bound {hbound:.2e})")
    assert np.abs(H).max() <= hbound


@pytest.mark.parametrize("sd", [2, 3])
def test_contravariant_sign_follows_the_signed_determinant(sd):
    """Reflecting the cell (x_0 -> -x_0) flips det J: J / det J then leaves component 0 and flips the others, J^-T flips
    component 0 only."""
    rng = np.random.default_rng(11)
    lo, hi = np.zeros(sd), np.ones(sd)
    V = R.perturbed_cells(rng, 4, sd)
    Vr = V.copy()
    Vr[..., 0] *= -1.0
    X = rng.uniform(0, 1, size=(4, 5, sd))
    tab = rng.standard_normal((4, 1, 3, sd, 5))
    assert (R.geometry(lo, hi, X, V)[2] > 0).all() and (R.geometry(lo, hi, X, Vr)[2] < 0).all()
    a, b = R.apply(lo, hi, X, V, tab, R.CONTRAVARIANT), R.apply(lo, hi, X, Vr, tab, R.CONTRAVARIANT)
    flip = np.array([1.0] + [-1.0] * (sd - 1))[:, None]
    assert np.abs(b - a * flip).max() <= 1e-14
    a, b = R.apply(lo, hi, X, V, tab, R.COVARIANT), R.apply(lo, hi, X, Vr, tab, R.COVARIANT)
    assert np.abs(b[..., 0, :] + a[..., 0, :]).max() <= 1e-14 and np.abs(b[..., 1:, :] - a[..., 1:, :]).max() <= 1e-14


# ---- the host entries ----------------------------------------------------------------------------------------------------

def route(sd, nn, mapping, order, nrows, vdim, npts, grid=0):
    buf = ctypes.create_string_buffer(160)
    _lib.companion_check(_lib.cellmaplib.fx_cellmap_kernel(sd, nn, mapping, order, nrows, vdim, npts, grid, buf, 160))
    return buf.value.decode()


def test_route_report():
    assert route(2, 3, 0, 1, 0, 1, 9) == "fxk::cellmap_tensor_kernel<2,3,1,false> image P=7"
    assert route(2, 3, 0, 0, 0, 1, 64) == "fxk::cellmap_tensor_kernel<2,3,0,false> image P=1"
    assert route(2, 2, 0, 1, 0, 1, 1) == "fxk::cellmap_tensor_kernel<2,2,1,false> image P=64"
    assert route(3, 3, 0, 1, 0, 1, 9) == "fxk::cellmap_tensor_kernel<3,3,1,false> image P=5"       # 4 * 27 * 9 doubles a request
    assert route(3, 5, 0, 1, 0, 1, 5, 1) == "fxk::cellmap_tensor_kernel<3,5,1,true> stream P=1"      # Q4 hexahedra, 125 points
    assert route(2, 5, 0, 1, 0, 1, 3, 1) == "fxk::cellmap_tensor_kernel<2,5,1,true> image P=7"
    assert route(3, 0, 2, 1, 6, 3, 9) == "fxk::cellmap_apply_kernel<3,1,2> contravariant P=7"
    assert route(2, 0, 1, 0, 12, 2, 65) == "fxk::cellmap_apply_kernel<2,0,1> covariant P=1"
    assert route(2, 0, 0, 1, 8, 1, 130) == "fxk::cellmap_apply_kernel<2,1,0> affine P=1"


def test_host_entries_reject_bad_arguments():
    """FX_EINVAL (ValueError) and FX_ENOTIMPL (NotImplementedError); the launching entries check before they touch a device."""
    L = _lib.cellmaplib
    for bad in [(1, 0, 0, 1, 4, 1, 9), (4, 0, 0, 1, 4, 1, 9), (2, 0, -1, 1, 4, 1, 9), (2, 0, 0, -1, 4, 1, 9), (2, 0, 0, 1, -1, 1, 9),
                (2, 0, 0, 1, 4, 1, -9), (2, 0, 0, 1, 4, 3, 9), (3, 0, 0, 1, 4, 2, 9), (2, 0, 1, 1, 4, 1, 9), (3, 0, 2, 0, 4, 1, 9),
                (2, 3, 1, 1, 0, 2, 9), (2, 3, 0, 1, 0, 2, 9), (2, -1, 0, 1, 0, 1, 9)]:
        with pytest.raises(ValueError):
            route(*bad)
    with pytest.raises(ValueError, match="no buffer"):
        _lib.companion_check(L.fx_cellmap_kernel(2, 0, 0, 1, 4, 1, 9, 0, None, 0))
    with pytest.raises(NotImplementedError, match="order 2"):
        route(2, 0, 0, 2, 4, 1, 9)
    with pytest.raises(NotImplementedError, match="order 2"):
        route(2, 3, 0, 2, 0, 1, 9)
    with pytest.raises(NotImplementedError, match="mapping 3"):
        route(2, 0, 3, 1, 4, 2, 9)
    for nn in (1, 6):
        with pytest.raises(NotImplementedError, match=f"{nn} nodes"):
            route(2, nn, 0, 1, 0, 1, 9)
    with pytest.raises(ValueError, match="entries"):                 # 4 * 1000 * 3 * npts >= 2^31
        route(3, 0, 0, 1, 1000, 3, 200000)
    assert b"entries" in _lib.lib.fx_last_error()                    # one error slot for the main library and its companions
    with pytest.raises(ValueError, match="entries"):
        route(3, 5, 0, 1, 0, 1, 5000000)
    # grids of 2^31 points or more are refused before q^sd is formed (1290^3 < 2^31 <= 1291^3, 46340^2 < 2^31 <= 46341^2)
    for sd, q in [(3, 1291), (3, 2 ** 21), (3, 2 ** 31 - 1), (2, 46341), (2, 2 ** 31 - 1)]:
        with pytest.raises(ValueError, match="2\\^31 points"):
            route(sd, 5, 0, 0, 0, 1, q, 1)
        with pytest.raises(ValueError, match="2\\^31 points"):
            _lib.companion_check(L.fx_cellmap_tensor_grid_batch(None, sd, 5, None, None, None, 0, 1, q, None, None, None, None))
    with pytest.raises(ValueError, match="entries"):                 # the largest grids that fit: refused by the request bound
        route(3, 5, 0, 0, 0, 1, 1290, 1)
    assert route(2, 2, 0, 0, 0, 1, 1000, 1) == "fxk::cellmap_tensor_kernel<2,2,0,true> stream P=1"
    box = np.array([0.0, 0.0, 0.0]), np.array([1.0, 1.0, 1.0])
    p = _lib.host_ptr
    with pytest.raises(ValueError, match="null context"):
        _lib.companion_check(L.fx_cellmap_apply(None, 2, 0, 1, 1, 9, 4, 1, p(box[0]), p(box[1]), None, None, None, None, None))
    with pytest.raises(ValueError, match="null context"):
        _lib.companion_check(L.fx_cellmap_geometry(None, 2, p(box[0]), p(box[1]), 1, 9, None, None, None, None, None, None))
    with pytest.raises(ValueError, match="null context"):
        _lib.companion_check(L.fx_cellmap_tensor_batch(None, 2, 3, None, p(box[0]), p(box[1]), 1, 1, 9, None, None, None, None))
    with pytest.raises(ValueError, match="null context"):
        _lib.companion_check(L.fx_cellmap_tensor_grid_batch(None, 2, 3, None, p(box[0]), p(box[1]), 1, 1, 3, None, None, None, None))
    with pytest.raises(ValueError, match="negative grid"):
        _lib.companion_check(L.fx_cellmap_tensor_grid_batch(None, 2, 3, None, p(box[0]), p(box[1]), 1, 1, -3, None, None, None, None))


def test_python_refusals_that_need_no_device():
    from fiat_amd import cellmap
    from fiat_amd.reference_element import TensorProductCell, UFCHexahedron, UFCQuadrilateral, ufc_simplex
    assert [list(v) for v in cellmap.box_of(UFCQuadrilateral())[1:]] == [[0.0, 0.0], [1.0, 1.0]]
    assert cellmap.box_of(TensorProductCell(TensorProductCell(ufc_simplex(1), ufc_simplex(1)), ufc_simplex(1)))[0] == 3
    assert cellmap.box_of(UFCHexahedron())[0] == 3
    with pytest.raises(NotImplementedError, match=r"tabulate_batch\(verts=\)"):
        cellmap.box_of(ufc_simplex(2))
    with pytest.raises(NotImplementedError, match=r"tabulate_batch\(verts=\)"):
        cellmap.box_of(ufc_simplex(3))
    with pytest.raises(NotImplementedError, match="dimension 1"):
        cellmap.box_of(ufc_simplex(1))
    with pytest.raises(NotImplementedError, match="prisms"):
        cellmap.box_of(TensorProductCell(ufc_simplex(2), ufc_simplex(1)))
    import fiat_amd
    assert fiat_amd.tabulate_on_cells is cellmap.tabulate_on_cells and fiat_amd.cell_geometry_batch is cellmap.cell_geometry_batch


# ---- the companion library -----------------------------------------------------------------------------------------------

EXPECTED_EXPORTS = {"fx_cellmap_abi_version", "fx_cellmap_kernel", "fx_cellmap_geometry", "fx_cellmap_apply",
                    "fx_cellmap_tensor_batch", "fx_cellmap_tensor_grid_batch"}


def test_companion_symbols_and_abi():
    assert set(_lib.CELLMAP_EXPORTS) == EXPECTED_EXPORTS
    others = (_lib.lib, _lib.serlib, _lib.sflib, _lib.dpclib, _lib.tracelib, _lib.hierlib, _lib.evallib)
    for name in _lib.CELLMAP_EXPORTS:
        assert getattr(_lib.cellmaplib, name) is not None
        for other in others:
            assert not hasattr(other, name), f"{name} belongs to the cell-map companion"
    for exports in (_lib.EXPORTS, _lib.SER_EXPORTS, _lib.SF_EXPORTS, _lib.DPC_EXPORTS, _lib.TRACE_EXPORTS, _lib.HIER_EXPORTS,
                    _lib.EVAL_EXPORTS):
        assert set(_lib.CELLMAP_EXPORTS).isdisjoint(exports)
    assert _lib.cellmaplib.fx_cellmap_abi_version() == 1
    assert _lib.lib.fx_abi_version() == 2
    header = open(os.path.join(ROOT, "include", "fiat_amd_cellmap.h")).read()
    assert set(re.findall(r"^int (fx_\w+)\(", header, flags=re.M)) == EXPECTED_EXPORTS
    assert "fx_cellmap" not in open(os.path.join(ROOT, "include", "fiat_amd.h")).read()
    nm = shutil.which("nm")
    if nm is not None:
        syms = subprocess.run([nm, "-D", "--defined-only", COMPANION], check=True, capture_output=True, text=True).stdout
        exported = {line.split()[-1] for line in syms.splitlines() if " T " in line and line.split()[-1].startswith("fx_")}
        assert exported == EXPECTED_EXPORTS


def test_companion_needs_the_main_library():
    readelf = shutil.which("readelf")
    if readelf is None:
        pytest.skip("no readelf")
    dyn = subprocess.run([readelf, "-d", COMPANION], check=True, capture_output=True, text=True).stdout
    assert "[libfiat_amd.so]" in dyn and "$ORIGIN" in dyn


def test_header_is_plain_c99(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "abi_check.c"
    src.write_text('#include "fiat_amd_cellmap.h"\n'
                   "int main(void) {\n"
                   "    char buf[96];\n"
                   "    double lo[3] = {0, 0, 0}, hi[3] = {1, 1, 1};\n"
                   "    if (fx_cellmap_abi_version() != 1 || fx_abi_version() != 2) return 1;\n"
                   "    if (fx_cellmap_kernel(2, 3, FX_MAP_AFFINE, 1, 0, 1, 9, 0, buf, 96) != FX_OK) return 2;\n"
                   "    if (fx_cellmap_kernel(3, 0, FX_MAP_COVARIANT_PIOLA, 1, 12, 3, 9, 0, buf, 96) != FX_OK) return 3;\n"
                   "    if (fx_cellmap_apply(0, 2, FX_MAP_AFFINE, 1, 1, 9, 4, 1, lo, hi, 0, 0, 0, 0, 0) != FX_EINVAL) return 4;\n"
                   "    if (fx_cellmap_geometry(0, 2, lo, hi, 1, 9, 0, 0, 0, 0, 0, 0) != FX_EINVAL) return 5;\n"
                   "    if (fx_cellmap_tensor_batch(0, 2, 3, 0, lo, hi, 1, 1, 9, 0, 0, 0, 0) != FX_EINVAL) return 6;\n"
                   "    if (fx_cellmap_tensor_grid_batch(0, 2, 3, 0, lo, hi, 1, 1, 3, 0, 0, 0, 0) != FX_EINVAL) return 7;\n"
                   "    return fx_cellmap_kernel(2, 0, FX_MAP_AFFINE, 2, 4, 1, 9, 0, buf, 96) == FX_ENOTIMPL ? 0 : 8;\n"
                   "}\n")
    inc = os.path.join(ROOT, "include")
    lib = os.path.join(ROOT, "fiat_amd", "csrc")
    exe = tmp_path / "abi_check"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{inc}", str(src), f"-L{lib}",
                    "-lfiat_amd_cellmap", "-lfiat_amd", f"-Wl,-rpath,{lib}", "-o", str(exe)], check=True, capture_output=True)
    assert subprocess.run([str(exe)], capture_output=True).returncode == 0


# every instance ships: none had to be dropped for scratch or VGPR spills
EXPECTED_KERNELS = ({f"fxk::cellmap_tensor_kernel<{sd},{nn},{o},{g}>" for sd in (2, 3) for nn in (2, 3, 4, 5) for o in (0, 1)
                     for g in ("false", "true")}
                    | {f"fxk::cellmap_apply_kernel<{sd},{o},{m}>" for sd in (2, 3) for o in (0, 1) for m in (0, 1, 2)}
                    | {f"fxk::cellmap_geometry_kernel<{sd}>" for sd in (2, 3)})


@pytest.fixture(scope="module")
def companion_report():
    import codeobject_report
    return codeobject_report.kernels(lib=COMPANION, all_units=True)


@needs_llvm
def test_companion_code_object(companion_report):
    """Exactly the 32 + 12 + 2 instances, gfx950 the only device target, no scratch and no VGPR spills."""
    import instance_manifest
    kernels, targets = companion_report
    assert sorted(targets) == ["hipv4-amdgcn-amd-amdhsa--gfx950", "host-x86_64-unknown-linux-gnu-"]
    names = instance_manifest.normalise_all([k["name"] for k in kernels])
    assert len(names) == len(set(names)) == 46
    assert set(names) == EXPECTED_KERNELS, set(names) ^ EXPECTED_KERNELS
    assert all(k["scratch"] == 0 and k["vgpr_spill"] == 0 for k in kernels), [k for k in kernels if k["scratch"] or k["vgpr_spill"]]


@needs_llvm
def test_recorded_resource_usage_matches_the_build(companion_report):
    """profiles/cellmap_resource_usage.txt lists every instance with the VGPR count of the build, 0 scratch and 0 spills."""
    import instance_manifest
    kernels, _ = companion_report
    built = dict(zip(instance_manifest.normalise_all([k["name"] for k in kernels]), (k["vgpr"] for k in kernels)))
    lines = [ln for ln in open(os.path.join(ROOT, "profiles", "cellmap_resource_usage.txt")) if not ln.startswith("#")]
    listed = {"fxk::" + ln.split(" vgpr")[0].strip().replace(", ", ","): int(ln.split(" vgpr")[1].split()[0]) for ln in lines}
    assert set(listed) == EXPECTED_KERNELS
    assert listed == built
    assert all("scratch 0  spill 0" in ln for ln in lines)


@needs_llvm
def test_main_library_kernel_set_unchanged():
    import codeobject_report
    kernels, _ = codeobject_report.kernels(all_units=True)
    assert not [k["name"] for k in kernels if "cellmap" in k["name"]]
    nm = shutil.which("nm")
    if nm is not None:
        syms = subprocess.run([nm, "-D", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
        assert "fx_cellmap" not in syms


def test_fixture_is_plain_numbers_and_small():
    path = os.path.join(HERE, "golden", "cellmap.npz")
    assert os.path.getsize(path) < 200 * 1000
    for key in G.files:
        assert G[key].dtype in (np.float64, np.int64), key
    assert sorted({k.rsplit("_", 1)[0] for k in G.files}) == sorted(M.CASES)
    for name, (sd, mapping) in M.CASES.items():
        assert G[f"{name}_tab"].shape[0] == 1 + sd and G[f"{name}_x"].shape == (M.NPTS, sd)
        assert (f"{name}_pushed" in G.files) == (mapping != "affine")
