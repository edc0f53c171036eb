"""The H(div) trace element and Legendre, host side (no GPU): the NumPy restatement (tests/trace_reference.py) against the
reference's fixtures (tests/golden/trace.npz); the facade's metadata, entity dofs, nodes, errors and registry keys, and the
matrix it prepares for the kernel, with the CPU oracle as arithmetic (tests/host_backend.py); the companion library
libfiat_amd_trace.so -- route reports, argument errors, symbols, header, code object, kernel set and scratch -- with the
kernel set of libfiat_amd.so left as it was.  Tolerance: the project's standing 1e-12 in the norm
max|x - ref| / max(1, max|ref|)."""
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

import make_golden_trace as M  # noqa: E402
import trace_reference as R  # noqa: E402
from host_backend import oracle_backend  # noqa: E402,F401  (fixture)

import fiat_amd.hdiv_trace  # noqa: E402,F401  (the feature: without it this module fails here)
from fiat_amd import _lib  # noqa: E402

G = np.load(os.path.join(HERE, "golden", "trace.npz"))
TOL = 1e-12
COMPANION = os.path.join(ROOT, "fiat_amd", "csrc", "libfiat_amd_trace.so")
SD = {"interval": 1, "triangle": 2, "tetrahedron": 3, "quadrilateral": 2, "product": 2, "prism": 3}
needs_llvm = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/clang-offload-bundler"),
                                reason="needs the LLVM tools of ROCm")
# the cases one facet element serves: (facet dimension, degree)
UNIFORM = {n: (SD[c[0]] - 1, c[1] if not isinstance(c[1], tuple) else c[1][0]) for n, c in M.CASES.items()
           if c[0] not in ("prism",) and not (isinstance(c[1], tuple) and len(set(c[1])) > 1)}


def nfacets(name):
    return len(G[f"{name}_facets"])


def facet_basis(name):
    """The restated facet basis of a uniform case, from the definition (equispaced, integral) or the fixture's nodes."""
    kind, degree, variant = M.CASES[name]
    fd, k = UNIFORM[name]
    if variant is None:
        return R.equispaced_basis(fd, k)
    if variant == "integral":
        return R.integral_basis(fd, k)
    # point variants: the nodes of facet block (sd, ...) in facet coordinates -- on a simplex the barycentric coordinates of
    # the nodes with the facet's own dropped; the last facet drops the last coordinate, so its nodes' cell coordinates ARE
    # the facet coordinates after the first is dropped
    sd = SD[kind]
    n = R.nf(fd, k)
    last = nfacets(name) - 1
    nodes = G[f"{name}_nodes"][last * n:(last + 1) * n]
    lam = R.barycentric(np.vstack([np.zeros(sd), np.eye(sd)]), nodes)
    return R.nodal_basis(fd, k, lam[:, 1:sd])


@pytest.mark.parametrize("name", sorted(UNIFORM))
def test_restatement_against_fixture(name):
    """One-facet tables of every facet, and on simplices the spanning and the failing identify-mode calls."""
    kind = M.CASES[name][0]
    fd, k = UNIFORM[name]
    basis = facet_basis(name)
    nfac = nfacets(name)
    worst = 0.0
    for j in range(nfac):
        pts, ref = G[f"{name}_f{j}_pts"], G[f"{name}_f{j}_tab"]
        got = R.tabulate_facets(nfac, basis, fd, [j], pts[None])[0, 0]
        worst = max(worst, R.rel_err(got, ref))
    if kind in M.SIMPLICES:
        verts = np.vstack([np.zeros(SD[kind]), np.eye(SD[kind])])
        got = R.tabulate_identify(verts, basis, G[f"{name}_span_pts"][None])[0, 0]
        worst = max(worst, R.rel_err(got, G[f"{name}_span_tab"]))
        n = 0
        while f"{name}_fail{n}_pts" in G.files:
            got = R.tabulate_identify(verts, basis, G[f"{name}_fail{n}_pts"][None])[0, 0]
            assert np.isnan(got).all() and np.isnan(G[f"{name}_fail{n}_tab"]).all() and got.shape == G[f"{name}_fail{n}_tab"].shape
            n += 1
        assert n == (1 if kind == "interval" else SD[kind])
    print(f"{name}: {worst:.2e}")
    assert worst <= TOL, (name, worst)


@pytest.mark.parametrize("fd,k", [(1, 0), (1, 3), (1, 6), (1, 12), (2, 0), (2, 2), (2, 6), (2, 12)])
def test_kernel_expansion_is_the_unnormalised_orthogonal_basis(fd, k):
    """The recurrence of csrc/trace.hpp, restated, times its normalisation equals the orthogonal basis in closed form."""
    from fiat_amd.hdiv_trace import _kernel_weights
    rng = np.random.default_rng(k)
    x = rng.uniform(size=(9, fd)) * (0.5 if fd == 2 else 1.0)
    assert R.rel_err(R.kernel_expansion(fd, k, x) * _kernel_weights(fd, k)[:, None], R.integral_basis(fd, k)(x)) <= TOL


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_facade_metadata_and_kernel_matrix(oracle_backend, name):  # noqa: F811
    import fiat_amd
    from fiat_amd.functional import PointEvaluation
    kind, degree, variant = M.CASES[name]
    el = M.build(fiat_amd, name)
    sd = el.get_reference_element().get_spatial_dimension()
    assert [el.degree(), el.space_dimension(), el.get_formdegree(), sd] == list(G[f"{name}_meta"])
    assert np.array_equal(M.eids_rows(el.entity_dofs()), G[f"{name}_eids"])
    assert [(M.dim_code(d), e) for d, e in M.facets_of(el)] == [tuple(r) for r in G[f"{name}_facets"]]
    assert [(M.dim_code(d), e) for d, e in el._facets] == [tuple(r) for r in G[f"{name}_facets"]]
    assert set(el.mapping()) == {"affine"} and el.value_shape() == () and el.is_nodal()
    nodes = M.node_points(el)
    if f"{name}_nodes" in G.files:
        assert all(isinstance(n, PointEvaluation) for n in el.dual_basis())
        assert np.abs(nodes - G[f"{name}_nodes"]).max() <= TOL
    else:
        assert nodes is None and variant == "integral"
    for method, args in (("get_coeffs", ()), ("get_nodal_basis", ()), ("dmats", ()), ("get_num_members", (1,))):
        with pytest.raises(NotImplementedError):
            getattr(el, method)(*args)
    # the matrix the kernel contracts with, against the fixture's one-facet tables through the restated recurrence
    if name in UNIFORM:
        fd, k = UNIFORM[name]
        assert el._kernel is not None and (el._kernel["fd"], el._kernel["degree"], el._kernel["nfac"]) == (fd, k, nfacets(name))
        C = el._kernel["C"]
        n = R.nf(fd, k)
        worst = 0.0
        for j in range(nfacets(name)):
            pts, ref = G[f"{name}_f{j}_pts"], G[f"{name}_f{j}_tab"]
            worst = max(worst, R.rel_err(C @ R.kernel_expansion(fd, k, pts), ref[j * n:(j + 1) * n]))
            assert not np.delete(ref, np.s_[j * n:(j + 1) * n], axis=0).any()
        print(f"{name}: matrix x expansion against the fixture {worst:.2e}")
        assert worst <= TOL, (name, worst)
        assert el.kernel(5).startswith(f"fxk::trace_kernel<{fd},{k if k <= 6 else -1}> ")
    else:
        assert el._kernel is None and el.kernel(5).startswith("general route")
    assert el.kernel(5, route="general").startswith("general route")


def test_constructor_errors_and_registry(oracle_backend):  # noqa: F811
    import fiat_amd
    from fiat_amd import reference_element as RE
    from fiat_amd.hdiv_trace import HDivTrace, TraceError
    assert list(G["hex_raises"]) == [1]
    with pytest.raises(NotImplementedError):
        HDivTrace(RE.UFCHexahedron(), 1)
    with pytest.raises(ValueError):
        HDivTrace(RE.Point(), 0)
    with pytest.raises(ValueError):
        HDivTrace(RE.UFCTriangle(), (1, 2))
    assert fiat_amd.supported_elements["HDiv Trace"] is HDivTrace is fiat_amd.HDivTrace
    assert fiat_amd.supported_elements["Legendre"] is fiat_amd.hierarchical.Legendre
    el = HDivTrace(RE.UFCTriangle(), 2)
    with pytest.raises(TraceError):
        el.tabulate_batch(1, np.zeros((1, 2, 1)), entity=(1, 0))
    with pytest.raises(ValueError):
        el.kernel(5, route="fast")
    # entities that are no facets: TraceError in every slot, without touching a device
    tab = el.tabulate(1, [(0.5,)], entity=(0, 1))
    assert sorted(tab) == [(0, 0), (0, 1), (1, 0)] and all(isinstance(v, TraceError) for v in tab.values())
    quad = HDivTrace(RE.UFCQuadrilateral(), 1)
    with pytest.raises(NotImplementedError):
        quad.tabulate(0, [(0.5, 0.0)])
    with pytest.raises(NotImplementedError):
        quad.kernel(5, "identify")
    big = HDivTrace(RE.UFCTriangle(), 13)
    assert big._kernel is None and big.kernel(4).startswith("general route")
    with pytest.raises(NotImplementedError):
        big.kernel(4, "identify")


def test_numpy_helpers():
    from fiat_amd.hdiv_trace import barycentric_coordinates, extract_facets, map_from_reference_facet, map_to_reference_facet
    verts = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])
    pts = np.array([[0.25, 0.75], [0.0, 0.5], [0.5, 0.0], [0.3, 0.7 - 1e-11]])
    lam = barycentric_coordinates(pts, verts)
    assert np.allclose(lam, R.barycentric(verts, pts), atol=1e-15)
    f2p, ok = extract_facets(lam)
    assert ok and dict(f2p) == {0: [0, 3], 1: [1], 2: [2]}
    assert extract_facets(barycentric_coordinates([[0.2, 0.2]], verts)) == ({}, False)
    assert extract_facets(barycentric_coordinates([[0.0, 0.0]], verts)) == ({}, False)
    f2p, ok = extract_facets(barycentric_coordinates([[0.0], [1.0]], np.array([[0.0], [1.0]])))
    assert ok and f2p[0] == [0] and f2p[1] == [1]                        # the interval: facet i is vertex i
    x = map_to_reference_facet(pts[:1], verts, 0)
    assert np.allclose(x, [[0.75]])
    assert np.allclose(map_from_reference_facet((0.75,), verts[[1, 2]]), pts[0])


@pytest.mark.parametrize("name", sorted(M.LEGENDRE))
def test_legendre_against_fixture(oracle_backend, name):  # noqa: F811
    import fiat_amd
    el = M.build(fiat_amd, name)
    sd = el.get_reference_element().get_spatial_dimension()
    assert [el.degree(), el.space_dimension(), el.get_formdegree(), sd] == list(G[f"{name}_meta"])
    assert R.rel_err(el.get_coeffs(), G[f"{name}_coeffs"]) <= TOL
    assert R.rel_err(el.tabulate(0, G[f"{name}_pts"])[(0,) * sd], G[f"{name}_tab"]) <= TOL
    assert R.rel_err(R.integral_basis(sd, M.LEGENDRE[name][1])(G[f"{name}_pts"]), G[f"{name}_tab"]) <= TOL


# ---- the companion library --------------------------------------------------------------------------------------------

def plan(fd, k, nfac, npts):
    buf = ctypes.create_string_buffer(160)
    _lib.check(_lib.tracelib.fx_trace_kernel(fd, k, nfac, npts, buf, 160))
    return buf.value.decode()


def test_route_report():
    # tetrahedron, degree 2: 4 * 6 * 6 doubles = 1152 B a request; 288 B of matrix; 10 requests fill 64 lanes
    assert plan(2, 2, 4, 6) == "fxk::trace_kernel<2,2> image P=10"
    assert plan(1, 3, 3, 4) == "fxk::trace_kernel<1,3> image P=16"
    assert plan(1, 0, 3, 1) == "fxk::trace_kernel<1,0> image P=64"
    assert plan(0, 0, 2, 5) == "fxk::trace_kernel<0,0> image P=12"
    assert plan(1, 0, 3, 65) == "fxk::trace_kernel<1,0> image P=1"              # chunks of 64 points, still an image
    assert plan(2, 7, 4, 5) == "fxk::trace_kernel<2,-1> image P=7"              # 5760 B a request, no LDS matrix: 7 fit 40 KB
    assert plan(2, 12, 4, 5) == "fxk::trace_kernel<2,-1> image P=2"             # 14 560 B
    assert plan(1, 12, 4, 130) == "fxk::trace_kernel<1,-1> stream P=1"          # 54 080 B
    # the image/stream boundary: degree 6 on the tetrahedron, 28 x 28 doubles of matrix leave 40 960 - 6272 = 34 688 B,
    # a request is 4 * 28 * 8 = 896 B a point
    assert plan(2, 6, 4, 38) == "fxk::trace_kernel<2,6> image P=1"              # 34 048 B
    assert plan(2, 6, 4, 39) == "fxk::trace_kernel<2,6> stream P=1"             # 34 944 B
    # P at its boundary: 7 points, 9 requests fill the lanes; 4 * 28 * 7 * 8 = 6272 B each, 5 fit
    assert plan(2, 6, 4, 7) == "fxk::trace_kernel<2,6> image P=5"
    assert plan(1, 6, 3, 7) == "fxk::trace_kernel<1,6> image P=9"


def test_host_entries_reject_bad_arguments():
    buf = ctypes.create_string_buffer(128)
    for args in ((3, 1, 4, 4), (-1, 0, 2, 4), (1, -1, 3, 4), (1, 1, 3, -4), (1, 1, 0, 4), (1, 1, 5, 4)):
        with pytest.raises(ValueError):
            _lib.check(_lib.tracelib.fx_trace_kernel(*args, buf, 128))
    with pytest.raises(ValueError):
        _lib.check(_lib.tracelib.fx_trace_kernel(1, 1, 3, 4, None, 0))
    with pytest.raises(NotImplementedError, match="degree 13"):
        _lib.check(_lib.tracelib.fx_trace_kernel(2, 13, 4, 4, buf, 128))
    with pytest.raises(NotImplementedError, match="degree 13"):
        _lib.check(_lib.tracelib.fx_trace_kernel(1, 13, 3, 4, buf, 128))
    with pytest.raises(NotImplementedError, match="on a point"):
        _lib.check(_lib.tracelib.fx_trace_kernel(0, 1, 2, 4, buf, 128))
    assert plan(2, 12, 4, 1474836) .endswith("stream P=1")               # 4 * 91 * 1 474 836 < 2^31
    with pytest.raises(NotImplementedError, match="entries"):            # 4 * 91 * 5 900 000 >= 2^31
        _lib.check(_lib.tracelib.fx_trace_kernel(2, 12, 4, 5900000, buf, 128))
    # the error text lands in the main library's slot: one fx_last_error for all
    assert b"entries" in _lib.lib.fx_last_error()
    # the batch entry checks its arguments before it touches the device
    t = _lib.tracelib.fx_trace_tabulate_batch
    with pytest.raises(ValueError, match="null context"):
        _lib.check(t(None, 1, 1, 3, 1, 0, None, None, None, None, 1, 4, None, None, None))
    fake = ctypes.c_void_p(8)            # (never dereferenced: every call below fails its argument checks)
    with pytest.raises(ValueError, match="mode 3"):
        _lib.check(t(fake, 1, 1, 3, 3, 0, None, None, None, None, 1, 4, None, None, None))
    with pytest.raises(ValueError, match="facet 3 of 3"):
        _lib.check(t(fake, 1, 1, 3, 1, 3, None, None, None, None, 1, 4, None, None, None))
    with pytest.raises(ValueError, match="simplices"):
        _lib.check(t(fake, 1, 1, 4, 0, 0, None, None, None, None, 1, 4, None, None, None))
    with pytest.raises(ValueError, match="barycentric map"):
        _lib.check(t(fake, 1, 1, 3, 0, 0, None, None, None, None, 1, 4, None, None, None))
    with pytest.raises(NotImplementedError, match="degree 13"):
        _lib.check(t(fake, 1, 13, 3, 1, 0, None, None, None, None, 1, 4, None, None, None))
    with pytest.raises(ValueError, match="null device pointer"):
        _lib.check(t(fake, 1, 1, 3, 1, 0, None, None, None, None, 1, 4, None, None, None))


def test_companion_symbols_and_abi():
    want = {"fx_trace_abi_version", "fx_trace_kernel", "fx_trace_tabulate_batch"}
    assert set(_lib.TRACE_EXPORTS) == want
    for name in want:
        assert getattr(_lib.tracelib, name) is not None
        for other in (_lib.lib, _lib.serlib, _lib.sflib, _lib.dpclib):
            assert not hasattr(other, name), f"{name} belongs to the trace companion"
    for others in (_lib.EXPORTS, _lib.SER_EXPORTS, _lib.SF_EXPORTS, _lib.DPC_EXPORTS):
        assert want.isdisjoint(others)
    assert _lib.tracelib.fx_trace_abi_version() == 1
    assert _lib.lib.fx_abi_version() == 2
    header = open(os.path.join(ROOT, "include", "fiat_amd_trace.h")).read()
    assert set(re.findall(r"^int (fx_\w+)\(", header, flags=re.M)) == want
    assert "trace" not in open(os.path.join(ROOT, "include", "fiat_amd.h")).read().lower()
    nm = shutil.which("nm")
    if nm is not None:
        syms = subprocess.run([nm, "-D", "--defined-only", COMPANION], check=True, capture_output=True, text=True).stdout
        exported = {line.split()[-1] for line in syms.splitlines() if " T " in line and line.split()[-1].startswith("fx_")}
        assert exported == want
        for path in (_lib.LIB_PATH, _lib.SER_LIB_PATH, _lib.SF_LIB_PATH, _lib.DPC_LIB_PATH):
            assert "fx_trace" not in subprocess.run([nm, "-D", path], check=True, capture_output=True, text=True).stdout


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
    src.write_text('#include "fiat_amd_trace.h"\n'
                   "int main(void) {\n"
                   "    char buf[96];\n"
                   "    if (fx_trace_abi_version() != 1 || fx_abi_version() != 2) return 1;\n"
                   "    if (fx_trace_kernel(2, 2, 4, 6, buf, 96) != FX_OK) return 2;\n"
                   "    if (FX_TRACE_IDENTIFY != 0 || FX_TRACE_ONE_FACET != 1 || FX_TRACE_FACETS != 2) return 3;\n"
                   "    return fx_trace_kernel(2, 13, 4, 6, buf, 96) == FX_ENOTIMPL ? 0 : 4;\n"
                   "}\n")
    inc = os.path.join(ROOT, "include")
    lib = os.path.join(ROOT, "fiat_amd", "csrc")
    exe = tmp_path / "abi_check"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{inc}", str(src), f"-L{lib}",
                    "-lfiat_amd_trace", "-lfiat_amd", f"-Wl,-rpath,{lib}", "-o", str(exe)], check=True, capture_output=True)
    assert subprocess.run([str(exe)], capture_output=True).returncode == 0


# the compiled instances: degree 0-6 per facet dimension 1 and 2, the constant on a point, and one
# run-time-degree instance (degree -1 in the name) per facet dimension
EXPECTED_KERNELS = ({f"fxk::trace_kernel<{fd},{k}>" for fd in (1, 2) for k in range(7)}
                    | {"fxk::trace_kernel<0,0>", "fxk::trace_kernel<1,-1>", "fxk::trace_kernel<2,-1>"})


@pytest.fixture(scope="module")
def companion_report():
    import codeobject_report
    return codeobject_report.kernels(lib=COMPANION, all_units=True)


@needs_llvm
def test_companion_code_object(companion_report):
    """Exactly the 17 instances, gfx950 only, within the project's 128 B scratch budget and without VGPR spills."""
    import instance_manifest
    kernels, targets = companion_report
    assert sorted(targets) == ["hipv4-amdgcn-amd-amdhsa--gfx950", "host-x86_64-unknown-linux-gnu-"]
    names = instance_manifest.normalise_all([k["name"] for k in kernels])
    assert len(names) == len(set(names)) == 17
    assert set(names) == EXPECTED_KERNELS, set(names) ^ EXPECTED_KERNELS
    for k in kernels:
        assert k["scratch"] <= 128 and k["vgpr_spill"] == 0, k


@needs_llvm
def test_recorded_resource_usage_matches_the_build(companion_report):
    """profiles/trace_resource_usage.txt lists every instance, with the scratch and the VGPR spills of this build."""
    import instance_manifest
    kernels, _ = companion_report
    lines = [ln for ln in open(os.path.join(ROOT, "profiles", "trace_resource_usage.txt")) if not ln.startswith("#")]
    listed = {"fxk::" + ln.split(" vgpr")[0].strip().replace(", ", ","): ln for ln in lines}
    assert set(listed) == EXPECTED_KERNELS
    for k, name in zip(kernels, instance_manifest.normalise_all([k["name"] for k in kernels])):
        assert f"scratch {k['scratch']}  spill {k['vgpr_spill']}" in listed[name], (name, k)


@needs_llvm
def test_main_library_kernel_set_unchanged():
    import codeobject_report
    kernels, _ = codeobject_report.kernels(all_units=True)
    assert not [k["name"] for k in kernels if "trace" in k["name"].lower()]
    nm = shutil.which("nm")
    if nm is not None:
        syms = subprocess.run([nm, "-D", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
        assert "trace" not in syms.lower()


def test_fixture_is_plain_numbers_and_small():
    path = os.path.join(HERE, "golden", "trace.npz")
    assert os.path.getsize(path) < 512 * 1024
    for key in G.files:
        assert G[key].dtype in (np.float64, np.int64), key
