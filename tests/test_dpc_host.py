"""DPC elements, host side (no GPU): the NumPy restatement of the closed form against the reference's fixtures
(tests/golden/dpc.npz), the C dof table against the fixtures' nodes, and the companion library libfiat_amd_dpc.so -- its
symbols, header, code object, kernel set and scratch -- with the kernel set of libfiat_amd.so left as it was."""
import ctypes
import os
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

import dpc_reference as R  # noqa: E402
import make_golden_dpc as M  # noqa: E402

from fiat_amd import _lib  # noqa: E402

G = np.load(os.path.join(HERE, "golden", "dpc.npz"))
SD = {"quad": 2, "hex": 3, "prod": 2}
TABLES = sorted(n for n, c in M.CASES.items() if c[2] is not None)
COMPANION = os.path.join(ROOT, "fiat_amd", "csrc", "libfiat_amd_dpc.so")
needs_llvm = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/clang-offload-bundler"),
                                reason="needs the LLVM tools of ROCm")


def errors(got, ref):
    e0 = R.rel_err(got[:1], ref[:1])
    e1 = R.rel_err(got[1:], ref[1:]) if ref.shape[0] > 1 else 0.0
    return e0, e1


@pytest.mark.parametrize("name", TABLES)
def test_restatement_against_fixture(name):
    """The float64 closed form against the reference's tables.  Degrees <= 5 at the standing 1e-12 / 1e-10, degree 6 at 1e-10 /
    1e-10, degree 7 (q7, a general-route fixture) at ten times the distance measured in
    test_reference_drift_from_extended_precision: 3.7e-12 / 6.0e-12."""
    kind, k, order = M.CASES[name]
    sd = SD[kind]
    ref = G[f"{name}_tab"]
    assert ref.shape[:2] == (len(R.mis(sd, order)), R.ndof(sd, k))
    e0, e1 = errors(R.tabulate(sd, k, order, G[f"{name}_pts"]), ref)
    print(f"{name}: values {e0:.2e} derivatives {e1:.2e}")
    tol = R.fixture_tol(k)
    assert e0 <= tol[0] and e1 <= tol[1], (name, e0, e1)
    assert list(G[f"{name}_meta"]) == [k, R.ndof(sd, k), sd, k]


def test_reference_drift_from_extended_precision():
    """Distance of the float64 closed form, and of the reference's fixture, from the closed form in extended precision
    (``longdouble``, 80 bits here), in the project's norm; fixture points: the vertices, two midpoints, six seeded points, two
    points at most 0.2 outside.  Measured on the CPU of the build container:

        case   closed form (values, derivatives)   reference (values, derivatives)
        q5     9.0e-17  1.1e-16                    1.8e-14  1.6e-14
        q6     2.1e-16  1.4e-16                    1.5e-13  1.3e-13
        h5     5.3e-16  2.7e-16                    2.3e-13  2.4e-13
        h6     4.3e-16  3.9e-16                    1.6e-12  1.4e-12
        q7     9.3e-17  1.0e-16                    3.7e-13  6.0e-13

    (degrees 1-4: closed form <= 5.8e-16, reference <= 3.6e-14).  So the reference's own degree-6 hexahedron values miss the
    standing 1e-12, and the degree-7 tolerance is ten times the last row.  Asserted: the closed form stays within 4e-15 of
    extended precision at every degree -- at most 8 rounded operations of relative error 1.1e-16 per 1-D function value and
    sd + 1 = 4 factors per product, on entries whose magnitude the norm's denominator bounds -- and the fixture is never
    closer to extended precision than the closed form is by more than that."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("no extended precision on this host")
    for name in TABLES:
        kind, k, order = M.CASES[name]
        sd = SD[kind]
        pts = G[f"{name}_pts"]
        ext = R.tabulate(sd, k, order, pts, longdouble=True)
        own = errors(R.tabulate(sd, k, order, pts).astype(np.longdouble), ext)
        ref = errors(G[f"{name}_tab"].astype(np.longdouble), ext)
        print(f"{name}: closed form {own[0]:.1e} {own[1]:.1e}   reference {ref[0]:.1e} {ref[1]:.1e}")
        assert max(own) <= 4e-15, (name, own)
        tol = R.fixture_tol(k)
        assert ref[0] <= tol[0] and ref[1] <= tol[1], (name, ref)


def test_restatement_batches():
    rng = np.random.default_rng(3)
    pts = rng.uniform(size=(4, 5, 3))
    got = R.tabulate(3, 4, 2, pts)
    assert got.shape == (4, 10, 35, 5)
    for r in range(4):
        assert np.array_equal(got[r], R.tabulate(3, 4, 2, pts[r]))


def c_descriptor(sd, k):
    rows = np.full((R.ndof(sd, k), sd + 1), 99, dtype=np.int32)
    _lib.check(_lib.dpclib.fx_dpc_descriptor(sd, k, _lib.host_ptr(rows)))
    return rows


@pytest.mark.parametrize("name", sorted(n for n, c in M.CASES.items() if c[1] >= 1))
def test_c_descriptor_equals_the_fixture_nodes(name):
    """Row for row, alpha = round(k * barycentric coordinates of the reference's dual nodes on the mapped simplex)."""
    kind, k, _ = M.CASES[name]
    sd = SD[kind]
    lam0, Gm = R.barycentric_map(sd)
    lam = lam0 + G[f"{name}_nodes"] @ Gm.T
    alpha = np.rint(k * lam).astype(np.int64)
    assert np.abs(k * lam - alpha).max() < 1e-12 and (alpha.sum(axis=1) == k).all() and alpha.min() >= 0
    rows = c_descriptor(sd, k)
    assert rows.shape == alpha.shape and np.array_equal(rows, alpha)
    assert np.array_equal(R.descriptor(sd, k), alpha)


@pytest.mark.parametrize("sd", [2, 3])
def test_c_descriptor_equals_python_beyond_the_fixtures(sd):
    for k in range(1, 13):
        assert np.array_equal(c_descriptor(sd, k), R.descriptor(sd, k)), k


def test_rows_and_counts_of_the_issue():
    assert [R.ndof(2, k) for k in range(1, 7)] == [3, 6, 10, 15, 21, 28]
    assert [R.ndof(3, k) for k in range(1, 7)] == [4, 10, 20, 35, 56, 84]
    assert c_descriptor(2, 2).tolist() == [[2, 0, 0], [0, 2, 0], [0, 0, 2], [0, 1, 1], [1, 0, 1], [1, 1, 0]]
    assert c_descriptor(3, 2).tolist() == [[2, 0, 0, 0], [0, 2, 0, 0], [0, 0, 2, 0], [0, 0, 0, 2], [0, 0, 1, 1], [0, 1, 0, 1],
                                           [0, 1, 1, 0], [1, 0, 0, 1], [1, 0, 1, 0], [1, 1, 0, 0]]
    assert R.simplex_vertices(2).tolist() == [[0, 0], [1, 0], [0.5, 1]]
    assert R.simplex_vertices(3).tolist() == [[0, 0, 0], [1, 0, 0], [0.5, 1.5, 0], [0.5, 0.5, 1]]


def test_fixture_metadata():
    for name, (kind, k, _) in M.CASES.items():
        sd = SD[kind]
        ndof = R.ndof(sd, k)
        assert list(G[f"{name}_meta"]) == [k, ndof, sd, k]
        assert G[f"{name}_coeffs"].shape == (ndof, ndof) and G[f"{name}_nodes"].shape == (ndof, sd)
        # every dof on the top entity, in the entity ids and in the closure ids
        top = 11 if kind == "prod" else sd
        want = [[top, 0, i] for i in range(ndof)]
        assert G[f"{name}_eids"].tolist() == want and G[f"{name}_cids"].tolist() == want
    assert np.array_equal(G["p3_nodes"], G["q3_nodes"])
    assert np.array_equal(G["q0_nodes"], [[0.5, 0.5]]) and np.array_equal(G["h0_nodes"], [[0.5, 0.5, 0.5]])
    # the product of a default line and a UFC interval: the reference's constructor raises a KeyError
    assert list(G["b2_keyerror"]) == [1]


def plan(sd, k, order, npts):
    buf = ctypes.create_string_buffer(160)
    _lib.check(_lib.dpclib.fx_dpc_kernel(sd, k, order, npts, buf, 160))
    return buf.value.decode()


def test_host_entries_reject_bad_arguments():
    rows = np.zeros((100, 4), dtype=np.int32)
    with pytest.raises(ValueError):
        _lib.check(_lib.dpclib.fx_dpc_descriptor(4, 2, _lib.host_ptr(rows)))
    with pytest.raises(ValueError):
        _lib.check(_lib.dpclib.fx_dpc_descriptor(2, 0, _lib.host_ptr(rows)))
    with pytest.raises(ValueError):
        _lib.check(_lib.dpclib.fx_dpc_descriptor(2, 2, None))
    buf = ctypes.create_string_buffer(128)
    with pytest.raises(ValueError):
        _lib.check(_lib.dpclib.fx_dpc_kernel(1, 2, 0, 4, buf, 128))
    with pytest.raises(ValueError):
        _lib.check(_lib.dpclib.fx_dpc_kernel(2, 2, -1, 4, buf, 128))
    with pytest.raises(ValueError):
        _lib.check(_lib.dpclib.fx_dpc_kernel(2, 2, 0, 4, None, 0))
    with pytest.raises(NotImplementedError, match="degree 7"):
        _lib.check(_lib.dpclib.fx_dpc_kernel(2, 7, 0, 4, buf, 128))
    with pytest.raises(NotImplementedError, match="degree 0"):
        _lib.check(_lib.dpclib.fx_dpc_kernel(3, 0, 0, 4, buf, 128))
    with pytest.raises(NotImplementedError, match="order 3"):
        _lib.check(_lib.dpclib.fx_dpc_kernel(3, 2, 3, 4, buf, 128))
    with pytest.raises(NotImplementedError, match="entries"):      # 10 * 84 * npts >= 2^31
        _lib.check(_lib.dpclib.fx_dpc_kernel(3, 6, 2, 2600000, buf, 128))
    # the error text lands in the main library's slot: one fx_last_error for both
    assert b"entries" in _lib.lib.fx_last_error()
    # the batch entry checks its arguments before it touches the device
    lam0, Gm = R.barycentric_map(2)
    with pytest.raises(ValueError, match="null context"):
        _lib.check(_lib.dpclib.fx_dpc_tabulate_batch(None, 2, 2, _lib.host_ptr(lam0), _lib.host_ptr(Gm), 0, 1, 4, None, None, None))


def test_route_report():
    assert plan(2, 2, 1, 9) == "fxk::dpc_kernel<2,2,1> image P=7"            # 3 * 6 * 9 doubles: 7 requests are 9 KB
    assert plan(3, 3, 1, 27) == "fxk::dpc_kernel<3,3,1> image P=2"           # 17 280 B each: 2 fit 40 KB
    assert plan(3, 6, 2, 64) == "fxk::dpc_kernel<3,6,2> stream P=1"          # 430 080 B
    assert plan(3, 6, 2, 6) == "fxk::dpc_kernel<3,6,2> image P=1"            # 40 320 B
    assert plan(3, 6, 2, 7) == "fxk::dpc_kernel<3,6,2> stream P=9"           # 47 040 B
    assert plan(2, 1, 0, 1) == "fxk::dpc_kernel<2,1,0> image P=64"
    assert plan(2, 1, 0, 65) == "fxk::dpc_kernel<2,1,0> image P=1"           # chunks of 64 points, still an image
    assert plan(2, 6, 2, 130) == "fxk::dpc_kernel<2,6,2> stream P=1"


def test_companion_symbols_and_abi():
    assert set(_lib.DPC_EXPORTS) == {"fx_dpc_abi_version", "fx_dpc_descriptor", "fx_dpc_kernel", "fx_dpc_tabulate_batch"}
    for name in _lib.DPC_EXPORTS:
        assert getattr(_lib.dpclib, name) is not None
        for other in (_lib.lib, _lib.serlib, _lib.sflib):
            assert not hasattr(other, name), f"{name} belongs to the DPC companion"
    for others in (_lib.EXPORTS, _lib.SER_EXPORTS, _lib.SF_EXPORTS):
        assert set(_lib.DPC_EXPORTS).isdisjoint(others)
    assert _lib.dpclib.fx_dpc_abi_version() == 1
    assert _lib.lib.fx_abi_version() == 2
    header = open(os.path.join(ROOT, "include", "fiat_amd_dpc.h")).read()
    import re
    declared = set(re.findall(r"^int (fx_\w+)\(", header, flags=re.M))
    assert declared == set(_lib.DPC_EXPORTS)
    assert "dpc" not in open(os.path.join(ROOT, "include", "fiat_amd.h")).read().lower()
    nm = shutil.which("nm")
    if nm is not None:
        syms = subprocess.run([nm, "-D", "--defined-only", COMPANION], check=True, capture_output=True, text=True).stdout
        exported = {line.split()[-1] for line in syms.splitlines() if " T " in line and line.split()[-1].startswith("fx_")}
        assert exported == set(_lib.DPC_EXPORTS)


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
    src.write_text('#include "fiat_amd_dpc.h"\n'
                   "int main(void) {\n"
                   "    int rows[10 * 4];\n"
                   "    char buf[96];\n"
                   "    if (fx_dpc_abi_version() != 1 || fx_abi_version() != 2) return 1;\n"
                   "    if (fx_dpc_descriptor(3, 2, rows) != FX_OK || rows[0] != 2 || rows[4 * 4 + 2] != 1) return 2;\n"
                   "    if (fx_dpc_kernel(2, 2, 1, 9, buf, 96) != FX_OK) return 3;\n"
                   "    return fx_dpc_kernel(2, 7, 1, 9, buf, 96) == FX_ENOTIMPL ? 0 : 4;\n"
                   "}\n")
    inc = os.path.join(ROOT, "include")
    lib = os.path.join(ROOT, "fiat_amd", "csrc")
    exe = tmp_path / "abi_check"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{inc}", str(src), f"-L{lib}",
                    "-lfiat_amd_dpc", "-lfiat_amd", f"-Wl,-rpath,{lib}", "-o", str(exe)], check=True, capture_output=True)
    assert subprocess.run([str(exe)], capture_output=True).returncode == 0


EXPECTED_KERNELS = {f"fxk::dpc_kernel<{sd},{k},{o}>" for sd in (2, 3) for k in range(1, 7) for o in range(3)}


@pytest.fixture(scope="module")
def companion_report():
    import codeobject_report
    return codeobject_report.kernels(lib=COMPANION, all_units=True)


@needs_llvm
def test_companion_code_object(companion_report):
    """Exactly the 36 instances, within the scratch budget tests/test_serendipity_host.py applies to its companion -- and,
    as every instance is a compile-time one, no scratch at all."""
    import instance_manifest
    kernels, targets = companion_report
    assert sorted(targets) == ["hipv4-amdgcn-amd-amdhsa--gfx950", "host-x86_64-unknown-linux-gnu-"]
    names = instance_manifest.normalise_all([k["name"] for k in kernels])
    assert len(names) == len(set(names)) == 36
    assert set(names) == EXPECTED_KERNELS, set(names) ^ EXPECTED_KERNELS
    for k in kernels:
        assert k["scratch"] <= 128 and k["vgpr_spill"] == 0, k
    assert all(k["scratch"] == 0 for k in kernels), [k for k in kernels if k["scratch"]]


@needs_llvm
def test_recorded_resource_usage_matches_the_build(companion_report):
    """profiles/dpc_resource_usage.txt lists every instance with 0 scratch and 0 spills."""
    lines = [ln for ln in open(os.path.join(ROOT, "profiles", "dpc_resource_usage.txt")) if not ln.startswith("#")]
    listed = {"fxk::" + ln.split(" vgpr")[0].strip().replace(", ", ",") for ln in lines}
    assert listed == EXPECTED_KERNELS
    assert all("scratch 0  spill 0" in ln for ln in lines)


@needs_llvm
def test_main_library_kernel_set_unchanged():
    import codeobject_report
    kernels, _ = codeobject_report.kernels(all_units=True)
    assert not [k["name"] for k in kernels if "dpc" in k["name"].lower()]
    nm = shutil.which("nm")
    if nm is not None:
        syms = subprocess.run([nm, "-D", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
        assert "fx_dpc" not in syms.lower()


def test_fixture_is_plain_numbers_and_small():
    path = os.path.join(HERE, "golden", "dpc.npz")
    assert os.path.getsize(path) < 512 * 1024
    for key in G.files:
        assert G[key].dtype in (np.float64, np.int64), key
