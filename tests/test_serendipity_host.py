"""Serendipity elements, host side (no GPU): the NumPy restatement of the product formula against the reference's fixtures
(tests/golden/serendipity.npz), the C dof table against the Python one, and the companion library
libfiat_amd_serendipity.so -- its symbols, header, code object, kernel set and scratch -- with the kernel set of
libfiat_amd.so left as it was."""
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

import make_golden_serendipity as M  # noqa: E402
import serendipity_reference as R  # noqa: E402

from fiat_amd import _lib  # noqa: E402

G = np.load(os.path.join(HERE, "golden", "serendipity.npz"))
VALUE_TOL, DERIV_TOL = 1e-12, 1e-10     # the project's standing tolerances (tests/test_gpu_hdivcurl.py)
BOXES = {"quad": (2, [0.0, 0.0], [1.0, 1.0]), "prod": (2, [0.0, 0.0], [1.0, 1.0]), "box": (2, [-1.0, 0.0], [1.0, 1.0]),
         "hex": (3, [0.0, 0.0, 0.0], [1.0, 1.0, 1.0])}
COMPANION = os.path.join(ROOT, "fiat_amd", "csrc", "libfiat_amd_serendipity.so")
needs_llvm = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/clang-offload-bundler"),
                                reason="needs the LLVM tools of ROCm")


def check_tables(got, ref, what):
    e0 = R.rel_err(got[:1], ref[:1])
    e1 = R.rel_err(got[1:], ref[1:]) if ref.shape[0] > 1 else 0.0
    print(f"{what}: values {e0:.2e} derivatives {e1:.2e}")
    assert e0 <= VALUE_TOL and e1 <= DERIV_TOL, (what, e0, e1)


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_restatement_against_fixture(name):
    kind, k, order, _ = M.CASES[name]
    sd, lo, hi = BOXES[kind]
    ref = G[f"{name}_tab"]
    assert ref.shape[:2] == (len(R.mis(sd, order)), R.ndof(sd, k))
    check_tables(R.tabulate(sd, k, order, G[f"{name}_pts"], lo, hi), ref, name)
    assert list(G[f"{name}_meta"]) == [k + 1, R.ndof(sd, k), 0, k]


def test_restatement_batches():
    rng = np.random.default_rng(3)
    pts = rng.uniform(size=(4, 5, 3))
    got = R.tabulate(3, 4, 2, pts)
    assert got.shape == (4, 10, 50, 5)
    for r in range(4):
        assert np.array_equal(got[r], R.tabulate(3, 4, 2, pts[r]))


@pytest.mark.parametrize("sd", [2, 3])
@pytest.mark.parametrize("k", range(1, 11))
def test_c_descriptor_equals_python(sd, k):
    n = ctypes.c_int(0)
    _lib.check(_lib.serlib.fx_serendipity_dims(sd, k, ctypes.byref(n)))
    assert n.value == R.ndof(sd, k)
    rows = np.full((n.value, 1 + sd), 99, dtype=np.int32)
    _lib.check(_lib.serlib.fx_serendipity_descriptor(sd, k, _lib.host_ptr(rows)))
    ref = R.descriptor(sd, k)
    assert ref.shape == rows.shape and np.array_equal(rows, ref)
    assert rows[:, 1:].max() <= k and set(np.unique(rows[:, 0])) <= {-1, 1}


def test_dof_counts_of_the_issue():
    assert [R.ndof(2, k) for k in range(1, 7)] == [4, 8, 12, 17, 23, 30]
    assert [R.ndof(3, k) for k in range(1, 7)] == [8, 20, 32, 50, 74, 105]


def test_host_entries_reject_bad_arguments():
    n = ctypes.c_int(0)
    with pytest.raises(ValueError):
        _lib.check(_lib.serlib.fx_serendipity_dims(4, 2, ctypes.byref(n)))
    with pytest.raises(ValueError):
        _lib.check(_lib.serlib.fx_serendipity_dims(2, 0, ctypes.byref(n)))
    buf = ctypes.create_string_buffer(128)
    with pytest.raises(NotImplementedError, match="degree 13"):
        _lib.check(_lib.serlib.fx_serendipity_kernel(2, 13, 0, 4, buf, 128))
    with pytest.raises(NotImplementedError, match="order 4"):
        _lib.check(_lib.serlib.fx_serendipity_kernel(3, 2, 4, 4, buf, 128))
    with pytest.raises(NotImplementedError, match="entries"):      # 10 * 105 * npts >= 2^31
        _lib.check(_lib.serlib.fx_serendipity_kernel(3, 6, 2, 2100000, buf, 128))
    # the error text lands in the main library's slot: one fx_last_error for both
    assert b"entries" in _lib.lib.fx_last_error()


def plan(sd, k, order, npts):
    buf = ctypes.create_string_buffer(160)
    _lib.check(_lib.serlib.fx_serendipity_kernel(sd, k, order, npts, buf, 160))
    return buf.value.decode()


def test_route_report():
    assert plan(2, 2, 1, 9) == "fxk::serendipity_kernel<2,2,1> image P=7"
    assert plan(3, 3, 1, 27) == "fxk::serendipity_kernel<3,3,1> image P=1"      # 2 requests are 55 KB: the item shrinks
    assert plan(3, 2, 2, 8) == "fxk::serendipity_kernel<3,2,2> image P=3"
    assert plan(3, 6, 2, 64) == "fxk::serendipity_kernel<3,6,2> stream P=1"
    assert plan(3, 6, 2, 4) == "fxk::serendipity_kernel<3,6,2> image P=1"       # 33 600 B
    assert plan(3, 6, 2, 5) == "fxk::serendipity_kernel<3,6,2> stream P=12"     # 42 000 B
    assert plan(3, 7, 1, 10) == "fxk::serendipity_generic<3> stream P=6"
    assert plan(2, 3, 3, 130) == "fxk::serendipity_generic<2> stream P=1"
    assert plan(2, 12, 3, 1) == "fxk::serendipity_generic<2> stream P=64"


def test_companion_symbols_and_abi():
    for name in ("fx_serendipity_abi_version", "fx_serendipity_dims", "fx_serendipity_descriptor", "fx_serendipity_kernel",
                 "fx_serendipity_tabulate_batch"):
        assert name in _lib.SER_EXPORTS
        assert getattr(_lib.serlib, name) is not None
        assert not hasattr(_lib.lib, name), f"{name} belongs to the companion, not to libfiat_amd.so"
    assert set(_lib.SER_EXPORTS).isdisjoint(_lib.EXPORTS)
    assert _lib.serlib.fx_serendipity_abi_version() == 1
    assert _lib.lib.fx_abi_version() == 2
    header = open(os.path.join(ROOT, "include", "fiat_amd_serendipity.h")).read()
    for name in _lib.SER_EXPORTS:
        assert f"int {name}(" in header
    assert "serendipity" not in open(os.path.join(ROOT, "include", "fiat_amd.h")).read().lower()


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
    src.write_text('#include "fiat_amd_serendipity.h"\n'
                   "int main(void) {\n"
                   "    int ndof = 0, rows[20 * 4];\n"
                   "    if (fx_serendipity_abi_version() != 1 || fx_abi_version() != 2) return 1;\n"
                   "    if (fx_serendipity_dims(3, 2, &ndof) != FX_OK || ndof != 20) return 2;\n"
                   "    if (fx_serendipity_descriptor(3, 2, rows) != FX_OK || rows[0] != 1 || rows[8 * 4] != -1) return 3;\n"
                   "    return fx_serendipity_dims(5, 2, &ndof) == FX_EINVAL ? 0 : 4;\n"
                   "}\n")
    inc = os.path.join(ROOT, "include")
    lib = os.path.join(ROOT, "fiat_amd", "csrc")
    exe = tmp_path / "abi_check"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{inc}", str(src), f"-L{lib}",
                    "-lfiat_amd_serendipity", "-lfiat_amd", f"-Wl,-rpath,{lib}", "-o", str(exe)], check=True, capture_output=True)
    assert subprocess.run([str(exe)], capture_output=True).returncode == 0


EXPECTED_KERNELS = {f"fxk::serendipity_kernel<{sd},{k},{o}>" for sd in (2, 3) for k in range(1, 7) for o in range(3)} | \
    {"fxk::serendipity_generic<2>", "fxk::serendipity_generic<3>"}


@pytest.fixture(scope="module")
def companion_report():
    import codeobject_report
    return codeobject_report.kernels(lib=COMPANION, all_units=True)


@needs_llvm
def test_companion_code_object(companion_report):
    import instance_manifest
    kernels, targets = companion_report
    assert sorted(targets) == ["hipv4-amdgcn-amd-amdhsa--gfx950", "host-x86_64-unknown-linux-gnu-"]
    names = instance_manifest.normalise_all([k["name"] for k in kernels])
    assert len(names) == len(set(names))
    assert set(names) == EXPECTED_KERNELS, set(names) ^ EXPECTED_KERNELS
    for k in kernels:
        assert k["scratch"] <= 128 and k["vgpr_spill"] == 0, k
    # the compile-time instances keep everything in registers
    assert all(k["scratch"] == 0 for k in kernels), [k for k in kernels if k["scratch"]]


@needs_llvm
def test_main_library_kernel_set_unchanged():
    import codeobject_report
    kernels, _ = codeobject_report.kernels(all_units=True)
    assert not [k["name"] for k in kernels if "serendipity" in k["name"].lower()]
    nm = shutil.which("nm")
    if nm is not None:
        syms = subprocess.run([nm, "-D", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
        assert "serendipity" not in syms.lower()


def test_fixture_is_plain_numbers_and_small():
    path = os.path.join(HERE, "golden", "serendipity.npz")
    assert os.path.getsize(path) < 567 * 1024
    for key in G.files:
        assert G[key].dtype in (np.float64, np.int64), key
