"""Compiled set = manifest set (no GPU): every kernel of the gfx950 code objects in libfiat_amd.so -- all translation units
-- is expected by at least one case of tests/instance_manifest.py, every kernel the manifest names exists in the code
object, and the cases are well-formed.  There is no list of exempt kernels: an instance no request can reach is deleted
from its registry / switch, one that the search did not reach gets a wider search (tools/instance_search.py)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import instance_manifest as M  # noqa: E402

needs_library = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/clang-offload-bundler"),
                                   reason="needs the LLVM tools of ROCm")


@pytest.fixture(scope="module")
def compiled():
    import codeobject_report
    kernels, _ = codeobject_report.kernels(all_units=True)
    return M.normalise_all([k["name"] for k in kernels])


def test_normalise():
    a = "void fxk::tabulate_simplex_pair<3, 3, 1, 20, 6, 8, true, 2, true, false>(fxk::FixedArgs<60>, double*, unsigned int*)"
    assert M.normalise(a) == "fxk::tabulate_simplex_pair<3,3,1,20,6,8,true,2,true,false>"
    assert M.normalise("fxk::map_points_kernel(fxk::MapArgs) [clone .kd]") == "fxk::map_points_kernel"
    assert M.normalise("void fxk::k<(bool)1, (int)3>(int)") == "fxk::k<true,3>"
    assert M.normalise("void (anonymous namespace)::k<fxk::A<2> >(fxk::A<2>)") == "(anonymousnamespace)::k<fxk::A<2>>"


@needs_library
def test_normalised_names_are_distinct_and_in_the_library_namespace(compiled):
    assert len(compiled) > 300
    assert len(set(compiled)) == len(compiled)
    assert all(n.startswith(M.NAMESPACE) for n in compiled)
    # a mangled symbol, with and without the kernel-descriptor suffix, normalises to the same name
    import codeobject_report
    sym = codeobject_report.kernels(all_units=True)[0][0]["name"]
    assert M.normalise(sym) == M.normalise(sym + ".kd") == compiled[0]


@needs_library
def test_every_compiled_kernel_has_a_case(compiled):
    expected = {k for c in M.CASES for k in c["kernels"]}
    missing = sorted(set(compiled) - expected)
    assert not missing, f"{len(missing)} of {len(compiled)} compiled kernels without a checked request shape: {missing[:40]}"


@needs_library
def test_every_manifest_kernel_is_compiled(compiled):
    stale = sorted({k for c in M.CASES for k in c["kernels"]} - set(compiled))
    assert not stale, f"kernels in the manifest that the code object does not hold: {stale[:40]}"


def test_cases_are_well_formed():
    assert M.CASES, "empty manifest"
    ids = [c["id"] for c in M.CASES]
    assert len(set(ids)) == len(ids)
    for c in M.CASES:
        assert c["entry"] in M.ENTRIES, c
        assert c["id"] == M.case_id(c), c
        assert isinstance(c["policy"], list) and all(p in M.POLICIES for p in c["policy"]), c
        assert c["kernels"] and all(k == M.normalise(k) and k.startswith(M.NAMESPACE) for k in c["kernels"]), c
        if c["entry"] in M.PACKING:
            # several requests per wave / workgroup / slab (registry rows with g > 1): a partial last group for every packing
            assert c["nreq"] > M.MAX_GROUP and all(c["nreq"] % g for g in range(2, M.MAX_GROUP + 1)), c
        for key in ("order", "npts", "nreq", "sd", "degree"):
            assert key not in c or (isinstance(c[key], int) and c[key] >= 0), c


def test_policy_names_match_the_library():
    """(host: fiat_amd._lib needs the shared library, not a GPU)"""
    pytest.importorskip("torch")
    lib = os.path.join(ROOT, "fiat_amd", "csrc", "libfiat_amd.so")
    if not os.path.exists(lib):
        pytest.skip("the library is not built")
    from fiat_amd import _lib
    assert set(M.POLICIES) == set(_lib.POLICY)
