"""BDMCE / BDMCF and the trimmed serendipity families, host side (no GPU): the NumPy evaluation of the descriptors against
the reference's fixtures (tests/golden/sforms.npz) with metadata and entity dofs, the relations between the descriptors, the
row counts, and the companion library libfiat_amd_sforms.so -- its symbols, header, code object, kernel set, scratch and
route report -- with the other two libraries left as they were."""
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

import make_golden_sforms as M  # noqa: E402
import sforms_reference as R  # noqa: E402

import fiat_amd  # noqa: E402
from fiat_amd import _lib, sforms  # noqa: E402

G = np.load(os.path.join(HERE, "golden", "sforms.npz"))
VALUE_TOL, DERIV_TOL = 1e-12, 1e-10     # the project's standing tolerances (tests/test_gpu_hdivcurl.py)
COMPANION = os.path.join(ROOT, "fiat_amd", "csrc", "libfiat_amd_sforms.so")
FAMILY = {"bdmce": "BDMCE", "bdmcf": "BDMCF", "sme": "SminusE", "smf": "SminusF", "smc": "SminusCurl", "smd": "SminusDiv"}
needs_llvm = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/clang-offload-bundler"),
                                reason="needs the LLVM tools of ROCm")
_WORST = {"values": 0.0, "derivatives": 0.0}


def check_tables(got, ref, what):
    e0 = R.rel_err(got[:1], ref[:1])
    e1 = R.rel_err(got[1:], ref[1:]) if ref.shape[0] > 1 else 0.0
    _WORST["values"], _WORST["derivatives"] = max(_WORST["values"], e0), max(_WORST["derivatives"], e1)
    print(f"{what}: values {e0:.2e} derivatives {e1:.2e}; worst so far {_WORST['values']:.2e} / {_WORST['derivatives']:.2e}")
    assert e0 <= VALUE_TOL and e1 <= DERIV_TOL, (what, e0, e1)


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_restatement_against_fixture(name):
    """Tables, metadata, entity dofs and closure dofs of every fixture."""
    c, kind, k, order = M.CASES[name]
    el = M.build(fiat_amd, name)
    sd = el.get_reference_element().get_spatial_dimension()
    coef, codes = el.descriptor()
    assert np.array_equal(coef, sforms.descriptor(FAMILY[c], sd, k)[0])
    ref = G[f"{name}_tab"]
    assert ref.shape[:3] == (len(R.mis(sd, order)), el.num_rows(), sd)
    check_tables(R.tabulate(coef, codes, k, order, G[f"{name}_pts"], el._lo, el._hi), ref, name)
    assert list(M.metadata(el)) == list(G[f"{name}_meta"])
    assert np.array_equal(M.eids_rows(el.entity_dofs()), G[f"{name}_eids"])
    assert np.array_equal(M.eids_rows(el.entity_closure_dofs()), G[f"{name}_cids"])
    assert el.value_shape() == (sd,) and el.degree() == k and el.get_order() == k
    for method in (el.dual_basis, el.get_coeffs):
        with pytest.raises(NotImplementedError):
            method()


@pytest.mark.parametrize("name,key,edim", M.ENTITIES)
def test_restatement_on_entities(name, key, edim):
    """entity= fixtures: the entity's affine map on the host, then the same evaluation."""
    el = M.build(fiat_amd, name)
    Mx, b = el._entity_affine(key)
    p = G[M.ent_name(name, key) + "_pts"]
    assert p.shape[1] == edim
    coef, codes = el.descriptor()
    check_tables(R.tabulate(coef, codes, el.degree(), 1, p @ Mx.T + b, el._lo, el._hi), G[M.ent_name(name, key) + "_tab"], (name, key))


def test_every_required_case_is_in_the_fixture():
    for c in M.CLASSES:
        for k in range(1, 7):
            assert M.CASES[f"{c}_q{k}"] == (c, "quad", k, 2 if k <= 4 else 1)
    for c, ks in (("smd", range(1, 6)), ("smc", range(1, 6)), ("sme", range(1, 4))):
        for k in ks:
            assert M.CASES[f"{c}_h{k}"][1:3] == ("hex", k) and M.CASES[f"{c}_h{k}"][3] >= (2 if k <= 2 else 1)
    kinds = [v[1] for v in M.CASES.values()]
    assert "prod" in kinds and kinds.count("box") >= 2
    for name in M.CASES:
        for suffix in ("pts", "tab", "meta", "eids", "cids"):
            assert f"{name}_{suffix}" in G.files
    dims = {(M.CASES[n][1], e) for n, _, e in M.ENTITIES}
    assert {("quad", 1), ("hex", 2), ("hex", 1)} <= dims


def test_bdmcf_is_the_rotation_of_bdmce():
    for k in range(1, 7):
        ce, ke = sforms.descriptor("BDMCE", 2, k)
        cf, kf = sforms.descriptor("BDMCF", 2, k)
        assert np.array_equal(cf[:, 0], -ce[:, 1]) and np.array_equal(cf[:, 1], ce[:, 0])
        assert np.array_equal(kf[:, 0], ke[:, 1]) and np.array_equal(kf[:, 1], ke[:, 0])


def test_relations_of_the_trimmed_quadrilateral_classes():
    """SminusE = SminusCurl and SminusF is its rotation at every degree; SminusDiv is SminusF only up to degree 2: from
    degree 3 on the reference lists its lower-order interior functions in another order."""
    for k in range(1, 7):
        ce, ke = sforms.descriptor("SminusE", 2, k)
        cc, kc = sforms.descriptor("SminusCurl", 2, k)
        cf, kf = sforms.descriptor("SminusF", 2, k)
        cd, kd = sforms.descriptor("SminusDiv", 2, k)
        assert np.array_equal(ce, cc) and np.array_equal(ke, kc)
        assert np.array_equal(cf[:, 0], -ce[:, 1]) and np.array_equal(cf[:, 1], ce[:, 0])
        assert np.array_equal(kf[:, 0], ke[:, 1]) and np.array_equal(kf[:, 1], ke[:, 0])
        same = np.array_equal(cd, cf) and np.array_equal(kd, kf)
        assert same == (k <= 2), k
        # as sets of rows the two agree at every degree
        rows = lambda c, kk: sorted(map(tuple, np.concatenate([c, kk.reshape(len(c), -1)], axis=1).tolist()))  # noqa: E731
        assert rows(cd, kd) == rows(cf, kf)


def test_row_counts_of_the_issue():
    n = lambda f, sd, k: sforms.descriptor(f, sd, k)[0].shape[0]  # noqa: E731
    for f in ("BDMCE", "BDMCF"):
        assert [n(f, 2, k) for k in range(1, 7)] == [8, 14, 22, 32, 44, 58]
    for f in ("SminusE", "SminusF", "SminusCurl", "SminusDiv"):
        assert [n(f, 2, k) for k in range(1, 7)] == [4, 10, 17, 26, 37, 50]
    assert [n("SminusDiv", 3, k) for k in range(1, 6)] == [6, 21, 45, 82, 135]
    assert [n("SminusCurl", 3, k) for k in range(1, 6)] == [12, 36, 66, 111, 173]
    assert [n("SminusE", 3, k) for k in range(1, 4)] == [12, 36, 66]


def test_coefficients_and_codes():
    """Coefficients are +-1 and BDMC's binomial ratio (the +-1/(k+1) of the reference's e_lambda_tilde functions enter no
    basis it builds); every code is within the family."""
    import math
    for (f, sd), kmax in sforms.MAX_DEGREE.items():
        for k in range(1, kmax + 1):
            coef, codes = sforms.descriptor(f, sd, k)
            allowed = {0.0, 1.0, -1.0}
            if f.startswith("BDMC"):
                c = math.comb(2 * k, k) / ((k + 1) * math.comb(2 * k - 2, k - 1))
                allowed |= {c, -c}
            assert set(np.unique(coef)) <= allowed, (f, sd, k)
            assert codes.min() >= 0 and codes.max() < sforms.ncodes(k)
            assert not codes[coef == 0.0].any()
            assert (coef != 0.0).any(axis=1).all()          # no basis function is identically zero


def test_builder_fails_outside_the_family():
    B = sforms._Blocks(2)
    with pytest.raises(ValueError, match="outside the 1-D family"):
        (B.P(0, 1) * B.P(0, 2)).classify(3)                 # two Legendre polynomials in one variable
    with pytest.raises(ValueError, match="outside the 1-D family"):
        (B.lam(0, 0) * B.P(0, 1)).classify(3)               # lambda0 L_1
    with pytest.raises(ValueError, match="outside the 1-D family"):
        (B.bub(1) * B.lam(1, 1)).classify(3)
    with pytest.raises(ValueError, match="beyond degree"):
        B.P(1, 4).classify(3)
    assert (B.lam(0, 1) * B.P(0, 0) * B.bub(1) * B.P(1, 2) / 4).classify(3) == (0.25, [1, 3 + 3 + 2])
    # the lower-order face functions of SminusE on the hexahedron leave the family at degree 4
    bad = 0
    for row in sforms.trimmed_hex_edge_rows(4):
        for term in row:
            try:
                term is None or term.classify(4)
            except ValueError:
                bad += 1
    assert bad > 0


def test_constructor_errors_without_a_gpu():
    from fiat_amd import reference_element as RE
    quad, hexa = RE.UFCQuadrilateral(), RE.UFCHexahedron()
    for cls in (fiat_amd.BrezziDouglasMariniCubeEdge, fiat_amd.BrezziDouglasMariniCubeFace, fiat_amd.TrimmedSerendipityEdge,
                fiat_amd.TrimmedSerendipityFace, fiat_amd.TrimmedSerendipityCurl, fiat_amd.TrimmedSerendipityDiv):
        with pytest.raises(Exception, match="only valid for k >= 1"):
            cls(quad, 0)
        with pytest.raises(Exception, match="only valid for dimension"):
            cls(fiat_amd.UFCInterval(), 1)
        with pytest.raises(NotImplementedError, match="degree 7"):
            cls(quad, 7)
    for cls in (fiat_amd.BrezziDouglasMariniCubeEdge, fiat_amd.BrezziDouglasMariniCubeFace, fiat_amd.TrimmedSerendipityFace):
        with pytest.raises(Exception, match="only valid for dimension 2"):
            cls(hexa, 1)
    with pytest.raises(NotImplementedError, match="disagree"):
        fiat_amd.TrimmedSerendipityEdge(hexa, 4)
    with pytest.raises(NotImplementedError, match="two Legendre polynomials"):
        fiat_amd.TrimmedSerendipityCurl(hexa, 6)
    with pytest.raises(NotImplementedError, match="degree 6"):
        fiat_amd.TrimmedSerendipityDiv(hexa, 6)
    assert fiat_amd.supported_elements["Brezzi-Douglas-Marini Cube Edge"] is fiat_amd.BrezziDouglasMariniCubeEdge
    assert fiat_amd.supported_elements["Brezzi-Douglas-Marini Cube Face"] is fiat_amd.BrezziDouglasMariniCubeFace
    assert fiat_amd.supported_elements["SminusE"] is fiat_amd.TrimmedSerendipityEdge
    assert fiat_amd.supported_elements["SminusF"] is fiat_amd.TrimmedSerendipityFace
    assert fiat_amd.supported_elements["SminusCurl"] is fiat_amd.TrimmedSerendipityCurl
    assert fiat_amd.supported_elements["SminusDiv"] is fiat_amd.TrimmedSerendipityDiv


def test_degree_one_trimmed_quadrilateral_mirrors_the_reference():
    """The reference counts 5 dofs but numbers and tabulates 4 functions."""
    from fiat_amd import reference_element as RE
    el = fiat_amd.TrimmedSerendipityDiv(RE.UFCQuadrilateral(), 1)
    assert el.space_dimension() == 5 and len(el.mapping()) == 5 and el.num_rows() == 4
    assert sorted(i for es in el.entity_dofs().values() for ids in es.values() for i in ids) == [0, 1, 2, 3]


# ---- the companion library -------------------------------------------------------------------------------------------

def test_companion_symbols_and_abi():
    names = ("fx_sforms_abi_version", "fx_sforms_element_create", "fx_sforms_element_destroy", "fx_sforms_kernel",
             "fx_sforms_tabulate_batch")
    assert set(names) == set(_lib.SF_EXPORTS)
    for name in names:
        assert getattr(_lib.sflib, name) is not None
        assert not hasattr(_lib.lib, name), f"{name} belongs to the companion, not to libfiat_amd.so"
        assert not hasattr(_lib.serlib, name), f"{name} belongs to the sforms companion, not to the serendipity one"
    assert set(_lib.SF_EXPORTS).isdisjoint(_lib.EXPORTS) and set(_lib.SF_EXPORTS).isdisjoint(_lib.SER_EXPORTS)
    assert _lib.sflib.fx_sforms_abi_version() == 1
    header = open(os.path.join(ROOT, "include", "fiat_amd_sforms.h")).read()
    for name in _lib.SF_EXPORTS:
        assert f"int {name}(" in header
    nm = shutil.which("nm")
    if nm is not None:
        for path, want in ((COMPANION, True), (_lib.LIB_PATH, False), (_lib.SER_LIB_PATH, False)):
            syms = subprocess.run([nm, "-D", path], check=True, capture_output=True, text=True).stdout
            assert ("sforms" in syms.lower()) == want, path
    for other in ("fiat_amd.h", "fiat_amd_serendipity.h"):
        assert "sforms" not in open(os.path.join(ROOT, "include", other)).read().lower()


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
    src.write_text('#include "fiat_amd_sforms.h"\n'
                   "int main(void) {\n"
                   "    char buf[128];\n"
                   "    fx_sforms_element* el = 0;\n"
                   "    if (fx_sforms_abi_version() != 1 || fx_abi_version() != 2) return 1;\n"
                   "    if (fx_sforms_kernel(2, 1, 8, 0, 4, buf, 128) != FX_OK) return 2;\n"
                   "    if (fx_sforms_kernel(4, 1, 8, 0, 4, buf, 128) != FX_EINVAL) return 3;\n"
                   "    if (fx_sforms_kernel(2, 1, 8, 3, 4, buf, 128) != FX_ENOTIMPL) return 4;\n"
                   "    return fx_sforms_element_destroy(el) == FX_OK ? 0 : 5;\n"
                   "}\n")
    inc = os.path.join(ROOT, "include")
    lib = os.path.join(ROOT, "fiat_amd", "csrc")
    exe = tmp_path / "abi_check"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{inc}", str(src), f"-L{lib}",
                    "-lfiat_amd_sforms", "-lfiat_amd", f"-Wl,-rpath,{lib}", "-o", str(exe)], check=True, capture_output=True)
    assert subprocess.run([str(exe)], capture_output=True).returncode == 0


EXPECTED_KERNELS = {f"fxk::sforms_kernel<{sd},{o}>" for sd in (2, 3) for o in range(3)}


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
    assert all(k["scratch"] == 0 and k["vgpr_spill"] == 0 for k in kernels), [k for k in kernels if k["scratch"] or k["vgpr_spill"]]


@needs_llvm
def test_other_libraries_hold_no_sforms_kernel():
    import codeobject_report
    for lib in (None, _lib.SER_LIB_PATH):
        kernels, _ = codeobject_report.kernels(all_units=True) if lib is None else codeobject_report.kernels(lib=lib, all_units=True)
        assert not [k["name"] for k in kernels if "sforms" in k["name"].lower()]


def test_fixture_is_plain_numbers_and_small():
    path = os.path.join(HERE, "golden", "sforms.npz")
    assert os.path.getsize(path) < 512 * 1024
    for key in G.files:
        assert G[key].dtype in (np.float64, np.int64), key


# ---- the route report ------------------------------------------------------------------------------------------------

def plan(sd, k, nrows, order, npts):
    buf = ctypes.create_string_buffer(160)
    _lib.ser_check(_lib.sflib.fx_sforms_kernel(sd, k, nrows, order, npts, buf, 160))
    return buf.value.decode()


def budget(sd, k, order):
    """The image budget as sforms.hpp sizes it: what a 40 KB workgroup leaves beside the 1-D tables
    (sd (order + 1) (2 k + 4) 64 doubles), at least 16 KB."""
    return max(16 * 1024, 40 * 1024 - sd * (order + 1) * (2 * k + 4) * 64 * 8)


def test_route_report():
    # BDMCF_1, order 1, 9 points: 3 * 8 * 2 * 9 doubles = 3456 B a request; tables 12 KB, budget 28 KB: all 7 fit
    assert plan(2, 1, 8, 1, 9) == f"fxk::sforms_kernel<2,1> image P=7 budget={28 * 1024}"
    # SminusDiv_2 quadrilateral, order 1, 9 points: 4320 B; tables 16 KB, budget 24 KB: the item shrinks to 5
    assert plan(2, 2, 10, 1, 9) == f"fxk::sforms_kernel<2,1> image P=5 budget={24 * 1024}"
    # SminusCurl_2 hexahedron, order 1, 27 points: 4 * 36 * 3 * 27 * 8 = 93 312 B: streams
    assert plan(3, 2, 36, 1, 27) == f"fxk::sforms_kernel<3,1> stream P=2 budget={16 * 1024}"
    assert plan(3, 3, 45, 2, 27) == f"fxk::sforms_kernel<3,2> stream P=2 budget={16 * 1024}"
    assert plan(3, 1, 6, 0, 3) == f"fxk::sforms_kernel<3,0> image P=21 budget={budget(3, 1, 0)}"
    assert plan(2, 6, 58, 2, 130) == f"fxk::sforms_kernel<2,2> stream P=1 budget={16 * 1024}"
    assert plan(2, 6, 58, 2, 2) == f"fxk::sforms_kernel<2,2> image P=1 budget={16 * 1024}"       # 11 136 B
    for sd, k, order in [(2, 1, 0), (2, 3, 1), (2, 6, 2), (3, 1, 1), (3, 2, 2), (3, 5, 2)]:
        assert plan(sd, k, 12, order, 1).endswith(f"budget={budget(sd, k, order)}")
        assert sd * (order + 1) * (2 * k + 4) * 64 * 8 <= 64 * 1024          # the 1-D tables alone


def test_host_entries_reject_bad_arguments():
    buf = ctypes.create_string_buffer(128)
    with pytest.raises(ValueError, match="dimension 4"):
        _lib.ser_check(_lib.sflib.fx_sforms_kernel(4, 2, 10, 0, 4, buf, 128))
    with pytest.raises(ValueError, match="degree 0"):
        _lib.ser_check(_lib.sflib.fx_sforms_kernel(2, 0, 10, 0, 4, buf, 128))
    with pytest.raises(NotImplementedError, match="degree 7"):
        _lib.ser_check(_lib.sflib.fx_sforms_kernel(2, 7, 10, 0, 4, buf, 128))
    with pytest.raises(NotImplementedError, match="order 3"):
        _lib.ser_check(_lib.sflib.fx_sforms_kernel(3, 2, 36, 3, 4, buf, 128))
    with pytest.raises(NotImplementedError, match="entries"):      # 10 * 135 * 3 * npts >= 2^31
        _lib.ser_check(_lib.sflib.fx_sforms_kernel(3, 5, 135, 2, 540000, buf, 128))
    # the error text lands in the main library's slot: one fx_last_error for all three libraries
    assert b"entries" in _lib.lib.fx_last_error()
