"""``evaluate_batch``, host side (no GPU): the NumPy restatement of the fused kernel's order of operations against the
reference's fixture (tests/golden/evaluate.npz), the folded coefficients, the stand-alone walk program, and the companion library
libfiat_amd_eval.so -- its symbols, header, code object, kernel set and scratch -- with the kernel set of libfiat_amd.so left as
it was."""
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

import evaluate_cells_reference as C  # noqa: E402
import evaluate_reference as R  # noqa: E402
import make_golden_evaluate as M  # noqa: E402

from fiat_amd import _lib  # noqa: E402
from oracle import fiat_oracle as fo  # noqa: E402

G = np.load(os.path.join(HERE, "golden", "evaluate.npz"))
STANDING = (1e-12, 1e-10)
FUSED = [n for n in M.CASES if n not in M.GENERAL_ONLY]
COMPANION = os.path.join(ROOT, "fiat_amd", "csrc", "libfiat_amd_eval.so")
needs_llvm = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/clang-offload-bundler"),
                                reason="needs the LLVM tools of ROCm")


def meta(name):
    n, ndof, sd, vdim, mapping, variant = (int(x) for x in G[f"{name}_meta"])
    return {"n": n, "ndof": ndof, "sd": sd, "vdim": vdim, "mapping": mapping, "variant": variant,
            "scale": float(G[f"{name}_scale"][0]), "value_shape": tuple(G[f"{name}_ref"].shape[2:-1])}


def restated(name, physical, longdouble=False):
    m = meta(name)
    kw = dict(verts=G[f"{name}_verts"], mapping=m["mapping"]) if physical else {}
    return R.evaluate(m["sd"], m["n"], R.VARIANTS[m["variant"]], m["scale"], G[f"{name}_coeffs"], M.ORDER,
                      G[f"{name}_ppts" if physical else f"{name}_pts"], G[f"{name}_dofs"], value_shape=m["value_shape"],
                      longdouble=longdouble, **kw)


@pytest.mark.parametrize("physical", [False, True], ids=["own", "physical"])
@pytest.mark.parametrize("name", FUSED)
def test_restatement_against_fixture(name, physical):
    """Fold, transform, walk and Piola matrix in float64 against the reference's own contraction, on the element's cell and on
    the skewed physical cell, at the standing 1e-12 / 1e-10."""
    ref = G[f"{name}_pref" if physical else f"{name}_ref"]
    m = meta(name)
    assert ref.shape == (len(R.jet(m["sd"], M.ORDER)), M.NRHS) + m["value_shape"] + (len(G[f"{name}_pts"]),)
    e0, e1 = R.errors(restated(name, physical), ref)
    print(f"{name} {'physical' if physical else 'own'}: values {e0:.2e} derivatives {e1:.2e}")
    assert e0 <= STANDING[0] and e1 <= STANDING[1], (name, e0, e1)


def test_restatement_drift_from_extended_precision():
    """The float64 restatement against the same operations in extended precision, at the standing tolerances: the
    transform-then-dot order loses nothing they would see.  Measured here (the printed table is the record, run with -s): at most
    1e-15 on the element's cell and 9.3e-14 on the skewed physical cell, where the inverse of the cell's edge matrix (edges of
    0.05, 30 % skew) carries most of it."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("no extended precision on this host")
    for name in FUSED:
        for physical in (False, True):
            ext = restated(name, physical, longdouble=True)
            e = R.errors(restated(name, physical).astype(np.longdouble), ext)
            print(f"{name} {'physical' if physical else 'own'}: {e[0]:.1e} {e[1]:.1e}")
            assert e[0] <= STANDING[0] and e[1] <= STANDING[1], (name, physical, e)


CELL_CASES = [(c, False) for c in C.ALL_CASES] + [(c, True) for c in C.OWN_CASES]


@pytest.mark.parametrize("case,own", CELL_CASES, ids=["-".join(str(x) for x in c) + ("-own" if own else "") for c, own in CELL_CASES])
def test_restatement_on_cells_against_closed_form(case, own):
    """Every batch that tests/test_gpu_evaluate_cells.py runs, here in float64 through the restatement against the closed-form
    oracle (the reference's tables on its reference cell, chained through B^-1 and pushed by J^-T or J / det J), every request
    compared at the standing 1e-12 / 1e-10: the inputs satisfy the stated conditions (cond_2(B) <= 8, both orientations) and
    the oracle alone stays inside the tolerances.  Measured (the printed lines are the record, run with -s): at most 1.8e-14 /
    1.5e-14 on UFC-built elements; 1.9e-13 / 3.6e-13 for elements built on the fixture's skewed cell, where the oracle is the
    reference's element built on that cell and the figure is the same in extended precision: the reference's own rounding on
    a cell with edges of 0.05, not the conditioning of the requests' cells."""
    b = C.batch(*case, own=own)
    nreq, npts, nrhs = case[3], case[2], case[4]
    assert b["ref"].shape[:3] == (nreq, len(R.jet(C.meta(case[0])["sd"], case[1])), nrhs) and b["ref"].shape[-1] == npts
    if nreq > 1:
        assert not np.array_equal(b["idx"][0], b["idx"][1]) or npts == 1
    e0, e1 = C.worst(C.restated(case[0], case[1], b, own=own), b["ref"])
    print(f"{case}{' own' if own else ''}: values {e0:.2e} derivatives {e1:.2e}")
    assert e0 <= STANDING[0] and e1 <= STANDING[1], (case, e0, e1)


def test_cell_case_lists():
    """The lists reach all 15 instances with per-request cells; the shapes are the ones their names promise."""
    assert C.instances_with_cells() == {(sd, o, v) for sd in (1, 2, 3) for o in range(3) for v in {1, sd}}
    assert len(C.FAMILY_CASES) == len(FUSED) == 19
    assert max(c[3] for c in C.ALL_CASES) <= 200
    assert C.plan("lag_tri2", 0, 7) == (9, 1) and C.plan("lag_tri2", 1, 70) == (1, 2)        # the alignment shapes
    assert C.plan("lag_tet3", 2, 23) == (2, 1) and C.plan("rt_tet2", 2, 70) == (1, 2) and C.plan("ned_tri3", 2, 9) == (7, 1)
    for name in C.SHAPE_ELEMENTS:
        assert 1 < C.plan(name, 2, 1)[0] < 64                                                 # P set by the LDS budget
        assert [C.plan(name, 2, p)[1] for p in C.SHAPE_POINTS] == [1, 1, 1, 2, 3]


def c_fold(name):
    m = meta(name)
    coeffs = np.ascontiguousarray(G[f"{name}_coeffs"], dtype=np.float64)
    out = np.full(coeffs.size, np.nan)
    _lib.ser_check(_lib.evallib.fx_eval_fold(m["sd"], m["n"], m["variant"], m["ndof"], m["vdim"], _lib.host_ptr(coeffs),
                                             _lib.host_ptr(out)))
    return out.reshape(m["ndof"], m["vdim"], -1)


@pytest.mark.parametrize("name", FUSED)
def test_folded_coefficients(name):
    """fx_eval_fold: ``coeffs @ T`` for the bubble variant (T of fx_plan_c0_transform and of the oracle's C0 basis), the
    coefficients themselves otherwise, columns in the order of fx_eval_walk_order, which is the restatement's."""
    m = meta(name)
    sd, n = m["sd"], m["n"]
    nexp = len(R.walk_members(sd, n))
    order = np.full(nexp, -1, dtype=np.int32)
    _lib.ser_check(_lib.evallib.fx_eval_walk_order(sd, n, _lib.host_ptr(order)))
    assert list(order) == R.walk_order(sd, n) and sorted(order) == list(range(nexp))
    C = G[f"{name}_coeffs"].reshape(m["ndof"], m["vdim"], nexp)
    if m["variant"] == 1:
        T = np.zeros((nexp, nexp))
        _lib.check(_lib.lib.fx_plan_c0_transform(sd, n, _lib.host_ptr(T)))
        assert np.array_equal(T, R.c0_matrix(sd, n))
        C = C @ T
    got = c_fold(name)
    scale = max(1.0, np.abs(C).max())
    assert np.abs(got - C[..., order]).max() <= 1e-14 * scale
    assert np.abs(got - R.fold(sd, n, R.VARIANTS[m["variant"]], G[f"{name}_coeffs"])).max() <= 1e-14 * scale


def walk_cases():
    cases = []
    for name in FUSED:
        m = meta(name)
        base = dict(sd=m["sd"], n=m["n"], variant=m["variant"], scale=m["scale"], order=M.ORDER, vdim=m["vdim"],
                    cell=fo.UFC_SIMPLEX[m["sd"]], coeffs=G[f"{name}_coeffs"].reshape(m["ndof"], m["vdim"], -1), dofs=G[f"{name}_dofs"])
        cases.append(dict(base, mapping=0, verts=None, pts=G[f"{name}_pts"], ref=G[f"{name}_ref"]))
        cases.append(dict(base, mapping=m["mapping"], verts=G[f"{name}_verts"], pts=G[f"{name}_ppts"], ref=G[f"{name}_pref"]))
    # random cells of both orientations per (sd, vdim, mapping), and elements built on their own skewed cell
    return cases + C.walk_cell_cases()


def test_walk_program_against_fixture(tmp_path):
    """tools/evaluate_walk_host.cpp: the kernel's __host__ __device__ walk, geometry and Piola matrix compiled for the CPU,
    every instance (sd, order, vdim), on both cells of every fixture case, on three random cells (one negatively oriented)
    per (sd, vdim, mapping) against the closed-form oracle, and per dimension on an element built on its own skewed cell with
    and without a request's cell on top, at the standing tolerances (the program's exit status)."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "walk"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'fiat_amd', 'csrc')}",
                    os.path.join(ROOT, "tools", "evaluate_walk_host.cpp"), "-o", str(exe)], check=True, capture_output=True)
    path = tmp_path / "cases.txt"
    cases = walk_cases()
    assert len(cases) == 2 * 19 + 3 * 7 + 2 * 3
    assert sum(c["verts"] is not None and np.linalg.det(C.edge_matrices(np.asarray(c["verts"])[None])[0]) < 0 for c in cases) >= 7
    assert sum(not np.array_equal(c["cell"], fo.UFC_SIMPLEX[c["sd"]]) for c in cases) == 6
    R.write_walk_cases(path, cases)
    run = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    print(run.stdout[-3000:])
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert f"{len(cases)} cases, 15 instances, 0 missing" in run.stdout
    assert run.stdout.count("eval_walk<") == 3 * len(cases) and "FAIL" not in run.stdout


def plan(sd, n, order, vdim, ndof, npts, nrhs=1):
    buf = ctypes.create_string_buffer(160)
    _lib.ser_check(_lib.evallib.fx_eval_kernel(sd, n, order, vdim, ndof, npts, nrhs, buf, 160))
    return buf.value.decode()


def test_route_report():
    assert plan(3, 3, 1, 1, 20, 23) == "fxk::eval_kernel<3,1,1> degree=3 P=2 chunks=1"
    assert plan(2, 2, 0, 1, 6, 6) == "fxk::eval_kernel<2,0,1> degree=2 P=10 chunks=1"
    assert plan(3, 2, 0, 3, 20, 23) == "fxk::eval_kernel<3,0,3> degree=2 P=2 chunks=1"
    assert plan(1, 1, 0, 1, 2, 1) == "fxk::eval_kernel<1,0,1> degree=1 P=64 chunks=1"
    assert plan(3, 6, 2, 1, 84, 1) == "fxk::eval_kernel<3,2,1> degree=6 P=11 chunks=1"      # 84 dofs + 84 w + 10 doubles each
    assert plan(2, 2, 1, 1, 6, 64) == "fxk::eval_kernel<2,1,1> degree=2 P=1 chunks=1"
    assert plan(2, 2, 1, 1, 6, 65) == "fxk::eval_kernel<2,1,1> degree=2 P=1 chunks=2"
    assert plan(3, 3, 1, 1, 20, 200, 8) == "fxk::eval_kernel<3,1,1> degree=3 P=1 chunks=4"
    for args in [(3, 3, 1, 1, 20, 23), (3, 6, 2, 1, 84, 1), (3, 6, 2, 3, 300, 5), (2, 4, 2, 2, 24, 3), (1, 3, 2, 1, 4, 7), (2, 2, 1, 1, 6, 200)]:
        assert plan(*args) == R.kernel_name(*args), args


def test_host_entries_reject_bad_arguments():
    """FX_EINVAL (ValueError) and FX_ENOTIMPL (NotImplementedError) from the entries that need no device; fx_eval_batch and
    fx_eval_element_create check their arguments before they touch one."""
    buf = ctypes.create_string_buffer(160)
    K = _lib.evallib.fx_eval_kernel
    for bad in [(0, 2, 0, 1, 6, 4, 1), (4, 2, 0, 1, 6, 4, 1), (2, -1, 0, 1, 6, 4, 1), (2, 2, -1, 1, 6, 4, 1), (2, 2, 0, 0, 6, 4, 1),
                (2, 2, 0, 1, 0, 4, 1), (2, 2, 0, 1, 6, -1, 1), (2, 2, 0, 1, 6, 4, 0), (2, 2, 0, 1, 6, 4, 9)]:
        with pytest.raises(ValueError):
            _lib.ser_check(K(*bad, buf, 160))
    with pytest.raises(ValueError):
        _lib.ser_check(K(2, 2, 0, 1, 6, 4, 1, None, 0))
    with pytest.raises(NotImplementedError, match="degree 7"):
        _lib.ser_check(K(2, 7, 0, 1, 36, 4, 1, buf, 160))
    with pytest.raises(NotImplementedError, match="degree 0"):
        _lib.ser_check(K(3, 0, 0, 1, 1, 4, 1, buf, 160))
    with pytest.raises(NotImplementedError, match="order 3"):
        _lib.ser_check(K(3, 2, 3, 1, 10, 4, 1, buf, 160))
    with pytest.raises(NotImplementedError, match="components"):
        _lib.ser_check(K(2, 2, 0, 4, 9, 4, 1, buf, 160))
    with pytest.raises(NotImplementedError, match="entries"):       # 10 * 8 * 3 * npts >= 2^31
        _lib.ser_check(K(3, 2, 2, 3, 20, 9000000, 8, buf, 160))
    assert b"entries" in _lib.lib.fx_last_error()                   # one error slot for the main library and its companions
    c = np.ones(6 * 6)
    with pytest.raises(NotImplementedError, match="dual"):
        _lib.ser_check(_lib.evallib.fx_eval_fold(2, 2, 2, 6, 1, _lib.host_ptr(c), _lib.host_ptr(c.copy())))
    with pytest.raises(ValueError):
        _lib.ser_check(_lib.evallib.fx_eval_fold(2, 2, 0, 6, 1, None, _lib.host_ptr(c)))
    with pytest.raises(ValueError):
        _lib.ser_check(_lib.evallib.fx_eval_walk_order(2, 2, None))
    with pytest.raises(ValueError, match="null context"):
        _lib.ser_check(_lib.evallib.fx_eval_batch(None, None, 0, 0, 1, 4, 1, None, None, None, None, None))
    h = ctypes.c_void_p()
    with pytest.raises(ValueError, match="null argument"):
        _lib.ser_check(_lib.evallib.fx_eval_element_create(None, 2, 2, 0, -1.0, None, 6, 1, _lib.host_ptr(c), ctypes.byref(h)))
    assert _lib.evallib.fx_eval_element_destroy(None) == 0


def test_companion_symbols_and_abi():
    expected = {"fx_eval_abi_version", "fx_eval_walk_order", "fx_eval_fold", "fx_eval_element_create", "fx_eval_element_destroy",
                "fx_eval_kernel", "fx_eval_batch"}
    assert set(_lib.EVAL_EXPORTS) == expected
    for name in _lib.EVAL_EXPORTS:
        assert getattr(_lib.evallib, name) is not None
        for other in (_lib.lib, _lib.serlib, _lib.sflib, _lib.dpclib, _lib.tracelib, _lib.hierlib):
            assert not hasattr(other, name), f"{name} belongs to the evaluation companion"
    for others in (_lib.EXPORTS, _lib.SER_EXPORTS, _lib.SF_EXPORTS, _lib.DPC_EXPORTS, _lib.TRACE_EXPORTS, _lib.HIER_EXPORTS):
        assert set(_lib.EVAL_EXPORTS).isdisjoint(others)
    assert _lib.evallib.fx_eval_abi_version() == 1
    assert _lib.lib.fx_abi_version() == 2
    header = open(os.path.join(ROOT, "include", "fiat_amd_eval.h")).read()
    assert set(re.findall(r"^int (fx_\w+)\(", header, flags=re.M)) == expected
    assert "fx_eval" not in open(os.path.join(ROOT, "include", "fiat_amd.h")).read()
    nm = shutil.which("nm")
    if nm is not None:
        syms = subprocess.run([nm, "-D", "--defined-only", COMPANION], check=True, capture_output=True, text=True).stdout
        exported = {line.split()[-1] for line in syms.splitlines() if " T " in line and line.split()[-1].startswith("fx_")}
        assert exported == expected


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
    src.write_text('#include "fiat_amd_eval.h"\n'
                   "int main(void) {\n"
                   "    int order[10];\n"
                   "    char buf[96];\n"
                   "    fx_eval_element* e = 0;\n"
                   "    double c[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, f[9];\n"
                   "    if (fx_eval_abi_version() != 1 || fx_abi_version() != 2) return 1;\n"
                   "    if (fx_eval_walk_order(3, 2, order) != FX_OK || order[0] != 0 || order[1] != 3 || order[9] != 4) return 2;\n"
                   "    if (fx_eval_fold(2, 1, FX_VARIANT_BUBBLE, 3, 1, c, f) != FX_OK) return 3;\n"
                   "    if (fx_eval_kernel(2, 2, 1, 1, 6, 9, 1, buf, 96) != FX_OK) return 4;\n"
                   "    if (fx_eval_batch(0, e, FX_MAP_AFFINE, 0, 1, 1, 1, 0, 0, 0, 0, 0) != FX_EINVAL) return 5;\n"
                   "    if (fx_eval_element_destroy(e) != FX_OK) return 6;\n"
                   "    return fx_eval_kernel(2, 7, 1, 1, 36, 9, 1, buf, 96) == FX_ENOTIMPL ? 0 : 7;\n"
                   "}\n")
    inc = os.path.join(ROOT, "include")
    lib = os.path.join(ROOT, "fiat_amd", "csrc")
    exe = tmp_path / "abi_check"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{inc}", str(src), f"-L{lib}",
                    "-lfiat_amd_eval", "-lfiat_amd", f"-Wl,-rpath,{lib}", "-o", str(exe)], check=True, capture_output=True)
    assert subprocess.run([str(exe)], capture_output=True).returncode == 0


# every instance ships: none had to be dropped for scratch or VGPR spills
EXPECTED_KERNELS = {f"fxk::eval_kernel<{sd},{o},{v}>" for sd in (1, 2, 3) for o in range(3) for v in {1, sd}}


@pytest.fixture(scope="module")
def companion_report():
    import codeobject_report
    return codeobject_report.kernels(lib=COMPANION, all_units=True)


@needs_llvm
def test_companion_code_object(companion_report):
    """Exactly the 15 instances, no scratch and no VGPR spills."""
    import instance_manifest
    kernels, targets = companion_report
    assert sorted(targets) == ["hipv4-amdgcn-amd-amdhsa--gfx950", "host-x86_64-unknown-linux-gnu-"]
    names = instance_manifest.normalise_all([k["name"] for k in kernels])
    assert len(names) == len(set(names)) == 15
    assert set(names) == EXPECTED_KERNELS, set(names) ^ EXPECTED_KERNELS
    assert all(k["scratch"] == 0 and k["vgpr_spill"] == 0 for k in kernels), [k for k in kernels if k["scratch"] or k["vgpr_spill"]]


@needs_llvm
def test_recorded_resource_usage_matches_the_build(companion_report):
    """profiles/evaluate_resource_usage.txt lists every instance with the VGPR count of the build, 0 scratch and 0 spills."""
    import instance_manifest
    kernels, _ = companion_report
    built = dict(zip(instance_manifest.normalise_all([k["name"] for k in kernels]), (k["vgpr"] for k in kernels)))
    lines = [ln for ln in open(os.path.join(ROOT, "profiles", "evaluate_resource_usage.txt")) if not ln.startswith("#")]
    listed = {"fxk::" + ln.split(" vgpr")[0].strip().replace(", ", ","): int(ln.split(" vgpr")[1].split()[0]) for ln in lines}
    assert set(listed) == EXPECTED_KERNELS
    assert listed == built
    assert all("scratch 0  spill 0" in ln for ln in lines)


@needs_llvm
def test_main_library_kernel_set_unchanged():
    import codeobject_report
    kernels, _ = codeobject_report.kernels(all_units=True)
    assert not [k["name"] for k in kernels if "eval_kernel" in k["name"]]
    nm = shutil.which("nm")
    if nm is not None:
        syms = subprocess.run([nm, "-D", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
        assert "fx_eval" not in syms


def test_fixture_is_plain_numbers_and_small():
    path = os.path.join(HERE, "golden", "evaluate.npz")
    assert os.path.getsize(path) < 500 * 1000
    for key in G.files:
        assert G[key].dtype in (np.float64, np.int64), key
    assert sorted({k.rsplit("_", 1)[0] for k in G.files}) == sorted(M.CASES)
    for name in M.GENERAL_ONLY:
        m = meta(name)
        assert m["n"] > R.MAXK or m["mapping"] > 2
    for name in FUSED:
        m = meta(name)
        assert 1 <= m["n"] <= R.MAXK and m["mapping"] <= 2 and m["variant"] in (0, 1) and m["vdim"] in (1, m["sd"])
