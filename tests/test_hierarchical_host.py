"""IntegratedLegendre, host side (no GPU): the NumPy restatement of the C0 hierarchy against the reference's fixtures
(tests/golden/hierarchical.npz), the diagonal structure of the reference's coefficients, the C dof table, and the companion
library libfiat_amd_hier.so -- its symbols, header, code object, kernel set and scratch -- with the kernel set of
libfiat_amd.so left as it was."""
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

import hierarchical_reference as R  # noqa: E402
import make_golden_hierarchical as M  # noqa: E402

from fiat_amd import _lib  # noqa: E402

G = np.load(os.path.join(HERE, "golden", "hierarchical.npz"))
SD = {"int": 1, "tri": 2, "tet": 3}
STANDING = (1e-12, 1e-10)
DIRECT = sorted(n for n, c in M.CASES.items() if c[1] <= 6 and c[3] <= 2)
COMPANION = os.path.join(ROOT, "fiat_amd", "csrc", "libfiat_amd_hier.so")
needs_llvm = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/clang-offload-bundler"),
                                reason="needs the LLVM tools of ROCm")


def errors(got, ref):
    e0 = R.table_error(got[:1], ref[:1])
    e1 = R.table_error(got[1:], ref[1:]) if ref.shape[0] > 1 else 0.0
    return e0, e1


def dims_of(name):
    """Entity dimension per dof, from the fixture's entity ids."""
    eids = G[f"{name}_eids"]
    dims = np.full(int(G[f"{name}_meta"][1]), -1)
    dims[eids[:, 2]] = eids[:, 0]
    return dims


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_restatement_against_fixture(name):
    """The float64 restatement against every table of the reference, at the standing 1e-12 / 1e-10 (orders 0-2; the order-3
    tables of tet3o3 are the general route's and have no restatement)."""
    c, k, _, order = M.CASES[name]
    sd = SD[c]
    ref = G[f"{name}_tab"]
    upto = min(order, 2)
    ntab = sum(len(R.mis(sd, o)) for o in range(upto + 1))
    assert ref.shape[1] == len(R.dof_table(sd, k)) and ref.shape[0] == sum(len(R.mis(sd, o)) for o in range(order + 1))
    e0, e1 = errors(R.tabulate(sd, k, upto, G[f"{name}_pts"]), ref[:ntab])
    print(f"{name}: values {e0:.2e} derivatives {e1:.2e}")
    assert e0 <= STANDING[0] and e1 <= STANDING[1], (name, e0, e1)
    assert list(G[f"{name}_meta"]) == [k, len(R.dof_table(sd, k)), 0, sd]


def test_entity_tables_against_fixture():
    """The fixtures' ``entity=`` tables: the restatement at the points mapped into the cell."""
    v = {2: np.array([[0, 0], [1, 0], [0, 1.0]]), 3: np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1.0]])}
    edges = {0: (1, 2), 1: (0, 2), 2: (0, 1)}
    faces = {0: (1, 2, 3), 1: (0, 2, 3), 2: (0, 1, 3), 3: (0, 1, 2)}
    for name in M.ENTITY:
        c, k, _, _ = M.CASES[name]
        sd = SD[c]
        dim, number = (int(x) for x in G[f"{name}_e_ent"])
        ids = (edges if dim == 1 else faces)[number]
        w = v[sd][list(ids)]
        x = w[0] + G[f"{name}_e_pts"] @ (w[1:] - w[0])
        e0, e1 = errors(R.tabulate(sd, k, 1, x), G[f"{name}_e_tab"])
        print(f"{name} entity {(dim, number)}: values {e0:.2e} derivatives {e1:.2e}")
        assert e0 <= STANDING[0] and e1 <= STANDING[1]


def test_reference_drift_from_extended_precision():
    """Distance of the float64 restatement, and of the reference's fixture, from the restatement in extended precision
    (``longdouble``, 80 bits here), in the project's norm over orders 0-2, at the fixture's points (vertices, an edge midpoint,
    the barycentre, six seeded points, two points up to 0.2 outside).  Measured on the CPU of the build container; the printed
    table is the record (run with -s).  The reference carries the round-off of its Vandermonde solve, which grows with the
    degree; the restatement has none.  Asserted: the restatement stays within 2e-14 of extended precision -- at most 6 chained
    three-term steps per level and three levels, each step a handful of rounded operations on entries the norm's denominator
    bounds, Hessians included -- and the fixture stays within the standing tolerance of it."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("no extended precision on this host")
    for name in DIRECT:
        c, k, _, order = M.CASES[name]
        sd = SD[c]
        pts = G[f"{name}_pts"]
        ext = R.tabulate(sd, k, order, pts, longdouble=True)
        own = errors(R.tabulate(sd, k, order, pts).astype(np.longdouble), ext)
        ref = errors(G[f"{name}_tab"].astype(np.longdouble), ext)
        print(f"{name}: restatement {own[0]:.1e} {own[1]:.1e}   reference {ref[0]:.1e} {ref[1]:.1e}")
        assert max(own) <= 2e-14, (name, own)
        assert ref[0] <= STANDING[0] and ref[1] <= STANDING[1], (name, ref)


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_coefficients_are_diagonal_with_one_scale_per_entity_dimension(name):
    """get_coeffs() of the reference: off-diagonal <= 1e-11, and the diagonal is SCALES[sd][entity dimension] at every
    degree (to 1e-11: the reference's solve noise), which the closed form ``scales`` reproduces to the printed digits."""
    c, k, _, _ = M.CASES[name]
    sd = SD[c]
    C = G[f"{name}_coeffs"]
    assert C.shape == (len(R.dof_table(sd, k)),) * 2
    off = np.abs(C - np.diag(np.diag(C))).max()
    dims = dims_of(name)
    assert list(dims) == [d for _, d in R.dof_table(sd, k)]
    assert off <= 1e-11, (name, off)
    for dim in sorted(set(dims)):
        diag = np.diag(C)[dims == dim]
        assert np.abs(diag - R.SCALES[sd][dim]).max() <= 1e-11, (name, dim, diag)
        assert abs(np.median(diag) - R.scales(sd)[dim]) <= 1e-11
    assert np.allclose(R.scales(sd), R.SCALES[sd], rtol=0, atol=1e-12)


def c_descriptor(sd, k):
    rows = np.full((len(R.dof_table(sd, k)), 4), 99, dtype=np.int32)
    _lib.check(_lib.hierlib.fx_hier_descriptor(sd, k, _lib.host_ptr(rows)))
    return rows


def python_descriptor(sd, k):
    return np.array([list(idx) + [0] * (3 - sd) + [dim] for idx, dim in R.dof_table(sd, k)], dtype=np.int32)


@pytest.mark.parametrize("name", DIRECT)
def test_c_descriptor_equals_the_fixture_and_the_restatement(name):
    c, k, _, _ = M.CASES[name]
    sd = SD[c]
    rows = c_descriptor(sd, k)
    assert np.array_equal(rows, python_descriptor(sd, k))
    assert list(rows[:, 3]) == list(dims_of(name))
    assert len({tuple(r[:3]) for r in rows}) == len(rows) and rows[:, :3].sum(axis=1).max() == k


@pytest.mark.parametrize("sd", [1, 2, 3])
def test_c_descriptor_equals_python_beyond_the_fixtures(sd):
    for k in range(1, 13):
        assert np.array_equal(c_descriptor(sd, k), python_descriptor(sd, k)), k


def plan(sd, k, order, npts):
    buf = ctypes.create_string_buffer(160)
    _lib.check(_lib.hierlib.fx_hier_kernel(sd, k, order, npts, buf, 160))
    return buf.value.decode()


def test_host_entries_reject_bad_arguments():
    rows = np.zeros((100, 4), dtype=np.int32)
    with pytest.raises(ValueError):
        _lib.check(_lib.hierlib.fx_hier_descriptor(4, 2, _lib.host_ptr(rows)))
    with pytest.raises(ValueError):
        _lib.check(_lib.hierlib.fx_hier_descriptor(2, 0, _lib.host_ptr(rows)))
    with pytest.raises(ValueError):
        _lib.check(_lib.hierlib.fx_hier_descriptor(2, 2, None))
    buf = ctypes.create_string_buffer(128)
    with pytest.raises(ValueError):
        _lib.check(_lib.hierlib.fx_hier_kernel(0, 2, 0, 4, buf, 128))
    with pytest.raises(ValueError):
        _lib.check(_lib.hierlib.fx_hier_kernel(2, 2, -1, 4, buf, 128))
    with pytest.raises(ValueError):
        _lib.check(_lib.hierlib.fx_hier_kernel(2, 2, 0, 4, None, 0))
    with pytest.raises(NotImplementedError, match="degree 7"):
        _lib.check(_lib.hierlib.fx_hier_kernel(2, 7, 0, 4, buf, 128))
    with pytest.raises(NotImplementedError, match="degree 0"):
        _lib.check(_lib.hierlib.fx_hier_kernel(3, 0, 0, 4, buf, 128))
    with pytest.raises(NotImplementedError, match="order 3"):
        _lib.check(_lib.hierlib.fx_hier_kernel(3, 2, 3, 4, buf, 128))
    with pytest.raises(NotImplementedError, match="entries"):      # 10 * 84 * npts >= 2^31
        _lib.check(_lib.hierlib.fx_hier_kernel(3, 6, 2, 2600000, buf, 128))
    # the error text lands in the main library's slot: one fx_last_error for both
    assert b"entries" in _lib.lib.fx_last_error()
    # the batch entry checks its arguments before it touches the device
    A, b = R.ufc_map(2)
    s = np.ones(4)
    with pytest.raises(ValueError, match="null context"):
        _lib.check(_lib.hierlib.fx_hier_tabulate_batch(None, 2, 2, 0, _lib.host_ptr(s), None, 1, 4, None, None,
                                                       _lib.host_ptr(A), _lib.host_ptr(b)))


def test_route_report():
    assert plan(3, 3, 1, 23) == "fxk::hier_kernel<3,3,1> image P=2"          # 4 * 20 * 23 doubles: 2 requests are 29 KB
    assert plan(3, 6, 2, 23) == "fxk::hier_kernel<3,6,2> stream P=2"         # 154 560 B
    assert plan(2, 4, 1, 6) == "fxk::hier_kernel<2,4,1> image P=10"          # 2 160 B each
    assert plan(3, 6, 2, 6) == "fxk::hier_kernel<3,6,2> image P=1"           # 40 320 B
    assert plan(3, 6, 2, 7) == "fxk::hier_kernel<3,6,2> stream P=9"          # 47 040 B
    assert plan(1, 1, 0, 1) == "fxk::hier_kernel<1,1,0> image P=64"
    assert plan(1, 1, 0, 65) == "fxk::hier_kernel<1,1,0> image P=1"          # chunks of 64 points, still an image
    assert plan(2, 6, 2, 130) == "fxk::hier_kernel<2,6,2> stream P=1"


def test_companion_symbols_and_abi():
    assert set(_lib.HIER_EXPORTS) == {"fx_hier_abi_version", "fx_hier_descriptor", "fx_hier_kernel", "fx_hier_tabulate_batch"}
    for name in _lib.HIER_EXPORTS:
        assert getattr(_lib.hierlib, name) is not None
        for other in (_lib.lib, _lib.serlib, _lib.sflib, _lib.dpclib, _lib.tracelib):
            assert not hasattr(other, name), f"{name} belongs to the hierarchical companion"
    for others in (_lib.EXPORTS, _lib.SER_EXPORTS, _lib.SF_EXPORTS, _lib.DPC_EXPORTS, _lib.TRACE_EXPORTS):
        assert set(_lib.HIER_EXPORTS).isdisjoint(others)
    assert _lib.hierlib.fx_hier_abi_version() == 1
    assert _lib.lib.fx_abi_version() == 2
    header = open(os.path.join(ROOT, "include", "fiat_amd_hier.h")).read()
    declared = set(re.findall(r"^int (fx_\w+)\(", header, flags=re.M))
    assert declared == set(_lib.HIER_EXPORTS)
    assert "hier" not in open(os.path.join(ROOT, "include", "fiat_amd.h")).read().lower()
    nm = shutil.which("nm")
    if nm is not None:
        syms = subprocess.run([nm, "-D", "--defined-only", COMPANION], check=True, capture_output=True, text=True).stdout
        exported = {line.split()[-1] for line in syms.splitlines() if " T " in line and line.split()[-1].startswith("fx_")}
        assert exported == set(_lib.HIER_EXPORTS)


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
    src.write_text('#include "fiat_amd_hier.h"\n'
                   "int main(void) {\n"
                   "    int rows[10 * 4];\n"
                   "    char buf[96];\n"
                   "    if (fx_hier_abi_version() != 1 || fx_abi_version() != 2) return 1;\n"
                   "    if (fx_hier_descriptor(3, 2, rows) != FX_OK || rows[1 * 4] != 1 || rows[4 * 4 + 1] != 1 || rows[4 * 4 + 3] != 1) return 2;\n"
                   "    if (fx_hier_kernel(2, 2, 1, 9, buf, 96) != FX_OK) return 3;\n"
                   "    return fx_hier_kernel(2, 7, 1, 9, buf, 96) == FX_ENOTIMPL ? 0 : 4;\n"
                   "}\n")
    inc = os.path.join(ROOT, "include")
    lib = os.path.join(ROOT, "fiat_amd", "csrc")
    exe = tmp_path / "abi_check"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{inc}", str(src), f"-L{lib}",
                    "-lfiat_amd_hier", "-lfiat_amd", f"-Wl,-rpath,{lib}", "-o", str(exe)], check=True, capture_output=True)
    assert subprocess.run([str(exe)], capture_output=True).returncode == 0


# every instance of the switch ships: none had to be dropped for scratch or VGPR spills
EXPECTED_KERNELS = {f"fxk::hier_kernel<{sd},{k},{o}>" for sd in (1, 2, 3) for k in range(1, 7) for o in range(3)}


@pytest.fixture(scope="module")
def companion_report():
    import codeobject_report
    return codeobject_report.kernels(lib=COMPANION, all_units=True)


@needs_llvm
def test_companion_code_object(companion_report):
    """Exactly the 54 instances, no scratch and no VGPR spills."""
    import instance_manifest
    kernels, targets = companion_report
    assert sorted(targets) == ["hipv4-amdgcn-amd-amdhsa--gfx950", "host-x86_64-unknown-linux-gnu-"]
    names = instance_manifest.normalise_all([k["name"] for k in kernels])
    assert len(names) == len(set(names)) == 54
    assert set(names) == EXPECTED_KERNELS, set(names) ^ EXPECTED_KERNELS
    assert all(k["scratch"] == 0 and k["vgpr_spill"] == 0 for k in kernels), [k for k in kernels if k["scratch"] or k["vgpr_spill"]]


@needs_llvm
def test_recorded_resource_usage_matches_the_build(companion_report):
    """profiles/hier_resource_usage.txt lists every instance with the VGPR count of the build, 0 scratch and 0 spills."""
    import instance_manifest
    kernels, _ = companion_report
    built = dict(zip(instance_manifest.normalise_all([k["name"] for k in kernels]), (k["vgpr"] for k in kernels)))
    lines = [ln for ln in open(os.path.join(ROOT, "profiles", "hier_resource_usage.txt")) if not ln.startswith("#")]
    listed = {"fxk::" + ln.split(" vgpr")[0].strip().replace(", ", ","): int(ln.split(" vgpr")[1].split()[0]) for ln in lines}
    assert set(listed) == EXPECTED_KERNELS
    assert listed == built
    assert all("scratch 0  spill 0" in ln for ln in lines)


@needs_llvm
def test_main_library_kernel_set_unchanged():
    import codeobject_report
    kernels, _ = codeobject_report.kernels(all_units=True)
    assert not [k["name"] for k in kernels if "hier" in k["name"].lower()]
    nm = shutil.which("nm")
    if nm is not None:
        syms = subprocess.run([nm, "-D", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
        assert "fx_hier" not in syms.lower()


def test_fixture_is_plain_numbers_and_small():
    path = os.path.join(HERE, "golden", "hierarchical.npz")
    assert os.path.getsize(path) < 500 * 1000
    for key in G.files:
        assert G[key].dtype in (np.float64, np.int64, np.uint8), key
    assert list(G["raises_degree0"]) == [1]
    assert bytes(G["raises_text"]).decode() == "IntegratedLegendre elements only valid for k >= 1"


def test_registry_key_and_constructor_errors():
    """The key and the degree check need no device: the ValueError is raised before anything is constructed."""
    import fiat_amd
    from fiat_amd import hierarchical
    assert fiat_amd.supported_elements["Integrated Legendre"] is fiat_amd.IntegratedLegendre is hierarchical.IntegratedLegendre
    for cell in (fiat_amd.ufc_simplex(1), fiat_amd.ufc_simplex(2), fiat_amd.ufc_simplex(3)):
        for k in (0, -1):
            with pytest.raises(ValueError, match=bytes(G["raises_text"]).decode()):
                fiat_amd.IntegratedLegendre(cell, k)
    assert hierarchical.HIER_KERNEL_MAXK == 6 and hierarchical.HIER_KERNEL_MAXORDER == 2
