"""Hdiv / Hcurl / EnrichedElement, host side (no GPU): the new C ABI symbols, the reference's tables of the quadrilateral /
hexahedral families (tests/golden/hdivcurl.npz) against a NumPy restatement of the fused kernel's rule, and the resources of
the new translation unit's kernels."""
import os
import sys

import numpy as np
import pytest

from fiat_amd import _lib
from fiat_amd.polynomial_set import mis

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_hdivcurl as M  # noqa: E402

G = np.load(os.path.join(ROOT, "tests", "golden", "hdivcurl.npz"))
HDC_OBJ = os.path.join(ROOT, "fiat_amd", "csrc", "hdivcurl.o")


def line_tables(nodes, x, order):
    """(order+1, n, npts): the 1-D Lagrange basis on ``nodes`` and its derivatives at x (barycentric form)."""
    nodes = np.asarray(nodes, dtype=float)
    n = len(nodes)
    out = np.zeros((order + 1, n, len(x)))
    for i in range(n):
        others = np.delete(nodes, i)
        denom = np.prod(nodes[i] - others)
        coef = np.poly(others) / denom if n > 1 else np.array([1.0])
        for k in range(order + 1):
            out[k, i] = np.polyval(np.polyder(coef, k) if k else coef, x)
    return out


def restated(kind, C, D, blocks, sd, order, pts):
    """(ntab, ndof, sd, npts): block c = sign * row-major product over d of C (H(div): d == c; H(curl): d != c) or D."""
    TC = [line_tables(C, pts[:, d], order) for d in range(sd)]
    TD = [line_tables(D, pts[:, d], order) for d in range(sd)]
    alphas = [a for k in range(order + 1) for a in mis(sd, k)]
    nb = len(C) * len(D) ** (sd - 1) if kind == "div" else len(D) * len(C) ** (sd - 1)
    out = np.zeros((len(alphas), nb * len(blocks), sd, len(pts)))
    for c, (off, sign) in blocks.items():
        fac = [TC[d] if (d == c) == (kind == "div") else TD[d] for d in range(sd)]
        for t, a in enumerate(alphas):
            prod = fac[0][a[0]]
            for d in range(1, sd):
                prod = (prod[:, None, :] * fac[d][a[d]][None, :, :]).reshape(-1, len(pts))
            out[t, off:off + nb, c] = sign * prod
    return out


def blocks_from_reference(tab, sd):
    """{component: (dof offset, sign)} read off the reference's value table: every dof has exactly one nonzero component."""
    ndof = tab.shape[1]
    comps = [int(np.argmax(np.abs(tab[0, i]).max(-1))) for i in range(ndof)]
    out = {}
    for c in sorted(set(comps)):
        rows = [i for i in range(ndof) if comps[i] == c]
        assert rows == list(range(rows[0], rows[0] + len(rows)))             # a contiguous range
        out[c] = rows[0]
    return out, comps


def kind_of(name):
    return "div" if name.startswith(("rtcf", "ncf", "sdiv")) else "curl"


@pytest.mark.parametrize("name", M.QUADHEX)
def test_fixture_matches_the_restated_rule(name):
    tab, pts = G[f"{name}_tab"], G[f"{name}_pts"]
    sd = pts.shape[1]
    order = M.max_order(name)
    starts, comps = blocks_from_reference(tab, sd)
    for i, c in enumerate(comps):   # the other components are exact zeros
        others = [e for e in range(sd) if e != c]
        assert np.all(tab[:, i, others] == 0.0)
    blocks = {}
    for c, off in starts.items():
        nb = sum(1 for cc in comps if cc == c)
        probe = restated(kind_of(name), G[f"{name}_c"], G[f"{name}_d"], {c: (0, 1)}, sd, order, pts)[:, :nb]
        ref = tab[:, off:off + nb]
        sign = 1 if np.abs(ref - probe).max() < np.abs(ref + probe).max() else -1
        blocks[c] = (off, sign)
    got = restated(kind_of(name), G[f"{name}_c"], G[f"{name}_d"], blocks, sd, order, pts)
    scale = max(1.0, np.abs(tab).max())
    assert np.abs(got - tab).max() <= 1e-10 * scale
    # the signs the descriptor rules give: Hdiv puts A's 0-form table in component 0 with sign -1, everything else +1
    for c, (_, sign) in blocks.items():
        assert sign == (-1 if kind_of(name) == "div" and c == 0 else 1)


@pytest.mark.parametrize("name", ["rtce2d0", "nce2d0", "rtce3s0"])
def test_rtce_nce_put_component_one_first(name):
    starts, _ = blocks_from_reference(G[f"{name}_tab"], G[f"{name}_pts"].shape[1])
    assert starts[1] == 0


def test_c_abi_symbols():
    for name in ("fx_hdivcurl_tabulate_batch", "fx_hdivcurl_tabulate_grid_batch", "fx_table_place_batch"):
        assert name in _lib.EXPORTS
        assert getattr(_lib.lib, name) is not None
    header = open(os.path.join(ROOT, "include", "fiat_amd.h")).read()
    for name in ("fx_hdivcurl_tabulate_batch", "fx_hdivcurl_tabulate_grid_batch", "fx_table_place_batch"):
        assert f"int {name}(" in header
    assert _lib.lib.fx_abi_version() == 2


def test_exports():
    import fiat_amd
    assert fiat_amd.Hdiv and fiat_amd.Hcurl and fiat_amd.EnrichedElement
    assert "EnrichedElement" not in fiat_amd.supported_elements and "Hdiv" not in fiat_amd.supported_elements


@pytest.mark.skipif(not os.path.exists(HDC_OBJ) or not os.path.exists("/opt/rocm/lib/llvm/bin/clang-offload-bundler"),
                    reason="needs the built hdivcurl.o and the LLVM tools of ROCm")
def test_translation_unit_has_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobject_report
    kernels, _ = codeobject_report.kernels(HDC_OBJ)
    fused = [k for k in kernels if "hdivcurl_kernel" in k["name"]]
    assert len(fused) == (4 + 3) * 3 * 2 * 2            # (K quad + K hex) x orders x kinds x (points, grid)
    assert any("table_place_kernel" in k["name"] for k in kernels)
    for k in kernels:
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0, k
