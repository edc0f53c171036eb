#!/usr/bin/env python3
"""Which kernel the planner picks for every request shape of a grid, written to a file (needs the GPU's context, launches no
tabulation kernel): python tools/route_sweep.py OUT.  Run it once per library -- FIAT_AMD_LIB=.../libfiat_amd.so -- and
compare the files with diff: a change to the registries or to plan_launch (csrc/api.hip) that is meant to keep every route
must leave them identical.

Grid: Lagrange, DG, both Nedelec kinds, RT, BDM and the matrix-valued families at every degree the registries hold, raw
scalar expansion sets of degree 0-8 on intervals, triangles and tetrahedra, the six lane-local macro shapes, one random
set of 75 rows; 1-130 points; orders 0-2; own cell / per-request cells / cells + the element's Piola map; batches of 1 and 100000 requests; the default
policy and every name of _lib.POLICY on its own.  One line per (policy, element, order, mode, batch): the report of
kernel_name(..., instance=True) -- MacroPolySet.kernel_name for macro elements -- over the point counts, runs of equal
reports folded into "first-last:name".  The last line counts the request shapes behind the file.  The macro lines come from
MacroPolySet.kernel_name, which mirrors the selection in Python: they pin that mirror, not the library's macro registry."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fiat_amd  # noqa: E402
from fiat_amd import _lib, runtime  # noqa: E402

POINTS = range(1, 131)
NREQ = (1, 100000)
FAMILIES = [("Lagrange", range(1, 9)), ("DiscontinuousLagrange", range(0, 9)), ("Nedelec", range(1, 5)),
            ("NedelecSecondKind", range(1, 5)), ("RaviartThomas", range(1, 5)), ("BrezziDouglasMarini", range(1, 5)),
            ("Regge", range(0, 4)), ("HellanHerrmannJohnson", range(0, 4)), ("GopalakrishnanLedererSchoberlSecondKind", range(0, 4))]
MACRO = [("Lagrange", 2, 1, "equispaced,iso"), ("Lagrange", 2, 2, "equispaced,alfeld"), ("Lagrange", 2, 3, "equispaced,alfeld"),
         ("Lagrange", 3, 1, "equispaced,iso"), ("Lagrange", 3, 2, "equispaced,alfeld"), ("Lagrange", 3, 3, "equispaced,alfeld")]


def elements():
    """(label, device polynomial set, mapping) of every element of the grid; a family without a degree is skipped."""
    for sd in (1, 2, 3):
        cell = fiat_amd.ufc_simplex(sd)
        for deg in range(0, 9):
            yield f"ONPolynomialSet,{sd},{deg}", fiat_amd.ONPolynomialSet(cell, deg).device_polyset(), "affine"
        for fam, degs in FAMILIES if sd > 1 else []:
            for deg in degs:
                if sd == 3 and deg > (7 if fam in ("Lagrange", "DiscontinuousLagrange") else 3):
                    continue
                try:
                    el = getattr(fiat_amd, fam)(cell, deg)
                    ps = el.device_polyset()
                except Exception as e:
                    print(f"# no element {fam},{sd},{deg}: {str(e)[:70]}", flush=True)
                    continue
                if isinstance(ps, runtime.SimplexPolySet):
                    yield f"{fam},{sd},{deg}", ps, el.mapping()[0]
    # 75 random members over the degree-3 set of the tetrahedron: an odd number of rows in the fifth row tile, which no family
    # has -- the shape the register-resident stacked rows take with odd tables under policy stacked_small
    cell = fiat_amd.ufc_simplex(3)
    es = fiat_amd.ExpansionSet(cell)
    coeffs = np.random.default_rng(75).standard_normal((75, es.get_num_members(3))) / 5.0
    yield "Random/75,3,3", fiat_amd.PolynomialSet(cell, 3, 3, es, coeffs).device_polyset(), "affine"
    for fam, sd, deg, variant in MACRO:
        el = getattr(fiat_amd, fam)(fiat_amd.ufc_simplex(sd), deg, variant)
        yield f"{fam}[{variant}],{sd},{deg}", el.device_polyset(), "affine"


def folded(names):
    """[(npts, name)] in point order -> 'first-last:name ...'"""
    runs = []
    for npts, name in names:
        if runs and runs[-1][2] == name:
            runs[-1][1] = npts
        else:
            runs.append([npts, npts, name])
    return " ".join(f"{a}-{b}:{n}" for a, b, n in runs)


def main(out_path):
    ctx = runtime.Context.get()
    els = list(elements())
    shapes = 0
    with open(out_path, "w") as out:
        for pol in [()] + [(p,) for p in _lib.POLICY]:
            ctx.set_policy(*pol)
            for label, ps, mapping in els:
                macro = isinstance(ps, runtime.MacroPolySet)
                modes = [("own", False, None), ("cells", True, None)]
                if not macro and mapping in ("covariant piola", "contravariant piola"):
                    modes.append(("piola", True, mapping))
                for order in (0, 1, 2):
                    for mode, cells, m in modes:
                        for nreq in NREQ:
                            if macro:
                                names = [(n, ps.kernel_name(order, nreq, n, has_verts=cells)) for n in POINTS]
                            else:
                                names = [(n, ps.kernel_name(order, nreq, n, has_verts=cells, instance=True, mapping=m)) for n in POINTS]
                            shapes += len(names)
                            out.write(f"{','.join(pol) or 'default'} {label} order={order} {mode} nreq={nreq} | {folded(names)}\n")
            print(f"policy {','.join(pol) or 'default'} done", flush=True)
        ctx.set_policy()
        out.write(f"# {len(els)} elements, {shapes} request shapes\n")
    print(f"{len(els)} elements, {shapes} request shapes -> {out_path}")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
