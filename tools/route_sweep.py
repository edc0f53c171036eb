#!/usr/bin/env python3
"""Which kernel the planner picks for every request shape of a grid, written to a file (needs the GPU's context, launches no
tabulation kernel): python tools/route_sweep.py [--digest | --digest-hash] OUT.  Run it once per library --
FIAT_AMD_LIB=.../libfiat_amd.so -- and compare the files with diff: a change to the registries or to plan_launch
(csrc/api.hip) that is meant to keep every route must leave them identical.

Grid: Lagrange, DG, both Nedelec kinds, RT, BDM and the matrix-valued families at every degree the registries hold, raw
scalar expansion sets of degree 0-8 on intervals, triangles and tetrahedra, the six lane-local macro shapes, one random
set of 75 rows; 1-130 points; orders 0-2; own cell / per-request cells / cells + the element's Piola map; batches of 1 and 100000 requests; the default
policy and every name of _lib.POLICY on its own.  One line per (policy, element, order, mode, batch): the report of
kernel_name(..., instance=True) -- MacroPolySet.kernel_name for macro elements -- over the point counts, runs of equal
reports folded into "first-last:name".  The last line counts the request shapes behind the file.  The macro lines come from
MacroPolySet.kernel_name, which mirrors the selection in Python: they pin that mirror, not the library's macro registry.

The names alone do not pin a plan: a change can keep every name and still move a grid, an LDS size, the requests per item or
a coefficient.  --digest asks for kernel_name(..., digest=True): every report is followed by "{...}", the launch itself --
family, registry row, grid, dynamic LDS bytes, every integer its launcher reads, which device table was chosen and a 64-bit
hash of the floating-point arguments; no pointer value.  The folding stays, but nearly every point count is now a run of its
own: about a gigabyte for the whole grid.  --digest-hash writes one short line per (policy, element, order),
"<policy> <element> order=<k> | digest <sha-256, 16 hex digits>", over the --digest lines of all its modes and batches: as
strict, sixty bytes where those are a few hundred kilobytes; a line that differs between two libraries is then looked at
with --digest --only "<start of the line>" (the lines that start with it)."""
import hashlib
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


def family_element(fam, sd, deg):
    """(label, device polynomial set, mapping) of one family member"""
    el = getattr(fiat_amd, fam)(fiat_amd.ufc_simplex(sd), deg)
    return f"{fam},{sd},{deg}", el.device_polyset(), el.mapping()[0]


def random_element():
    """75 random members over the degree-3 set of the tetrahedron: an odd number of rows in the fifth row tile, which no family
    has -- the shape the register-resident stacked rows take with odd tables under policy stacked_small"""
    cell = fiat_amd.ufc_simplex(3)
    es = fiat_amd.ExpansionSet(cell)
    coeffs = np.random.default_rng(75).standard_normal((75, es.get_num_members(3))) / 5.0
    return "Random/75,3,3", fiat_amd.PolynomialSet(cell, 3, 3, es, coeffs).device_polyset(), "affine"


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
                    label, ps, mapping = family_element(fam, sd, deg)
                except Exception as e:
                    print(f"# no element {fam},{sd},{deg}: {str(e)[:70]}", flush=True)
                    continue
                if isinstance(ps, runtime.SimplexPolySet):
                    yield label, ps, mapping
    yield random_element()
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


def sweep_lines(ctx, els, policies, digest=None, points=POINTS, nreqs=NREQ, only=None):
    """The lines of the sweep over `els` [(label, set, mapping)] and `policies` [tuple of names] as (line, request shapes behind
    it): one per (policy, element, order, mode, batch), or with digest="hash" one per (policy, element, order) over the
    digest="full" lines of its modes and batches (module docstring); only: keep the lines that start with it.  Leaves the
    context on the last policy."""
    for pol in policies:
        ctx.set_policy(*pol)
        for label, ps, mapping in els:
            macro = isinstance(ps, runtime.MacroPolySet)
            modes = [("own", False, None), ("cells", True, None)]
            if not macro and mapping in ("covariant piola", "contravariant piola"):
                modes.append(("piola", True, mapping))
            for order in (0, 1, 2):
                block = []
                for mode, cells, m in modes:
                    for nreq in nreqs:
                        head = f"{','.join(pol) or 'default'} {label} order={order} {mode} nreq={nreq}"
                        if only and not head.startswith(only):
                            continue
                        if macro:
                            names = [(n, ps.kernel_name(order, nreq, n, has_verts=cells)) for n in points]
                        else:
                            names = [(n, ps.kernel_name(order, nreq, n, has_verts=cells, instance=True, mapping=m, digest=bool(digest)))
                                     for n in points]
                        block.append((f"{head} | {folded(names)}", len(names)))
                if digest == "hash" and block:
                    sha = hashlib.sha256("\n".join(line for line, _ in block).encode()).hexdigest()[:16]
                    yield f"{','.join(pol) or 'default'} {label} order={order} | digest {sha}", sum(n for _, n in block)
                else:
                    yield from block


def main(out_path, digest=None, only=None):
    ctx = runtime.Context.get()
    els = list(elements())
    shapes = 0
    with open(out_path, "w") as out:
        for pol in [()] + [(p,) for p in _lib.POLICY]:
            for line, n in sweep_lines(ctx, els, [pol], digest, only=only):
                out.write(line + "\n")
                shapes += n
            print(f"policy {','.join(pol) or 'default'} done", flush=True)
        ctx.set_policy()
        out.write(f"# {len(els)} elements, {shapes} request shapes\n")
    print(f"{len(els)} elements, {shapes} request shapes -> {out_path}")


if __name__ == "__main__":
    args = sys.argv[1:]
    digest = "full" if "--digest" in args else "hash" if "--digest-hash" in args else None
    only = args[args.index("--only") + 1] if "--only" in args else None
    rest = [a for a in args if a not in ("--digest", "--digest-hash", "--only", only)]
    if len(rest) != 1:
        sys.exit(__doc__)
    main(rest[0], digest, only)
