#!/usr/bin/env python3
"""Which request shape reaches which compiled kernel (a tool, run on the MI355X; not part of the suite).

  python tools/instance_search.py --walk DIR [--part simplex,cells,other]   launch candidates, record what ran (DIR/*.jsonl)
  python tools/instance_search.py --select DIR [--write]                     (no GPU) cheapest reaching shape per kernel;
                                                                             prints the kernels never reached; --write puts
                                                                             the cases into tests/instance_manifest.py

The walk goes through the entry points of tests/instance_runner.py: the element families of tools/coverage_map*.py and the raw
expansion sets, degrees 0-8, orders 0-2, point counts on both sides of the planner's window edges (even and odd table sizes),
own cell / per-request cells / the element's Piola map, the default policy and every FX_POLICY_* opt-in / opt-out (plus the
combinations the parity tests use), one reference point set in many cells, macro / tensor / grid / prism / Bernstein /
H(div) / H(curl) elements and the auxiliary kernels.  fx_plan_kernel (host code, launches nothing) prunes the simplex walk:
for one (element, order, points, cells, map) a policy is only launched when the planner's report differs from the ones
already taken.  Kernel selection does not depend on the batch size (plan_launch reads nreq only for grid sizes), so every
candidate is a batch of NREQ requests: a count below the grid that leaves a partial last group for every packing factor.
Every candidate runs once unrecorded (lazy set-up: stacked matrices, differentiation matrices) and once under
torch.profiler; a batch of candidates shares one profiler session, separated by marker kernels."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import instance_manifest as M  # noqa: E402

NREQ = 37
MAX_BYTES = 48 << 20            # output of one candidate
POINTS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13, 15, 16, 17, 23, 24, 25, 31, 32, 33, 47, 48, 49, 50, 63, 64, 65, 74, 79, 80, 95, 96,
          97, 122, 127, 128, 129]
POLICY_SETS = [()] + [(p,) for p in M.POLICIES] + [
    ("no_fixed", "no_stacked", "no_wg"), ("no_fixed", "no_stacked", "no_coop", "no_small"), ("no_stacked", "no_small"),
    ("wg_small", "no_fixed", "no_small"), ("wg_small", "no_fixed", "no_small", "no_stacked_mix"), ("no_stacked_mix", "wg_small"),
    ("no_fixed", "no_stacked"), ("no_fixed", "no_small"), ("no_fixed", "no_stacked", "no_small"), ("no_fixed", "no_stacked_mix"),
    ("no_wg", "no_stacked_mix"), ("no_fixed", "no_wg"), ("no_fixed", "no_stacked", "no_wg", "no_small"),
    ("no_fixed", "no_stacked", "no_wg", "no_coop"), ("stacked_small", "no_fixed")]
SIMPLEX = [("Lagrange", range(1, 9)), ("DiscontinuousLagrange", range(0, 8)), ("Nedelec", range(1, 5)), ("RaviartThomas", range(1, 5)),
           ("BrezziDouglasMarini", range(1, 4)), ("NedelecSecondKind", range(1, 4)), ("ONPolynomialSet", range(0, 9)),
           ("Lagrange-1", range(2, 8)), ("RaviartThomas-1", range(1, 4)), ("VectorON", range(0, 7)),
           # sub-spaces of few rows (PolynomialSet.take): row-tile classes no whole family of that degree has
           ("Lagrange/40", range(5, 7)), ("Lagrange/17", range(4, 7)), ("RaviartThomas/12", range(1, 5)), ("Nedelec/12", range(1, 5)),
           ("RaviartThomas/6", range(1, 5)), ("BrezziDouglasMarini/11", range(2, 4)), ("Lagrange/41", range(5, 7)), ("VectorON/33", range(5, 7))] + \
          [(f"Random/{k}", range(3, 7)) for k in (23, 29, 32, 41, 45, 61, 64, 99, 100, 113)]


def simplex_elements():
    for sd in (1, 2, 3):
        for fam, degs in SIMPLEX:
            for deg in degs:
                if sd == 1 and fam != "ONPolynomialSet":
                    continue
                if sd == 3 and (deg > 7 or (fam.split("/")[0].split("-")[0] in ("Nedelec", "RaviartThomas") and deg > 3)):
                    continue
                yield fam, sd, deg


def simplex_candidates(part, per_key=20):
    """tabulate_batch / tabulate_batch_mapped and tabulate_cells.  Pruned by what the planner's report (fx_plan_kernel, host
    code) and the dispatch switches can tell apart: for one (element, order, points, cells, map) a policy is only launched
    when the report differs from the ones already taken, and of all candidates with the same report, expansion degree,
    order, cell / map mode, flush parity (whole table and last row tile) and row-tile class at most ``per_key`` are
    launched -- those with the fewest points, which the walk meets first."""
    import numpy as np
    import instance_runner as IR
    from fiat_amd import runtime
    ctx = runtime.Context.get()
    elements = []
    for fam, sd, deg in simplex_elements():
        try:
            el = IR.element(fam, sd, deg)
            dev = IR.polyset(el).device_polyset()
            if not isinstance(dev, runtime.SimplexPolySet):
                raise TypeError("not a simplex polynomial set on the device")
            elements.append((fam, sd, deg, el, dev, IR.mapping_of(el)))
        except Exception as e:          # a family without this degree
            print(f"# no element {fam} sd{sd} k{deg}: {str(e)[:60]}", flush=True)
    taken = {}
    points = POINTS + ([200, 201, 400, 401, 800, 801] if part == "cells" else [])
    for npts in points:
        for fam, sd, deg, el, ps, mapping in elements:
            for order in (0, 1, 2):
                shape1 = ps.out_shape(order, 1, npts)
                if 8 * NREQ * int(np.prod(shape1[1:])) > MAX_BYTES:
                    continue
                rows, ntab, n = ps.ndof * ps.vdim, shape1[1], ps.n
                last = rows - 16 * ((rows + 15) // 16 - 1)
                parity = ((rows * npts) % 2, (last * npts) % 2, (ntab * rows * npts) % 2)
                base = {"family": fam, "sd": sd, "degree": deg, "order": order, "npts": npts, "nreq": NREQ}
                if part == "simplex":
                    for entry, cells in (("tabulate_batch", False), ("tabulate_batch", True), ("tabulate_batch_mapped", True)):
                        if entry == "tabulate_batch_mapped" and mapping not in ("covariant piola", "contravariant piola"):
                            continue
                        seen = set()
                        for pol in POLICY_SETS:
                            ctx.set_policy(*pol)
                            name = ps.kernel_name(order, NREQ, npts, has_verts=cells, instance=True,
                                                  mapping=mapping if entry == "tabulate_batch_mapped" else None)
                            if name in seen:
                                continue
                            seen.add(name)
                            few_tiles = (ntab * rows + 15) // 16 <= 4
                            key = (name, sd, n, order, cells, entry, parity, few_tiles, ps.vdim > 1)
                            if "<" not in name:          # families without an instance form in the report: rows and column tiles too
                                key += (rows, (ntab * npts + 15) // 16, fam == "ONPolynomialSet")
                            if taken.get(key, 0) >= per_key:
                                continue
                            taken[key] = taken.get(key, 0) + 1
                            yield dict(base, entry=entry, cells=cells, policy=list(pol))
                        ctx.set_policy()
                else:
                    if sd == 1 and mapping != "affine":
                        continue
                    table = rows * npts
                    units = table if table % 2 else table // 2
                    for pol in [(), ("no_small",), ("no_shared_wave",), ("no_shared_wave", "no_small"), ("no_shared_reg",),
                                ("no_shared_reg", "no_small"), ("no_shared_reg", "no_shared_wave"),
                                ("no_shared_reg", "no_shared_wave", "no_small")]:
                        # (launch_shared: units per thread of the register-resident kernel, the flat kernel's size classes, the
                        # wave kernel's slots, the lane-local kernel's byte limit)
                        key = (sd, order, mapping != "affine", ps.vdim, table % 2, min(4, (units + 255) // 256), ntab * table <= 12,
                               ntab * table <= 32, ((1 + sd) * table // 2 + 63) // 64 <= 32, 8 * ntab * table <= (3072 if sd == 2 else 2048),
                               n if 8 * ntab * table <= 3072 else -1, pol)
                        if taken.get(key, 0) >= per_key:
                            continue
                        taken[key] = taken.get(key, 0) + 1
                        yield dict(base, entry="tabulate_cells", cells=True, policy=list(pol))


def high_order_candidates():
    """Differentiation-matrix orders 3-6 at the shapes of the recorded reference tables (tests/golden): an order-0 launch of
    the stacked element and, with cells, the table-mixing passes."""
    import instance_runner as IR
    for fixture, (_, names) in IR.GOLDEN_HIGH.items():
        for name in names:
            for order in ((3, 4) if fixture == "round3" else (5, 6)):
                for cells in ((True,) if fixture == "round3" else (False, True)):
                    yield {"entry": "golden_high_order", "fixture": fixture, "name": name, "order": order, "cells": cells, "policy": []}


def other_candidates():
    import edge_reference as R
    import instance_runner as IR
    for fam in IR.MACRO:
        _, sd, deg, _ = IR.MACRO[fam]
        for order in (0, 1, 2):
            for npts in (3, 7, 16, 23, 64, 65, 130):
                for cells in (False, True):
                    for pol in ((), ("no_macro_small",)):
                        yield {"entry": "macro", "family": fam, "sd": sd, "degree": deg, "order": order, "npts": npts, "nreq": NREQ,
                               "cells": cells, "policy": list(pol)}
    for nf in (1, 2, 3):
        for nn in [1, 2, 3, 4, 5, 6, (2, 3, 4)[:nf]]:
            if isinstance(nn, tuple) and nf == 1:
                continue
            for order in (0, 1, 2):
                for pol in ((), ("no_small",)):
                    for npts in (1, 8, 9, 27, 64, 65):
                        yield {"entry": "tensor", "nf": nf, "nn": list(nn) if isinstance(nn, tuple) else nn, "order": order, "npts": npts,
                               "nreq": NREQ, "policy": list(pol)}
                    for q in (1, 2, 3, 4, 8, 9):
                        if q ** nf > 729:
                            continue
                        yield {"entry": "tensor_grid", "nf": nf, "nn": list(nn) if isinstance(nn, tuple) else nn, "order": order, "q": q,
                               "npts": q ** nf, "nreq": NREQ, "policy": list(pol)}
    for nn in (1, 2, 5, 16, 17, 40):
        for order in (0, 1, 2, 3):
            for nreq, npts in ((NREQ, 9), (3, 300)):
                yield {"entry": "line", "nn": nn, "order": order, "npts": npts, "nreq": nreq, "policy": []}
    for fam, degs in (("Lagrange", (1, 2, 3, 4)), ("DiscontinuousLagrange", (0, 1, 2, 3)), ("RaviartThomas", (1, 2, 3)), ("Nedelec", (1, 2, 3)),
                      ("BrezziDouglasMarini", (1, 2))):
        for deg in degs:
            for nn in (1, 2, 3, 4, 5):
                for order in (0, 1, 2):
                    for npts in (1, 7, 8, 16, 33):
                        yield {"entry": "prism", "family": fam, "degree": deg, "nn": nn, "order": order, "npts": npts, "nreq": NREQ,
                               "policy": []}
    for sd in (1, 2, 3):
        for n in list(range(0, 9)) + [12, 16]:
            for order in (0, 1, 2, 3, 4):
                for mode in ("own", "cells", "shared"):
                    for npts in (7, 33, 129):
                        if 8 * NREQ * math.comb(sd + order, sd) * math.comb(n + sd, sd) * npts > MAX_BYTES:
                            continue
                        yield {"entry": "bernstein", "sd": sd, "degree": n, "order": order, "npts": npts, "nreq": NREQ, "mode": mode,
                               "policy": []}
    for kind in (0, 1):
        for sd, ks in ((2, (1, 2, 3, 4)), (3, (1, 2, 3))):
            for K in ks:
                for single in (False, True):
                    name = R.hdc_name(kind, sd, K, single)
                    for order in (0, 1, 2):
                        for npts in (9, 33):
                            yield {"entry": "hdivcurl", "name": name, "order": order, "npts": npts, "nreq": NREQ, "policy": []}
                        for q in (3, 4):
                            yield {"entry": "hdivcurl_grid", "name": name, "order": order, "q": q, "npts": q ** sd, "nreq": NREQ,
                                   "policy": []}
    for ntables, rows, npts in ((37, 10, 23), (5, 120, 129), (1, 1, 1)):
        yield {"entry": "classify_tables", "ntables": ntables, "rows": rows, "npts": npts, "policy": []}
        yield {"entry": "tables_point_major", "ntables": ntables, "rows": rows, "npts": npts, "policy": []}
        for vdim in (1, 3):
            yield {"entry": "tables_squared_norm", "ntables": ntables, "rows": rows, "vdim": vdim, "npts": npts, "policy": []}
    for din, dout in ((1, 2), (2, 3), (1, 3), (2, 2)):
        yield {"entry": "map_points", "din": din, "dout": dout, "nreq": NREQ, "npts": 23, "policy": []}
    for sdA, sdB, rowsA, rowsB, vA, vB, npts, order in ((2, 1, 6, 3, 0, 0, 23, 1), (2, 1, 8, 2, 2, 0, 7, 2), (1, 1, 3, 3, 0, 0, 9, 2),
                                                        (2, 1, 45, 6, 0, 0, 200, 2), (3, 0, 20, 1, 0, 0, 23, 1), (2, 1, 21, 5, 2, 0, 129, 2)):
        yield {"entry": "table_outer", "sdA": sdA, "sdB": sdB, "rowsA": rowsA, "rowsB": rowsB, "vdimA": vA, "vdimB": vB, "npts": npts,
               "order": order, "nreq": NREQ, "policy": []}
    for vs, vd in ((1, 2), (2, 3), (1, 3), (3, 3)):
        yield {"entry": "table_place", "nreq": NREQ, "ntab": 3, "rows": 4, "vdim_src": vs, "vdim_dst": vd, "npts": 9, "rows_dst": 12,
               "row_offset": 4, "policy": []}
    yield {"entry": "riesz_assemble", "nrows": 20, "nq": 35, "nexp": 20, "policy": []}
    yield {"entry": "vandermonde_solve", "nsys": 3, "ndof": 20, "m": 20, "policy": []}
    yield {"entry": "vandermonde_solve", "nsys": 2, "ndof": 100, "m": 100, "policy": []}
    for sd in (1, 2, 3):
        for cells in (False, True):
            yield {"entry": "collapsed_quadrature", "sd": sd, "m": 5, "cells": cells, "policy": []}
    for order in (0, 1, 2):
        yield {"entry": "jacobi", "a": 1.0, "b": 0.5, "n": 9, "order": order, "npts": 101, "policy": []}


def names_of(events):
    return [(e.time_range.start, e.name) for e in events
            if e.device_type.name == "CUDA" and "Memcpy" not in e.name and "Memset" not in e.name]


def walk(part, cands, out_dir, batch=150):
    import torch
    from torch.profiler import ProfilerActivity, profile
    import instance_runner as IR
    from fiat_amd import runtime
    ctx = runtime.Context.get()
    marker = torch.zeros(64, dtype=torch.float32, device="cuda")
    path = os.path.join(out_dir, f"walk_{part}.jsonl")
    log = open(path, "a")
    t0, done = time.time(), 0
    while True:
        group = []
        for c in cands:
            c["id"] = M.case_id(c)
            group.append(c)
            if len(group) == batch:
                break
        if not group:
            break
        with open(os.path.join(out_dir, f"current_{part}.json"), "w") as f:       # what was running, should the walk end early
            json.dump(group, f)
        runs = []
        for c in group:
            ctx.set_policy(*c["policy"])
            try:
                p = IR.prepare(c)
                p.run()                                       # unrecorded: lazy set-up of the element happens here
                runs.append((c, p))
            except Exception as e:                            # a shape the entry refuses (FX_ENOTIMPL ...): not a candidate
                log.write(json.dumps({"case": c, "error": str(e)[:120]}) + "\n")
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for c, p in runs:
                marker.fill_(1.0)
                ctx.set_policy(*c["policy"])
                p.run()
            marker.fill_(1.0)
            torch.cuda.synchronize()
        ctx.set_policy()
        ev = sorted(names_of(prof.events()))
        chunks, cur = [], None
        for _, name in ev:
            if "FillFunctor" in name:
                cur = []
                chunks.append(cur)
            elif cur is not None:
                cur.append(name)
        if len(chunks) != len(runs) + 1:
            print(f"# batch of {len(runs)}: {len(chunks)} markers seen, recording one by one", flush=True)
            chunks = []
            for c, p in runs:
                ctx.set_policy(*c["policy"])
                with profile(activities=[ProfilerActivity.CUDA]) as prof:
                    p.run()
                    torch.cuda.synchronize()
                chunks.append([n for _, n in sorted(names_of(prof.events()))])
            ctx.set_policy()
        for (c, p), raw in zip(runs, chunks):
            norm = M.normalise_all(raw)
            cost = int(__import__("numpy").prod(p.shape)) if p.shape else 0
            log.write(json.dumps({"case": c, "kernels": sorted({n for n in norm if n.startswith(M.NAMESPACE)}), "cost": cost,
                                  "raw": sorted(set(raw))[:3] if done == 0 else None}) + "\n")
        log.flush()
        del runs
        done += len(group)
        print(f"# {part}: {done} candidates, {time.time() - t0:.0f} s", flush=True)
    log.close()


def select(out_dir, write):
    import codeobject_report
    ks, _ = codeobject_report.kernels(all_units=True)
    compiled = sorted(set(M.normalise_all([k["name"] for k in ks])))
    best = {}
    nrec = 0
    for fn in sorted(os.listdir(out_dir)):
        if not (fn.startswith("walk_") and fn.endswith(".jsonl")):
            continue
        for line in open(os.path.join(out_dir, fn)):
            rec = json.loads(line)
            if "kernels" not in rec:
                continue
            nrec += 1
            # cheapest shape; among equals the default policy, then fewer kernels in the call
            key = (rec["cost"], len(rec["case"]["policy"]), len(rec["kernels"]))
            for k in rec["kernels"]:
                if k not in best or key < best[k][0]:
                    best[k] = (key, rec)
    chosen = {}
    for k in compiled:
        if k in best:
            rec = best[k][1]
            chosen[rec["case"]["id"]] = dict(rec["case"], kernels=rec["kernels"])
    reached = {k for c in chosen.values() for k in c["kernels"]}
    missing = [k for k in compiled if k not in reached]
    stray = sorted(k for k in best if k not in compiled)
    print(f"{nrec} recorded launches; {len(compiled)} kernels compiled, {len(compiled) - len(missing)} reached by {len(chosen)} cases")
    for k in missing:
        print("UNREACHED", k)
    for k in stray:
        print("NOT IN THE CODE OBJECT", k)
    if write:
        path = os.path.join(ROOT, "tests", "instance_manifest.py")
        src = open(path).read()
        head, rest = src.split("# --- generated by tools/instance_search.py: begin ---\n")
        _, tail = rest.split("# --- generated by tools/instance_search.py: end ---\n")
        lines = ["CASES = ["]
        for cid in sorted(chosen):
            c = chosen[cid]
            kern = c.pop("kernels")
            lines.append("    " + repr(c)[:-1] + ",")
            lines.append("     'kernels': " + repr(kern) + "},")
        lines.append("]")
        with open(path, "w") as f:
            f.write(head + "# --- generated by tools/instance_search.py: begin ---\n" + "\n".join(lines) + "\n" +
                    "# --- generated by tools/instance_search.py: end ---\n" + tail)
        print(f"wrote {len(chosen)} cases to {path}")
    return missing


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--walk")
    ap.add_argument("--select")
    ap.add_argument("--part", default="simplex,cells,high,other")
    ap.add_argument("--write", action="store_true")
    a = ap.parse_args()
    if a.walk:
        os.makedirs(a.walk, exist_ok=True)
        for part in a.part.split(","):
            gen = {"simplex": lambda: simplex_candidates("simplex"), "cells": lambda: simplex_candidates("cells"),
                   "high": high_order_candidates, "other": other_candidates}[part]()
            walk(part, gen, a.walk)
    if a.select:
        select(a.select, a.write)
