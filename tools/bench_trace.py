#!/usr/bin/env python3
"""Throughput of the fused facet kernel of the H(div) trace element (fiat_amd/csrc/trace.hpp): HIP-event timing after warm-up,
one JSON line per shape with the algorithmic bytes (tables + points + facet numbers) against 8 TB/s.  Beside each shape, in the
same process and interleaved round by round: ``torch.fill_`` of the same bytes (the box's write rate, as tools/kernel_ab.py)
and, in the facet-per-request mode, the general route of the same element (``route="general"``: the facet element's own
kernel, then the placement into a zeroed table; identify mode has no general route).  Kernel times come from a separate run
under ``rocprofv3 --kernel-trace --stats`` (``--only-trace`` keeps the other kernels out of it).  Two of the shapes share a
kernel instance and so one row of the profiler's statistics: ``--by-shape KERNEL_TRACE.csv`` splits that run's kernel trace
into one CSV row per shape (the dispatches of ``trace_kernel`` in launch order, equal counts per shape).  Measurement tooling.

    python tools/bench_trace.py [--steps 20] [--warmup 3] [--rounds 3] [--only-trace]
    python tools/bench_trace.py --by-shape <dir>/<pid>_kernel_trace.csv > profiles/trace_kernel_by_shape.csv"""
import argparse
import csv
import json
import statistics
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

HBM = 8.0e12

SHAPES = [  # tag, spatial dimension, degree, points, nreq, mode: about 1 GB of tables each
    ("HDivTrace_2 tetrahedron, 6 points, facet per request", 3, 2, 6, 870_000, "facets"),
    ("HDivTrace_2 tetrahedron, 6 points, identify", 3, 2, 6, 870_000, "identify"),
    ("HDivTrace_3 triangle, 4 points, facet per request", 2, 3, 4, 2_600_000, "facets"),
]


def by_shape(path):
    """The trace_kernel dispatches of a ``--only-trace`` run under the profiler, in launch order, split evenly over SHAPES."""
    rows = [r for r in csv.DictReader(open(path)) if "trace_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per = len(rows) // len(SHAPES)
    assert per * len(SHAPES) == len(rows), f"{len(rows)} dispatches do not split over {len(SHAPES)} shapes"
    out = csv.writer(sys.stdout, quoting=csv.QUOTE_NONNUMERIC)
    out.writerow(["Shape", "Name", "Calls", "AverageNs", "MedianNs", "MinNs", "MaxNs"])
    for i, shape in enumerate(SHAPES):
        part = rows[i * per:(i + 1) * per]
        names = {r["Kernel_Name"] for r in part}
        assert len(names) == 1, names
        ns = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in part]
        out.writerow([shape[0], names.pop(), per, round(statistics.mean(ns), 1), statistics.median(ns), min(ns), max(ns)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3, help="interleaved rounds; the best of each is reported")
    ap.add_argument("--only-trace", action="store_true")
    ap.add_argument("--by-shape", metavar="KERNEL_TRACE.csv", help="split a profiled run's kernel trace by shape; no GPU needed")
    args = ap.parse_args()
    if args.by_shape:
        return by_shape(args.by_shape)
    import torch

    import fiat_amd
    from bench_hdivcurl import timed
    rng = np.random.default_rng(19)
    for tag, sd, k, npts, nreq, mode in SHAPES:
        el = fiat_amd.HDivTrace(fiat_amd.ufc_simplex(sd), k)
        facets = rng.integers(0, sd + 1, size=nreq).astype(np.int32)
        # points of the facet simplex; identify mode: the same points in cell coordinates, lambda_f exactly 0
        lam = rng.uniform(0.05, 1.0, size=(nreq, npts, sd))
        lam /= lam.sum(-1, keepdims=True)
        if mode == "identify":
            cell = np.insert(lam, 0, 0.0, axis=-1)                      # (nreq, npts, sd + 1), the facet's own coordinate first
            for f in range(1, sd + 1):                                  # move the zero to column f
                sel = facets == f
                cell[sel] = np.concatenate([cell[sel][..., 1:f + 1], cell[sel][..., :1], cell[sel][..., f + 1:]], axis=-1)
            pts = torch.as_tensor(np.ascontiguousarray(cell[..., 1:])).cuda()
            kw = {}
        else:
            pts = torch.as_tensor(np.ascontiguousarray(lam[..., 1:])).cuda()
            kw = {"facets": torch.as_tensor(facets).cuda()}
        out = el.tabulate_batch(0, pts, **kw)
        assert bool(torch.isfinite(out).all())
        nbytes = out.numel() * 8 + pts.numel() * 8 + (nreq * 4 if mode == "facets" else 0)
        runs = {"trace": lambda: el.tabulate_batch(0, pts, out=out, **kw)}
        if not args.only_trace:
            flat = torch.empty(nbytes // 8, dtype=torch.float64, device=out.device)
            runs["fill"] = lambda: flat.fill_(1.0)
            if mode == "facets":
                gout = el.tabulate_batch(0, pts, route="general", **kw)
                agree = float((gout - out).abs().max() / max(1.0, float(out.abs().max())))
                runs["general"] = lambda: el.tabulate_batch(0, pts, out=gout, route="general", **kw)
        best = {name: float("inf") for name in runs}
        for _ in range(args.rounds):
            for name, fn in runs.items():
                best[name] = min(best[name], timed(fn, args.steps, args.warmup))
        ms = best["trace"]
        rec = {"shape": tag, "kernel": el.kernel(npts, mode), "ndof": el.space_dimension(), "nreq": nreq, "npts": npts,
               "ms": round(ms, 4), "tabulations_per_s": round(nreq / (ms * 1e-3), 1), "bytes": nbytes,
               "hbm_fraction": round(nbytes / (ms * 1e-3) / HBM, 3)}
        if not args.only_trace:
            rec.update({"fill_ms": round(best["fill"], 4), "fill_hbm_fraction": round(nbytes / (best["fill"] * 1e-3) / HBM, 3)})
            if mode == "facets":
                rec.update({"general_ms": round(best["general"], 4),
                            "general_hbm_fraction": round(nbytes / (best["general"] * 1e-3) / HBM, 3), "routes_differ_by": agree})
        print(json.dumps(rec), flush=True)
        del out, pts, runs, kw


if __name__ == "__main__":
    main()
