#!/usr/bin/env python3
"""Throughput of the direct IntegratedLegendre kernel (fiat_amd/csrc/hierarchical.hpp): HIP-event timing after warm-up, one
JSON line per shape with the algorithmic bytes (tables + points) against 8 TB/s.  Beside each shape, in the same process and
interleaved round by round: ``torch.fill_`` of the same bytes (the box's write rate, as tools/kernel_ab.py) and the general
route of the same element (``route="general"``: the contraction of the nodal coefficients on the simplex kernels).  Kernel
times come from a separate run under ``rocprofv3 --kernel-trace --stats`` (``--only-hier`` keeps the other kernels out of it;
take no counters in that run).  Every row of the table is written exactly once, so the bytes hold no read-modify-write
traffic.  Measurement tooling.

    python tools/bench_hierarchical.py [--steps 20] [--warmup 3] [--rounds 3] [--only-hier]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import fiat_amd  # noqa: E402
from bench_hdivcurl import timed  # noqa: E402

HBM = 8.0e12

SHAPES = [  # tag, sd, degree, order, points, nreq: about 1 GB of tables each
    ("IntegratedLegendre_3 tetrahedron, order 1, 23 points", 3, 3, 1, 23, 65_000),
    ("IntegratedLegendre_6 tetrahedron, order 2, 23 points", 3, 6, 2, 23, 6_500),
    ("IntegratedLegendre_4 triangle, order 1, 6 points", 2, 4, 1, 6, 450_000),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3, help="interleaved rounds; the best of each is reported")
    ap.add_argument("--only-hier", action="store_true")
    args = ap.parse_args()
    rng = np.random.default_rng(17)
    for tag, sd, k, order, npts, nreq in SHAPES:
        el = fiat_amd.IntegratedLegendre(fiat_amd.ufc_simplex(sd), k)
        e = rng.exponential(size=(nreq, npts, sd + 1))
        pts = torch.as_tensor(np.ascontiguousarray((e / e.sum(-1, keepdims=True))[..., 1:])).cuda()
        out = el.tabulate_batch(order, pts)
        nbytes = out.numel() * 8 + pts.numel() * 8
        runs = {"hier": lambda: el.tabulate_batch(order, pts, out=out)}
        if not args.only_hier:
            flat = torch.empty(nbytes // 8, dtype=torch.float64, device=out.device)
            runs["fill"] = lambda: flat.fill_(1.0)
            gout = el.tabulate_batch(order, pts, route="general")
            agree = float((gout - out).abs().max() / max(1.0, float(out.abs().max())))
            runs["general"] = lambda: el.tabulate_batch(order, pts, out=gout, route="general")
        best = {name: float("inf") for name in runs}
        for _ in range(args.rounds):
            for name, fn in runs.items():
                best[name] = min(best[name], timed(fn, args.steps, args.warmup))
        ms = best["hier"]
        rec = {"shape": tag, "kernel": el.kernel(order, npts), "ndof": el.space_dimension(), "nreq": nreq, "npts": npts,
               "ms": round(ms, 4), "tabulations_per_s": round(nreq / (ms * 1e-3), 1), "bytes": nbytes,
               "hbm_fraction": round(nbytes / (ms * 1e-3) / HBM, 3)}
        if not args.only_hier:
            rec.update({"fill_ms": round(best["fill"], 4), "fill_hbm_fraction": round(nbytes / (best["fill"] * 1e-3) / HBM, 3),
                        "general_kernel": el.device_polyset().kernel_name(order, nreq, npts),
                        "general_ms": round(best["general"], 4),
                        "general_hbm_fraction": round(nbytes / (best["general"] * 1e-3) / HBM, 3),
                        "routes_differ_by": agree})
        print(json.dumps(rec), flush=True)
        del out, pts, runs


if __name__ == "__main__":
    main()
