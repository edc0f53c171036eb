#!/usr/bin/env python3
"""Throughput of the closed-form DPC kernel (fiat_amd/csrc/dpc.hpp): HIP-event timing after warm-up, one JSON line per shape
with the algorithmic bytes (tables + points) against 8 TB/s.  Beside each shape, in the same process and interleaved round by
round: ``torch.fill_`` of the same bytes (the box's write rate, as tools/kernel_ab.py) and the general route of the same
element (``route="general"``: the contraction of the nodal coefficients on the simplex kernels).  Kernel times come from a
separate run under ``rocprofv3 --kernel-trace --stats`` (``--only-dpc`` keeps the other kernels out of it).  ``fp64_fraction``
is the kernel's own arithmetic (``flops``: the multiplications and additions of the recurrences and of dpc_dof, counted from
the dof table; an FMA counts two) against the 78.6 TFLOP/s vector fp64 peak.  Measurement tooling.

    python tools/bench_dpc.py [--steps 20] [--warmup 3] [--rounds 3] [--only-dpc]"""
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
from fiat_amd import runtime  # noqa: E402
from fiat_amd.reference_element import ufc_hypercube  # noqa: E402

HBM = 8.0e12
FP64 = 78.6e12

SHAPES = [  # tag, sd, degree, order, points per direction, nreq
    ("DPC_2 quadrilateral, order 1, 3x3", 2, 2, 1, 3, 1_000_000),
    ("DPC_3 hexahedron, order 1, 27", 3, 3, 1, 3, 100_000),
    ("DPC_6 hexahedron, order 2, 64", 3, 6, 2, 4, 8_000),
]


def flops_per_point(sd, k, order):
    """Multiplications and additions per point of dpc_kernel<sd, k, order> (an FMA is two)."""
    n = (sd + 1) * (sd * 2 + k * (3 + (4 if order >= 1 else 0) + (4 if order >= 2 else 0)))      # lambda, then the recurrences
    for alpha in runtime.dpc_descriptor(sd, k):
        pos = [int(a) for a in alpha if a >= 1]
        s = len(pos)
        n += s - 1                                                   # the value
        if order >= 1:
            n += s * ((s - 1) + 2 * sd)                              # D1 products, contraction with G
        if order >= 2:
            pairs = sum(1 for a in pos if a >= 2) + s * (s - 1) // 2
            n += pairs * max(s - 1, 0) + (sum(1 for a in pos if a >= 2) + s * (s - 1)) * 2 * sd   # D2 products, H
            n += (sd * (sd + 1) // 2) * 2 * s                        # the second-order tables
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3, help="interleaved rounds; the best of each is reported")
    ap.add_argument("--only-dpc", action="store_true")
    args = ap.parse_args()
    rng = np.random.default_rng(17)
    for tag, sd, k, order, q, nreq in SHAPES:
        el = fiat_amd.DPC(ufc_hypercube(sd), k)
        g = np.polynomial.legendre.leggauss(q)[0] * 0.5 + 0.5
        coords = np.broadcast_to(g, (nreq, sd, q)) + rng.uniform(-0.01, 0.01, size=(nreq, sd, 1))
        idx = np.stack(np.meshgrid(*[np.arange(q)] * sd, indexing="ij"), -1).reshape(-1, sd)
        pts = torch.as_tensor(np.ascontiguousarray(np.stack([coords[:, d, idx[:, d]] for d in range(sd)], -1))).cuda()
        npts = q ** sd
        out = el.tabulate_batch(order, pts)
        nbytes = out.numel() * 8 + pts.numel() * 8
        runs = {"dpc": lambda: el.tabulate_batch(order, pts, out=out)}
        if not args.only_dpc:
            flat = torch.empty(nbytes // 8, dtype=torch.float64, device=out.device)
            runs["fill"] = lambda: flat.fill_(1.0)
            gout = el.tabulate_batch(order, pts, route="general")
            agree = float((gout - out).abs().max() / max(1.0, float(out.abs().max())))
            runs["general"] = lambda: el.tabulate_batch(order, pts, out=gout, route="general")
        best = {name: float("inf") for name in runs}
        for _ in range(args.rounds):
            for name, fn in runs.items():
                best[name] = min(best[name], timed(fn, args.steps, args.warmup))
        ms = best["dpc"]
        flops = flops_per_point(sd, k, order) * nreq * npts
        rec = {"shape": tag, "kernel": el.kernel(order, npts), "ndof": el.space_dimension(), "nreq": nreq, "npts": npts,
               "ms": round(ms, 4), "tabulations_per_s": round(nreq / (ms * 1e-3), 1), "bytes": nbytes,
               "hbm_fraction": round(nbytes / (ms * 1e-3) / HBM, 3), "flops": flops,
               "fp64_fraction": round(flops / (ms * 1e-3) / FP64, 3)}
        if not args.only_dpc:
            rec.update({"fill_ms": round(best["fill"], 4), "fill_hbm_fraction": round(nbytes / (best["fill"] * 1e-3) / HBM, 3),
                        "general_kernel": el.device_polyset().kernel_name(order, nreq, npts),
                        "general_ms": round(best["general"], 4),
                        "general_hbm_fraction": round(nbytes / (best["general"] * 1e-3) / HBM, 3),
                        "routes_differ_by": agree})
        print(json.dumps(rec), flush=True)
        del out, pts, runs


if __name__ == "__main__":
    main()
