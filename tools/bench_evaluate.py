#!/usr/bin/env python3
"""Throughput of ``evaluate_batch`` (fiat_amd/csrc/evaluate.hpp): HIP-event timing after warm-up (the protocol of DESIGN 6), one
JSON line per shape.  Beside the fused route, in the same process and interleaved round by round: the general route as a whole
(``tabulate_batch`` plus ``torch.einsum``, the composition a user can write today) and a ``torch.fill_`` of the fused route's
output bytes (the box's write rate).  Every line carries both lower bounds of the fused kernel: the bytes it has to move (points +
dofs + vertices + output) against 8 TB/s, and its fp64 FMAs (transform + accumulation of the walk) against the vector fp64 rate
of the chip (1024 SIMDs x 16 lanes x 2.4 GHz = 39.3 TFMA/s), and says which of the two binds.  Measurement tooling.

    python tools/bench_evaluate.py [--steps 20] [--warmup 3] [--rounds 3] [--out profiles/evaluate_bench_lines.jsonl]"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import fiat_amd  # noqa: E402
from bench_hdivcurl import timed  # noqa: E402

HBM = 8.0e12
FMA_RATE = 1024 * 16 * 2.4e9     # vector fp64 FMAs per second: one per lane and cycle, 16 lanes per SIMD

SHAPES = [  # tag, element, order, points, requests, per-request cells, push-forward
    ("P3 tetrahedron, order 1, 23 points, own cell", lambda: fiat_amd.Lagrange(fiat_amd.ufc_simplex(3), 3), 1, 23, 100_000, False, False),
    ("P2 triangle, order 0, 6 points, per-request cells", lambda: fiat_amd.Lagrange(fiat_amd.ufc_simplex(2), 2), 0, 6, 1_000_000, True, False),
    ("Nedelec 2 tetrahedron, order 0, 23 points, per-request cells, covariant Piola",
     lambda: fiat_amd.Nedelec(fiat_amd.ufc_simplex(3), 2), 0, 23, 100_000, True, True),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3, help="interleaved rounds; the best of each is reported")
    ap.add_argument("--out", default=None, help="append the lines to this file too")
    args = ap.parse_args()
    rng = np.random.default_rng(23)
    for tag, make, order, npts, nreq, cells, push in SHAPES:
        el = make()
        sd = el.get_reference_element().get_spatial_dimension()
        vs = tuple(el.value_shape())
        vdim = int(np.prod(vs, dtype=int)) if vs else 1
        ndof, n = el.space_dimension(), el.degree()
        nexp, ntab = math.comb(n + sd, sd), math.comb(sd + order, sd)
        e = rng.exponential(size=(nreq, npts, sd + 1))
        ref_pts = (e / e.sum(-1, keepdims=True))[..., 1:]
        verts = None
        pts = ref_pts
        if cells:
            A = np.eye(sd) + 0.3 * rng.standard_normal((nreq, sd, sd))
            v0 = rng.standard_normal((nreq, 1, sd))
            verts = np.concatenate([v0, v0 + np.swapaxes(A, 1, 2)], axis=1)
            pts = np.einsum("rde,rpe->rpd", A, ref_pts) + v0
            verts = torch.as_tensor(np.ascontiguousarray(verts)).cuda()
        pts = torch.as_tensor(np.ascontiguousarray(pts)).cuda()
        dofs = torch.as_tensor(rng.uniform(-1, 1, size=(nreq, ndof))).cuda()
        kw = dict(verts=verts, pushforward=push)
        out = el.evaluate_batch(order, pts, dofs, route="fused", **kw)
        gout = el.evaluate_batch(order, pts, dofs, route="general", **kw)
        agree = float((gout - out).abs().max() / max(1.0, float(gout.abs().max())))
        flat = torch.empty(out.numel(), dtype=torch.float64, device=out.device)
        runs = {"fused": lambda: el.evaluate_batch(order, pts, dofs, out=out, route="fused", **kw),
                "general": lambda: el.evaluate_batch(order, pts, dofs, out=gout, route="general", **kw),
                "fill": lambda: flat.fill_(1.0)}
        best = {name: float("inf") for name in runs}
        for _ in range(args.rounds):
            for name, fn in runs.items():
                best[name] = min(best[name], timed(fn, args.steps, args.warmup))
        nbytes = 8 * (pts.numel() + dofs.numel() + (verts.numel() if cells else 0) + out.numel())
        table_bytes = 8 * nreq * ntab * ndof * vdim * npts
        fma = nreq * (ndof * vdim * nexp + npts * nexp * ntab * vdim)      # transform + accumulation (the steps come on top)
        bound_bytes_ms, bound_fma_ms = nbytes / HBM * 1e3, fma / FMA_RATE * 1e3
        rec = {"shape": tag, "kernel": el.evaluate_kernel(order, npts, has_verts=cells, pushforward=push), "ndof": ndof,
               "nreq": nreq, "npts": npts, "fused_ms": round(best["fused"], 4), "general_ms": round(best["general"], 4),
               "fused_over_general": round(best["fused"] / best["general"], 3), "fill_ms": round(best["fill"], 4),
               "bytes": nbytes, "table_bytes_not_written": table_bytes, "fma": fma,
               "bound_bytes_ms": round(bound_bytes_ms, 4), "bound_fma_ms": round(bound_fma_ms, 4),
               "binding_bound": "fma" if bound_fma_ms > bound_bytes_ms else "bytes",
               "fused_over_binding_bound": round(best["fused"] / max(bound_bytes_ms, bound_fma_ms), 2),
               "points_per_s": round(nreq * npts / (best["fused"] * 1e-3), 1), "routes_differ_by": agree}
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        del out, gout, flat, pts, dofs, runs


if __name__ == "__main__":
    main()
