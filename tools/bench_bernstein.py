#!/usr/bin/env python3
"""Throughput of the Bernstein kernels (fiat_amd/csrc/bernstein.hpp): HIP-event timing after warm-up, one JSON line per
shape with the algorithmic bytes (points + cells + tables) against 8 TB/s, the algorithmic fp64 flops against 78.6 TF
and the bound that binds.  ``--compare-contraction`` also times the same shape through the Dubiner-coefficient route
(Bernstein as coefficients of the orthonormal expansion set, the existing contraction kernels).  Measurement tooling.

    python tools/bench_bernstein.py [--steps 20] [--warmup 3] [--compare-contraction]"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import fiat_amd  # noqa: E402

HBM, FP64 = 8.0e12, 78.6e12
SHAPES = [  # name, sd, degree, order, nreq, npts, route
    ("P3 tet order 1", 3, 3, 1, 100_000, 23, "own"),
    ("P6 tet order 2", 3, 6, 2, 125_000, 23, "own"),
    ("P3 tet order 1, per-request cells", 3, 3, 1, 100_000, 23, "cells"),
    ("P2 tri order 1, shared points", 2, 2, 1, 100_000, 12, "shared"),
]


def flops_per_point(sd, n, order):
    """fp64 operations of the compile-time instance per point: powers, per dof the value, the first and second
    barycentric derivatives (products of sd+1 powers) and their contraction with G."""
    ndof = math.comb(n + sd, sd)
    f = (sd + 1) * n
    per = sd + 1
    if order >= 1:
        per += (sd + 1) * (sd + 2) + 2 * sd * (sd + 1)
    if order >= 2:
        npair = (sd + 1) * (sd + 2) // 2
        per += npair * (sd + 2) + 2 * npair * 2 * sd + 2 * (sd * (sd + 1) // 2) * (sd + 1)
    return f + ndof * per


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--compare-contraction", action="store_true")
    args = ap.parse_args()
    rng = np.random.default_rng(11)
    for name, sd, n, order, nreq, npts, route in SHAPES:
        cell = fiat_amd.ufc_simplex(sd)
        el = fiat_amd.Bernstein(cell, n)
        ref = np.array(cell.get_vertices(), dtype=float)
        e = rng.exponential(size=(nreq if route != "shared" else 1, npts, sd + 1))
        bary = e / e.sum(-1, keepdims=True)
        ndof, ntab = math.comb(n + sd, sd), math.comb(sd + order, sd)
        out = torch.empty((nreq, ntab, ndof, npts), dtype=torch.float64, device="cuda")
        verts = None
        if route != "own":
            A = np.eye(sd) + 0.1 * rng.standard_normal((nreq, sd, sd))
            verts = torch.as_tensor(np.einsum("vd,red->rve", ref, A) + rng.standard_normal((nreq, 1, sd))).cuda()
        if route == "shared":
            ref_pts = torch.as_tensor(bary[0] @ ref).cuda()
            fn = lambda: el.tabulate_cells(order, ref_pts, verts, out=out)  # noqa: E731
            pts_bytes = npts * sd * 8
        else:
            pts = torch.as_tensor(bary @ ref).cuda()
            if route == "cells":
                pts = torch.einsum("rpv,rvd->rpd", torch.as_tensor(bary).cuda(), verts).contiguous()
            fn = lambda: el.tabulate_batch(order, pts, verts=verts, out=out)  # noqa: E731
            pts_bytes = nreq * npts * sd * 8
        ms = timed(fn, args.steps, args.warmup)
        nbytes = pts_bytes + (0 if verts is None else nreq * (sd + 1) * sd * 8) + out.numel() * 8
        flops = nreq * npts * flops_per_point(sd, n, order)
        fb, ff = nbytes / (ms * 1e-3) / HBM, flops / (ms * 1e-3) / FP64
        rec = {"shape": name, "route": route, "nreq": nreq, "npts": npts, "ms": round(ms, 4),
               "tabulations_per_s": round(nreq / (ms * 1e-3), 1), "bytes": nbytes, "hbm_fraction": round(fb, 3),
               "flops": flops, "fp64_fraction": round(ff, 4), "bound": "hbm" if nbytes / HBM >= flops / FP64 else "fp64"}
        if args.compare_contraction and route == "own":
            on = fiat_amd.ONPolynomialSet(cell, n)
            lat = np.array(fiat_amd.make_lattice(cell.get_vertices(), n, variant="gll"))
            z = (0,) * sd
            C = np.linalg.solve(on.tabulate(lat, 0)[z].T, el.tabulate(0, lat)[z].T).T
            ps = fiat_amd.PolynomialSet(cell, n, n, on.get_expansion_set(), C).device_polyset()
            rec["contraction_ms"] = round(timed(lambda: ps.tabulate_batch(order, pts, out=out), args.steps, args.warmup), 4)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
