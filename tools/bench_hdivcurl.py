#!/usr/bin/env python3
"""Throughput of the H(div) / H(curl) kernels (fiat_amd/csrc/hdivcurl.hpp): HIP-event timing after warm-up, one JSON line
per shape with the algorithmic bytes (tables + points) against 8 TB/s.  ``--compare-general`` also times the general route
(every leaf tabulated by its own kernels, then placed) on the same shape.  Measurement tooling.

    python tools/bench_hdivcurl.py [--steps 20] [--warmup 3] [--compare-general]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import fiat_amd  # noqa: E402
from fiat_amd import hdivcurl  # noqa: E402
from fiat_amd.reference_element import UFCInterval  # noqa: E402

HBM = 8.0e12


def family(name, k):
    I, T = UFCInterval(), fiat_amd.TensorProductElement
    CG, DG = (lambda n: fiat_amd.Lagrange(I, n)), (lambda n: fiat_amd.DiscontinuousLagrange(I, n))
    E = fiat_amd.EnrichedElement
    if name == "RTCF":
        return E(fiat_amd.Hdiv(T(CG(k), DG(k - 1))), fiat_amd.Hdiv(T(DG(k - 1), CG(k))))
    if name == "RTCE":
        return E(fiat_amd.Hcurl(T(CG(k), DG(k - 1))), fiat_amd.Hcurl(T(DG(k - 1), CG(k))))
    if name == "NCF":
        return E(fiat_amd.Hdiv(T(family("RTCF", k), DG(k - 1))), fiat_amd.Hdiv(T(T(DG(k - 1), DG(k - 1)), CG(k))))
    if name == "NCE":
        return E(fiat_amd.Hcurl(T(family("RTCE", k), CG(k))), fiat_amd.Hcurl(T(T(CG(k), CG(k)), DG(k - 1))))
    tri = fiat_amd.ufc_simplex(2)     # prism H(div)
    return E(fiat_amd.Hdiv(T(fiat_amd.RaviartThomas(tri, k), DG(k - 1))), fiat_amd.Hdiv(T(fiat_amd.DiscontinuousLagrange(tri, k - 1), CG(k))))


SHAPES = [  # tag, family, k, order, q (Gauss points per direction; prism: 6 points), nreq, grid
    ("S1 RTCF_2 quad, order 1, 3x3", "RTCF", 2, 1, 3, 400_000, False),
    ("S2 RTCE_3 quad, order 1, 4x4", "RTCE", 3, 1, 4, 100_000, False),
    ("S3 NCF_2 hex, order 1, 27", "NCF", 2, 1, 3, 40_000, False),
    ("S3 NCF_2 hex, order 1, 27, grid", "NCF", 2, 1, 3, 40_000, True),
    ("S4 NCE_1 hex, order 0, 8", "NCE", 1, 0, 2, 1_000_000, False),
    ("S5 prism H(div) k=1, order 1, 6", "PRISM", 1, 1, 6, 500_000, False),
]


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
    ap.add_argument("--compare-general", action="store_true")
    args = ap.parse_args()
    rng = np.random.default_rng(17)
    for tag, fam, k, order, q, nreq, grid in SHAPES:
        el = family(fam, k)
        sd = el.get_reference_element().get_spatial_dimension()
        if fam == "PRISM":
            e = rng.exponential(size=(nreq, q, 3))
            pts = np.concatenate([(e / e.sum(-1, keepdims=True))[..., 1:], rng.uniform(size=(nreq, q, 1))], -1)
            npts = q
        else:
            g = np.polynomial.legendre.leggauss(q)[0] * 0.5 + 0.5
            coords = np.broadcast_to(g, (nreq, sd, q)) + rng.uniform(-0.01, 0.01, size=(nreq, sd, 1))
            idx = np.stack(np.meshgrid(*[np.arange(q)] * sd, indexing="ij"), -1).reshape(-1, sd)
            pts = np.stack([coords[:, d, idx[:, d]] for d in range(sd)], -1)
            npts = q ** sd
        dev_pts = torch.as_tensor(np.ascontiguousarray(coords if grid else pts)).cuda()
        out = el.tabulate_batch(order, dev_pts, grid=grid)
        fn = lambda: el.tabulate_batch(order, dev_pts, out=out, grid=grid)  # noqa: E731
        ms = timed(fn, args.steps, args.warmup)
        nbytes = out.numel() * 8 + dev_pts.numel() * 8
        rec = {"shape": tag, "route": "general" if fam == "PRISM" else "fused", "nreq": nreq, "npts": npts, "ms": round(ms, 4),
               "tabulations_per_s": round(nreq / (ms * 1e-3), 1), "bytes": nbytes,
               "hbm_fraction": round(nbytes / (ms * 1e-3) / HBM, 3)}
        if args.compare_general and fam != "PRISM" and not grid:
            flat = dev_pts
            rec["general_ms"] = round(timed(lambda: hdivcurl.tabulate_general(el, order, flat, out=out), args.steps, args.warmup), 4)
        print(json.dumps(rec), flush=True)
        del out, dev_pts


if __name__ == "__main__":
    main()
