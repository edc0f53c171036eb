#!/usr/bin/env python3
"""Throughput of the Serendipity kernels (fiat_amd/csrc/serendipity.hpp): HIP-event timing after warm-up, one JSON line per
shape with the algorithmic bytes (tables + points) against 8 TB/s.  Beside each shape, in the same process and interleaved
round by round: ``torch.fill_`` of the same bytes (the box's write rate, as tools/kernel_ab.py) and the fused Q_k tensor
kernel at the nearest table size.  Kernel times come from a separate run under ``rocprofv3 --kernel-trace --stats``
(``--only-serendipity`` keeps the other kernels out of it).  Measurement tooling.

    python tools/bench_serendipity.py [--steps 20] [--warmup 3] [--rounds 3] [--only-serendipity]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import fiat_amd  # noqa: E402
from fiat_amd.reference_element import UFCInterval, ufc_hypercube  # noqa: E402

HBM = 8.0e12

SHAPES = [  # tag, sd, degree, order, points per direction, nreq, degree of the Q_k beside it (nearest dof count)
    ("S_2 quadrilateral, order 1, 3x3", 2, 2, 1, 3, 1_000_000, 2),
    ("S_3 hexahedron, order 1, 27", 3, 3, 1, 3, 100_000, 2),
    ("S_2 hexahedron, order 2, 8", 3, 2, 2, 2, 200_000, 2),
    ("S_6 hexahedron, order 2, 64", 3, 6, 2, 4, 8_000, 4),
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


def q_element(sd, k):
    L = fiat_amd.Lagrange(UFCInterval(), k)
    el = fiat_amd.TensorProductElement(L, L)
    return fiat_amd.TensorProductElement(el, L) if sd == 3 else el


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3, help="interleaved rounds; the best of each is reported")
    ap.add_argument("--only-serendipity", action="store_true")
    args = ap.parse_args()
    rng = np.random.default_rng(17)
    for tag, sd, k, order, q, nreq, qk in SHAPES:
        el = fiat_amd.Serendipity(ufc_hypercube(sd), k)
        g = np.polynomial.legendre.leggauss(q)[0] * 0.5 + 0.5
        coords = np.broadcast_to(g, (nreq, sd, q)) + rng.uniform(-0.01, 0.01, size=(nreq, sd, 1))
        idx = np.stack(np.meshgrid(*[np.arange(q)] * sd, indexing="ij"), -1).reshape(-1, sd)
        pts = torch.as_tensor(np.ascontiguousarray(np.stack([coords[:, d, idx[:, d]] for d in range(sd)], -1))).cuda()
        npts = q ** sd
        out = el.tabulate_batch(order, pts)
        nbytes = out.numel() * 8 + pts.numel() * 8
        runs = {"serendipity": lambda: el.tabulate_batch(order, pts, out=out)}
        qbytes = None
        if not args.only_serendipity:
            flat = torch.empty(nbytes // 8, dtype=torch.float64, device=out.device)
            runs["fill"] = lambda: flat.fill_(1.0)
            Q = q_element(sd, qk)
            qout = Q.tabulate_batch(order, pts)
            qbytes = qout.numel() * 8 + pts.numel() * 8
            runs["q"] = lambda: Q.tabulate_batch(order, pts, out=qout)
        best = {name: float("inf") for name in runs}
        for _ in range(args.rounds):
            for name, fn in runs.items():
                best[name] = min(best[name], timed(fn, args.steps, args.warmup))
        ms = best["serendipity"]
        rec = {"shape": tag, "kernel": el.kernel(order, npts), "nreq": nreq, "npts": npts, "ms": round(ms, 4),
               "tabulations_per_s": round(nreq / (ms * 1e-3), 1), "bytes": nbytes, "hbm_fraction": round(nbytes / (ms * 1e-3) / HBM, 3)}
        if not args.only_serendipity:
            rec.update({"fill_ms": round(best["fill"], 4), "fill_hbm_fraction": round(nbytes / (best["fill"] * 1e-3) / HBM, 3),
                        "q_degree": qk, "q_ms": round(best["q"], 4), "q_bytes": qbytes,
                        "q_hbm_fraction": round(qbytes / (best["q"] * 1e-3) / HBM, 3)})
        print(json.dumps(rec), flush=True)
        del out, pts, runs


if __name__ == "__main__":
    main()
