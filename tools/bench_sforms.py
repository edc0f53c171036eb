#!/usr/bin/env python3
"""Throughput of the term-table kernel of BDMCE / BDMCF and the trimmed serendipity families (fiat_amd/csrc/sforms.hpp):
HIP-event timing after warm-up, one JSON line per shape with the algorithmic bytes (tables + points) against 8 TB/s.  Beside
each shape, in the same process and interleaved round by round: ``torch.fill_`` of the same bytes (the box's write rate, as
tools/kernel_ab.py) and the project's fused hdivcurl_kernel on the RTCF / NCE element of the nearest dof count.  Kernel
times come from a separate run under ``rocprofv3 --kernel-trace --stats`` (``--only-sforms`` keeps the other kernels out of
it).  Measurement tooling.

    python tools/bench_sforms.py [--steps 20] [--warmup 3] [--rounds 3] [--only-sforms]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import fiat_amd  # noqa: E402
from bench_hdivcurl import family, timed  # noqa: E402
from fiat_amd.reference_element import ufc_hypercube  # noqa: E402

HBM = 8.0e12

SHAPES = [  # tag, class, sd, degree, order, points per direction, nreq, the tensor-product family beside it and its degree
    ("BDMCF_1 quadrilateral, order 1, 3x3", fiat_amd.BrezziDouglasMariniCubeFace, 2, 1, 1, 3, 400_000, "RTCF", 2),
    ("SminusDiv_2 quadrilateral, order 1, 3x3", fiat_amd.TrimmedSerendipityDiv, 2, 2, 1, 3, 400_000, "RTCF", 2),
    ("SminusCurl_2 hexahedron, order 1, 27", fiat_amd.TrimmedSerendipityCurl, 3, 2, 1, 3, 20_000, "NCE", 2),
    ("SminusDiv_3 hexahedron, order 2, 27", fiat_amd.TrimmedSerendipityDiv, 3, 3, 2, 3, 5_000, "NCE", 2),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3, help="interleaved rounds; the best of each is reported")
    ap.add_argument("--only-sforms", action="store_true")
    args = ap.parse_args()
    rng = np.random.default_rng(17)
    for tag, cls, sd, k, order, q, nreq, fam, fk in SHAPES:
        el = cls(ufc_hypercube(sd), k)
        g = np.polynomial.legendre.leggauss(q)[0] * 0.5 + 0.5
        coords = np.broadcast_to(g, (nreq, sd, q)) + rng.uniform(-0.01, 0.01, size=(nreq, sd, 1))
        idx = np.stack(np.meshgrid(*[np.arange(q)] * sd, indexing="ij"), -1).reshape(-1, sd)
        pts = torch.as_tensor(np.ascontiguousarray(np.stack([coords[:, d, idx[:, d]] for d in range(sd)], -1))).cuda()
        npts = q ** sd
        out = el.tabulate_batch(order, pts)
        nbytes = out.numel() * 8 + pts.numel() * 8
        runs = {"sforms": lambda: el.tabulate_batch(order, pts, out=out)}
        if not args.only_sforms:
            flat = torch.empty(nbytes // 8, dtype=torch.float64, device=out.device)
            runs["fill"] = lambda: flat.fill_(1.0)
            H = family(fam, fk)
            hout = H.tabulate_batch(order, pts)
            hbytes = hout.numel() * 8 + pts.numel() * 8
            runs["hdivcurl"] = lambda: H.tabulate_batch(order, pts, out=hout)
        best = {name: float("inf") for name in runs}
        for _ in range(args.rounds):
            for name, fn in runs.items():
                best[name] = min(best[name], timed(fn, args.steps, args.warmup))
        ms = best["sforms"]
        rec = {"shape": tag, "kernel": el.kernel(order, npts), "rows": el.num_rows(), "nreq": nreq, "npts": npts, "ms": round(ms, 4),
               "tabulations_per_s": round(nreq / (ms * 1e-3), 1), "bytes": nbytes, "hbm_fraction": round(nbytes / (ms * 1e-3) / HBM, 3)}
        if not args.only_sforms:
            rec.update({"fill_ms": round(best["fill"], 4), "fill_hbm_fraction": round(nbytes / (best["fill"] * 1e-3) / HBM, 3),
                        "hdivcurl_element": f"{fam}_{fk}", "hdivcurl_rows": H.space_dimension(), "hdivcurl_ms": round(best["hdivcurl"], 4),
                        "hdivcurl_bytes": hbytes, "hdivcurl_hbm_fraction": round(hbytes / (best["hdivcurl"] * 1e-3) / HBM, 3)})
        print(json.dumps(rec), flush=True)
        del out, pts, runs


if __name__ == "__main__":
    main()
