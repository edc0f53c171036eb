#!/usr/bin/env python3
"""Cost of tabulating on physical quadrilaterals / hexahedra (fiat_amd/cellmap.py, csrc/cellmap.hpp): HIP-event timing after
warm-up, one JSON line per shape.  Three variants per shape, in the same process and interleaved round by round:

  fused      the fused kernel of 1-D Lagrange products (where it exists), which writes the physical tables directly;
  general    the element's own tabulation followed by the pass in place (fx_cellmap_apply);
  reference  the element's own reference-cell tabulation alone: it writes the same table bytes, so it is the yardstick for
             what the physical-cell version may cost.

Bytes are tables + points + corners; ``*_hbm_fraction`` is those bytes over the window time against 8 TB/s (the general route
moves the tables three times; the figure is still of the algorithmic bytes).  Kernel times come from a separate run under
``rocprofv3 --kernel-trace --stats`` (``--only fused|general|reference`` keeps the other variants out of it).  Measurement
tooling.

    python tools/bench_cellmap.py [--steps 10] [--warmup 2] [--rounds 3] [--scale 1.0] [--only VARIANT]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import fiat_amd  # noqa: E402
from bench_hdivcurl import timed  # noqa: E402
from fiat_amd import cellmap  # noqa: E402

HBM = 8.0e12


def q_element(sd, k):
    I = fiat_amd.ufc_simplex(1)
    el = fiat_amd.TensorProductElement(fiat_amd.Lagrange(I, k), fiat_amd.Lagrange(I, k))
    return el if sd == 2 else fiat_amd.TensorProductElement(el, fiat_amd.Lagrange(I, k))


def rtcf(k):
    import make_golden_hdivcurl
    return make_golden_hdivcurl.build(fiat_amd, f"rtcf{k}d0")


SHAPES = [  # tag, element, sd, points per direction, nreq, grid input, push-forward
    ("Q4 hexahedron (P4^3, BASELINE C5), order 1, 5^3 grid", lambda: q_element(3, 4), 3, 5, 20_000, True, False),
    ("Q2 quadrilateral, order 1, 3x3", lambda: q_element(2, 2), 2, 3, 1_000_000, True, False),
    ("RTCF_2 quadrilateral, order 1, 3x3, contravariant Piola", lambda: rtcf(2), 2, 3, 400_000, False, True),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3, help="interleaved rounds; the best of each is reported")
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies every request count")
    ap.add_argument("--only", choices=["fused", "general", "reference"])
    args = ap.parse_args()
    rng = np.random.default_rng(23)
    for tag, make, sd, q, nreq, grid, push in SHAPES:
        nreq = max(1, int(nreq * args.scale))
        el = make()
        g = np.polynomial.legendre.leggauss(q)[0] * 0.5 + 0.5
        coords = np.broadcast_to(g, (nreq, sd, q)) + rng.uniform(-0.01, 0.01, size=(nreq, sd, 1))
        idx = np.stack(np.meshgrid(*[np.arange(q)] * sd, indexing="ij"), -1).reshape(-1, sd)
        explicit = torch.as_tensor(np.ascontiguousarray(np.stack([coords[:, d, idx[:, d]] for d in range(sd)], -1))).cuda()
        pts = torch.as_tensor(np.ascontiguousarray(coords)).cuda() if grid else explicit
        base = np.array([[(i >> (sd - 1 - d)) & 1 for d in range(sd)] for i in range(2 ** sd)], dtype=float)
        corners = torch.as_tensor(base + rng.uniform(-0.15, 0.15, size=(nreq,) + base.shape)).cuda()
        kw = {"grid": True} if grid else {}
        npts = q ** sd
        fused = cellmap.fused_refusal(el) is None
        out = cellmap.tabulate_on_cells(el, 1, pts, corners, pushforward=push, route="general", **kw)
        nbytes = (out.numel() + pts.numel() + corners.numel()) * 8
        runs = {}
        rec = {"shape": tag, "ndof": el.space_dimension(), "nreq": nreq, "npts": npts, "bytes": nbytes,
               "route": cellmap.kernel(el, 1, q if grid else npts, push, grid)}
        if fused:
            fout = cellmap.tabulate_on_cells(el, 1, pts, corners, route="fused", **kw)
            rec["routes_differ_by"] = float((fout - out).abs().max() / max(1.0, float(out.abs().max())))
            runs["fused"] = lambda: cellmap.tabulate_on_cells(el, 1, pts, corners, out=fout, route="fused", **kw)
        runs["general"] = lambda: cellmap.tabulate_on_cells(el, 1, pts, corners, out=out, pushforward=push, route="general", **kw)
        runs["reference"] = lambda: el.tabulate_batch(1, pts, out=out, **kw)
        if args.only:
            runs = {k: v for k, v in runs.items() if k == args.only}
        best = {name: float("inf") for name in runs}
        for _ in range(args.rounds):
            for name, fn in runs.items():
                best[name] = min(best[name], timed(fn, args.steps, args.warmup))
        for name, ms in best.items():
            rec[f"{name}_ms"] = round(ms, 4)
            rec[f"{name}_hbm_fraction"] = round(nbytes / (ms * 1e-3) / HBM, 3)
        print(json.dumps(rec), flush=True)
        del out, pts, explicit, corners, runs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
