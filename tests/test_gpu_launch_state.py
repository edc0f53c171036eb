"""Launch state of the dynamically scheduled kernels: which work counter (csrc/work_queue.hpp) a launch gets when
launches are pending on several streams, come out of a replayed graph, or queue up deep on one stream
(csrc/counter_handout.hpp).  The kernels trust their counter completely, so two unordered launches on
one counter each leave part of their tables unwritten -- silently: no fault, no error mark.

Every output is filled with NaN before its launch and must afterwards be complete and BIT-EQUAL to a serial launch of the
same request; that serial launch is compared once with the pinned C oracle (1e-12 on values, 1e-10 on derivatives,
relative to max(1, max|ref|) of the table), so every output that passes meets the oracle's tolerance with the same figures.

Shapes.  The P3 tetrahedron of elements.npz at order 1 and 23 points (fxk::tabulate_simplex_pair) and a degree-4 set at
order 0 and 16 points (fxk::tabulate_simplex_stacked).  A workgroup's first WQ_AHEAD = 1 chunk is static (chunk b of
workgroup b), every further chunk comes from the counter: with ``grid`` workgroups, three quarters of the chunks are dynamic
once nchunks >= 4 * grid.  A chunk is 8 units.
  * pair kernel: a unit is two requests, a chunk 16; one 512-thread workgroup fits a CU's LDS, grid = num_cu;
    nreq = 16 * 4 * num_cu + 1 (16 385 on 256 CUs: 1 025 chunks on 256 workgroups).
  * stacked kernel <3,4,3,3>: a unit is a group of three requests, a chunk 24; two 256-thread workgroups a CU,
    grid = 2 * num_cu; nreq = 24 * 4 * 2 * num_cu + 1 (49 153: 2 049 chunks on 512 workgroups).
test_gate_and_control reads both grids from the profiler's records and asserts the inequality."""
import math
import os
import sys

import numpy as np
import pytest

from oracle import fiat_oracle as fo

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edge_reference as er  # noqa: E402  (the profiler's device-side records)

TOL_VAL = 1e-12
TOL_DER = 1e-10
NAN = float("nan")
FILL_MS = 0.08          # one fill_ of the 512 MB gate buffer (HBM at ~6 TB/s); the gates are sized in these


class Shape:
    """One request shape: its device set, the kernel it runs on, the three batch sizes of the tests."""

    def __init__(self, key, ps, n, coeffs, order, npts, oracle_kw, kernel, chunk_requests, grid):
        self.key, self.ps, self.n, self.coeffs, self.order, self.npts = key, ps, n, coeffs, order, npts
        self.oracle_kw, self.kernel, self.chunk_requests, self.grid = oracle_kw, kernel, chunk_requests, grid
        self.dynamic = chunk_requests * 4 * grid + 1       # smallest batch with nchunks >= 4 * grid, plus a ragged unit
        self.sizes = (1, grid * 8 - 1, self.dynamic)
        self.cases = {}

    def nchunks(self, nreq):
        return math.ceil(math.ceil(nreq / (self.chunk_requests // 8)) / 8)


class Case:
    """A batch of one shape: points on the device, the serial launch's tables (checked against the oracle)."""

    def __init__(self, shape, nreq, seed):
        import torch
        from oracle import c_oracle
        self.shape, self.nreq = shape, nreq
        rng = np.random.default_rng(seed)
        e = rng.exponential(size=(nreq, shape.npts, 4))
        pts = (e / e.sum(-1, keepdims=True))[..., 1:].copy()
        self.pts = torch.as_tensor(pts).cuda()
        assert shape.ps.kernel_name(shape.order, nreq, shape.npts) == shape.kernel
        self.ref = shape.ps.tabulate_batch(shape.order, self.pts)
        torch.cuda.synchronize()
        got = self.ref.cpu().numpy()
        want = c_oracle.tabulate_batch(fo.UFC_SIMPLEX[3], shape.n, shape.coeffs, shape.order, pts, **shape.oracle_kw)
        num = np.abs(got - want).max(axis=(2, 3))
        den = np.maximum(1.0, np.abs(want).max(axis=(2, 3)))
        err = (num / den).max(axis=0)
        assert np.isfinite(got).all()
        assert err[0] <= TOL_VAL and (len(err) == 1 or err[1:].max() <= TOL_DER), (shape.key, nreq, err)

    def out(self):
        import torch
        return torch.full(self.ref.shape, NAN, dtype=torch.float64, device="cuda")

    def launch(self, out, stream):
        self.shape.ps.tabulate_batch(self.shape.order, self.pts, out=out, stream=stream)

    def check(self, out, what):
        """Complete, and bit-equal to the serial launch (whose distance to the oracle is within the tolerances)."""
        import torch
        if torch.equal(out.view(torch.int64), self.ref.view(torch.int64)):
            return
        unwritten = int(torch.isnan(out).sum())
        differ = int((out.view(torch.int64) != self.ref.view(torch.int64)).sum())
        raise AssertionError(f"{what}: {unwritten} of {out.numel()} entries never written (NaN left), {differ} differ from the serial launch")


class Lab:
    def __init__(self, golden):
        import torch
        from fiat_amd import runtime
        assert torch.cuda.is_available(), "these tests need the MI355X"
        self.ctx = runtime.Context.get()
        ncu = self.ctx.num_cu
        co3 = golden("elements")["c2_p3tet_q6_coeffs"]
        p3 = runtime.SimplexPolySet(3, 3, variant="bubble", scale=1, coeffs=co3)
        co4 = np.random.default_rng(44).standard_normal((35, 35))
        p4 = runtime.SimplexPolySet(3, 4, coeffs=co4)
        self.shapes = {
            "pair": Shape("pair", p3, 3, co3, 1, 23, dict(scale=1, variant="bubble"), "fxk::tabulate_simplex_pair", 16, ncu),
            "stacked": Shape("stacked", p4, 4, co4, 0, 16, {}, "fxk::tabulate_simplex_stacked", 24, 2 * ncu),
        }
        self.gate_stream = torch.cuda.Stream()
        self.gate_buf = torch.empty(1 << 26, dtype=torch.float64, device="cuda")      # 512 MB
        self.A, self.B, self.F = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
        self._filler_out = None

    def case(self, key, nreq=None):
        shape = self.shapes[key]
        nreq = shape.dynamic if nreq is None else nreq
        if nreq not in shape.cases:
            shape.cases[nreq] = Case(shape, nreq, seed=1000 + nreq % 977)
        return shape.cases[nreq]

    def gate(self, ms):
        """An event on a stream of its own behind ``ms`` milliseconds of fills: streams that wait for it start together."""
        import torch
        ev = torch.cuda.Event()
        with torch.cuda.stream(self.gate_stream):
            for _ in range(int(math.ceil(ms / FILL_MS))):
                self.gate_buf.fill_(0.0)
            ev.record(self.gate_stream)
        return ev

    def fillers(self, count):
        """``count`` dynamic launches of the pair shape on a third stream, into one buffer: they run at once."""
        if count == 0:
            return
        case = self.case("pair")
        if self._filler_out is None:
            self._filler_out = case.out()
        for _ in range(count):
            case.launch(self._filler_out, self.F)


@pytest.fixture(scope="module")
def lab(golden):
    import torch
    lab = Lab(golden)
    yield lab
    torch.cuda.synchronize()
    del lab
    torch.cuda.empty_cache()


def _gated_pair(lab, case, out_a, out_b, between=0, first=None):
    """out_a's launch on stream A and out_b's on stream B behind one gate, ``between`` filler launches planned between
    the two; ``first`` replaces the launch on A (a graph replay).  Returns whether the gate was still closed when both
    were queued -- if not, the two did not start together and the caller has tested nothing."""
    import torch
    with torch.cuda.stream(lab.A):
        out_a.fill_(NAN)
    with torch.cuda.stream(lab.B):
        out_b.fill_(NAN)
    ev = lab.gate(4.0 + 0.2 * between)
    lab.A.wait_event(ev)
    lab.B.wait_event(ev)
    if first is None:
        case.launch(out_a, lab.A)
    else:
        with torch.cuda.stream(lab.A):
            first()
    lab.fillers(between)
    case.launch(out_b, lab.B)
    closed = not ev.query()
    torch.cuda.synchronize()
    return closed


# ---- a. the gate, and a control pair whose counters certainly differ -----------------------------------------------------
@pytest.mark.parametrize("key", ["pair", "stacked"])
def test_gate_and_control(lab, key, tmp_path):
    """Two launches planned back to back, on two streams behind the gate: their device time ranges (profiler records)
    intersect.  Everything else in this file rests on the gate producing concurrency, so no overlap is a FAILURE.  The
    records also give the launch grids: the batch sizes of this file assume them (module docstring)."""
    case = lab.case(key)
    shape = case.shape
    oa, ob = case.out(), case.out()
    _gated_pair(lab, case, oa, ob)                      # the profiler's first use, the streams' first launches
    state = {}
    records = er.launched_records(lambda: state.update(closed=_gated_pair(lab, case, oa, ob)), tmp_path / "trace.json")
    mine = [r for r in records if shape.kernel.split("::")[1] in r["name"]]
    assert len(mine) == 2, [r["name"] for r in records]
    for r in mine:
        assert r["grid"] == shape.grid, (r["grid"], shape.grid)
    assert shape.nchunks(case.nreq) >= 4 * shape.grid, (shape.nchunks(case.nreq), shape.grid)
    assert mine[0]["stream"] != mine[1]["stream"], mine
    overlap = min(r["end"] for r in mine) - max(r["start"] for r in mine)
    print(f"{key}: device ranges {[(r['start'], r['end']) for r in mine]}, overlap {overlap:.1f} us, gate closed at queueing: {state['closed']}")
    assert overlap > 0, f"the gate produced no concurrency: the two launches ran {-overlap:.1f} us apart ({mine})"
    case.check(oa, "control launch on A")
    case.check(ob, "control launch on B")
    lab.ctx.check()


# ---- b. two gated launches with d launches planned between them -----------------------------------------------------------
@pytest.mark.parametrize("between", [0, 1, 63, 64, 65, 127, 128])
def test_colliding_plans(lab, between):
    """LA on A behind the gate, ``between`` filler launches on a third stream (they run at once), LB on B behind the gate,
    release.  Whatever the number of launches planned in between, both outputs are complete.  (No overlap is asserted: a
    hand-out may serialise the two.  That both were queued before the gate opened is asserted: otherwise nothing was tested.)"""
    case = lab.case("pair")
    oa, ob = case.out(), case.out()
    closed = _gated_pair(lab, case, oa, ob, between=between)
    case.check(oa, f"LA, {between} launches before LB")
    case.check(ob, f"LB, {between} launches after LA")
    assert closed, "the gate opened before both launches were queued"
    lab.ctx.check()


# ---- c. one stream far behind the other -----------------------------------------------------------------------------------
def test_lagging_stream(lab):
    """200 launches on stream A held back until stream B is mid-way through its 200 (A waits for an event recorded behind B's
    100th; B itself starts behind a gate, so that everything is queued before anything runs), round-robin into four outputs
    per stream.  The last four outputs of each stream are checked.  (Nine buffers of 241 MB: 2.2 GB.)"""
    import torch
    case = lab.case("pair")
    n, nbuf = 200, 4
    outs = {s: [case.out() for _ in range(nbuf)] for s in ("A", "B")}
    streams = {"A": lab.A, "B": lab.B}

    def queue(name, lo, hi):
        for i in range(lo, hi):
            o = outs[name][i % nbuf]
            if i >= n - nbuf:
                with torch.cuda.stream(streams[name]):
                    o.fill_(NAN)
            case.launch(o, streams[name])

    torch.cuda.synchronize()
    ev = lab.gate(8.0)
    lab.B.wait_event(ev)
    queue("B", 0, n // 2)
    mid = torch.cuda.Event()
    mid.record(lab.B)
    lab.A.wait_event(mid)
    queue("A", 0, n)
    queue("B", n // 2, n)
    torch.cuda.synchronize()
    for name in ("A", "B"):
        for k, o in enumerate(outs[name]):
            case.check(o, f"stream {name}, output {k}")
    lab.ctx.check()


# ---- d. a replayed graph against direct launches ----------------------------------------------------------------------------
@pytest.mark.parametrize("between", [0, 63, 64, 65])
def test_graph_replay_against_direct_launches(lab, between):
    """One dynamic launch captured on a side stream after a warm-up there (one stream, no parallel branches); ``between``
    direct launches later, a replay on stream A and a direct launch of the same request on stream B start together.  The
    graph holds its counter for good: no direct launch may ever receive it.  Three replays."""
    import torch
    case = lab.case("pair")
    og, ob = case.out(), case.out()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        case.launch(og, side)                            # warm-up
    torch.cuda.synchronize()
    case.check(og, "warm-up on the side stream")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        case.launch(og, side)
    torch.cuda.synchronize()
    lab.fillers(between)
    for rep in range(3):
        closed = _gated_pair(lab, case, og, ob, first=graph.replay)
        case.check(og, f"replay {rep} after {between} direct launches")
        case.check(ob, f"direct launch beside replay {rep}")
        assert closed, "the gate opened before the replay and the launch were queued"
    lab.ctx.check()


# ---- e. a deep queue of mixed grids on one stream ---------------------------------------------------------------------------
def test_deep_queue_with_mixed_grids(lab):
    """128 launches on one stream with no synchronisation, alternating the two kernels and three batch sizes each (one
    request: one workgroup, no dynamic chunk; grid * 8 - 1: every workgroup, static chunks only; the dynamic size): the
    counter a large launch leaves behind serves a small one and the other way round.  Every output is compared on the
    stream (bit-equal to the serial launch), the verdicts are read once at the end."""
    import torch
    combos = []
    for k in range(3):
        combos.append(lab.case("pair", lab.shapes["pair"].sizes[(2 * k) % 3]))
        combos.append(lab.case("stacked", lab.shapes["stacked"].sizes[(2 * k + 1) % 3]))
    assert {(c.shape.key, c.nreq) for c in combos} == {(s.key, n) for s in lab.shapes.values() for n in s.sizes}
    bufs = [c.out() for c in combos]
    nlaunch = 128
    ok = torch.zeros(nlaunch, dtype=torch.bool, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for i in range(nlaunch):
            c, o = combos[i % len(combos)], bufs[i % len(combos)]
            o.fill_(NAN)
            c.launch(o, stream)
            ok[i] = (o.view(torch.int64) == c.ref.view(torch.int64)).all()
    torch.cuda.synchronize()
    bad = [(i, combos[i % len(combos)].shape.key, combos[i % len(combos)].nreq) for i in torch.nonzero(~ok).flatten().tolist()]
    assert not bad, f"launches with incomplete or different output: {bad}"
    lab.ctx.check()
