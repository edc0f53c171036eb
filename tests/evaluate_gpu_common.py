"""TEST INFRASTRUCTURE -- helpers shared by the GPU tests of ``evaluate_batch`` (tests/test_gpu_evaluate.py,
tests/test_gpu_evaluate_cells.py): elements of the fixture's cases, the restatement on an element's own coefficients, the
comparison in the project's norm, and the discipline of every fused call: a guarded output, exactly the named instance
launched."""
import math
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.join(HERE, "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import edge_reference as E  # noqa: E402  (guarded outputs, request samples, profiler records)
import evaluate_reference as R  # noqa: E402
import make_golden_evaluate as M  # noqa: E402

G = np.load(os.path.join(HERE, "golden", "evaluate.npz"))
STANDING = (1e-12, 1e-10)
_ELS = {}


def element(name, own=False):
    """The fixture's element on the UFC cell or, ``own``, built on the fixture's skewed cell ``{name}_verts``."""
    import fiat_amd
    if (name, own) not in _ELS:
        _ELS[(name, own)] = M.build(fiat_amd, name, verts=G[f"{name}_verts"] if own else None)
    return _ELS[(name, own)]


def facts(el):
    sd = el.get_reference_element().get_spatial_dimension()
    vs = tuple(el.value_shape())
    return sd, el.degree(), vs, int(np.prod(vs, dtype=int)) if vs else 1, el.space_dimension()


def restated(el, order, pts, dofs, verts=None, pushforward=False, cell=None, longdouble=False):
    """(nreq, ntab, nrhs, *value_shape, npts): the restatement, request by request, from the element's own coefficients;
    ``cell``: the cell the element is built on where that is not the UFC simplex."""
    sd, n, vs, _, _ = facts(el)
    mapping = R_MAPPINGS[el.mapping()[0]] if pushforward else 0
    return np.stack([R.evaluate(sd, n, el._expansion_variant, el._expansion_scale, el.get_coeffs(), order, pts[r], dofs[r],
                                cell=cell, verts=None if verts is None else verts[r], mapping=mapping, value_shape=vs,
                                longdouble=longdouble)
                     for r in range(len(pts))])


R_MAPPINGS = {"affine": 0, "covariant piola": 1, "contravariant piola": 2}


def check(got, ref, what, tol=STANDING):
    """Per request (ntab, ...): values and derivatives apart."""
    got, ref = np.asarray(got, dtype=float), np.asarray(ref, dtype=float)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    worst = [0.0, 0.0]
    for r in range(len(ref)):
        e0, e1 = R.errors(got[r], ref[r])
        worst = [max(worst[0], e0), max(worst[1], e1)]
        assert e0 <= tol[0], (what, r, "values", e0)
        assert e1 <= tol[1], (what, r, "derivatives", e1)
    print(f"{what}: values {worst[0]:.2e} derivatives {worst[1]:.2e}")
    return worst


def instance(el, order):
    sd, _, _, vdim, _ = facts(el)
    return f"eval_kernel<{sd},{order},{vdim}>"


def assert_launched(names, el, order):
    """Exactly the named instance ran: one device kernel, and it is that instance."""
    squeezed = {re.sub(r"\s", "", n) for n in names}
    assert len(squeezed) == 1 and instance(el, order) in next(iter(squeezed)), (names, instance(el, order))


def fused(el, order, pts, dofs, verts=None, pushforward=False, offset=1, **kw):
    """route="fused" into a guarded output, under the profiler; returns the output tensor."""
    import torch
    from fiat_amd import runtime
    sd, _, vs, _, _ = facts(el)
    dshape = tuple(dofs.shape)
    shape = (len(pts), len(E.jet(sd, order))) + (dshape[1:2] if len(dshape) == 3 else ()) + vs + (pts.shape[1],)
    buf, out = E.guarded_out(shape, offset, runtime.Context.get().device)
    res = []
    names = E.launched(lambda: res.append(el.evaluate_batch(order, pts, dofs, verts=verts, out=out, pushforward=pushforward,
                                                            route="fused", **kw)))
    torch.cuda.synchronize()
    assert res[0] is out
    assert_launched(names, el, order)
    E.check_guarded(buf, out)
    return out


def inputs(el, npts, nreq, rng, nrhs=None, lo=-0.1, hi=1.1):
    sd, _, _, _, ndof = facts(el)
    pts = rng.uniform(lo, hi, size=(nreq, npts, sd))
    dofs = rng.uniform(-1.0, 1.0, size=(nreq, ndof) if nrhs is None else (nreq, nrhs, ndof))
    return pts, dofs


def as3(dofs):
    return dofs if dofs.ndim == 3 else dofs[:, None]


def expected_plan(sd, n, order, vdim, ndof, npts):
    """(P, chunks), the arithmetic of the launcher: more than 64 points are chunks of 64 of one request; otherwise 64 // npts
    whole requests, fewer where dofs (rounded up to 4 requests) + w + image, each rounded to an even number of doubles, pass
    16 KB."""
    if npts > 64:
        return 1, -(-npts // 64)
    nexp, ntab = math.comb(n + sd, sd), math.comb(sd + order, sd)
    even = lambda x: x + (x & 1)     # noqa: E731
    P = 64 // npts
    while P > 1 and 8 * (even(-(-P // 4) * 4 * ndof) + even(P * vdim * nexp) + even(P * ntab * vdim * npts)) > 16 * 1024:
        P -= 1
    return P, 1
