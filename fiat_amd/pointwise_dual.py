"""A dual basis of point evaluations for an element given by its basis functions (FIAT/pointwise_dual.py).

The functionals are the rows of the inverse of the transposed basis-at-points matrix: the basis is tabulated at the
points on the device and the square system is inverted there (runtime.vandermonde_solve_batch)."""
from collections import defaultdict

import numpy

from . import runtime
from .dual_set import DualSet
from .functional import Functional


def compute_pointwise_dual(el, pts):
    """DualSet of point-evaluation functionals dual to the basis of ``el`` at the unisolvent points ``pts``
    (npts, sd), one functional per basis function; weights with |w| <= 1e-12 are dropped."""
    pts = numpy.asarray(pts, dtype=float)
    ref_el = el.get_reference_element()
    sd = ref_el.get_spatial_dimension()
    nbf = el.space_dimension()
    shape = tuple(el.value_shape())
    if pts.shape != (nbf // int(numpy.prod(shape, dtype=int)), sd):
        raise ValueError(f"need {nbf} points of dimension {sd}, got shape {pts.shape}")
    V = runtime.fetch(el.tabulate_batch(0, pts[None]))[0, 0]          # (nbf, *shape, npts)
    Vm = V.reshape(nbf, -1)
    # vandermonde_solve_batch returns X = (A B^T)^{-T} B: A = V, B = I gives the inverse of V^T
    alphas = runtime.fetch(runtime.vandermonde_solve_batch(Vm, numpy.eye(nbf)))[0].reshape(V.shape)
    nodes = []
    for weights in alphas:
        pt_dict = defaultdict(list)
        for index in zip(*numpy.nonzero(numpy.abs(weights) > 1.e-12)):
            *comp, j = index
            pt_dict[tuple(pts[j])].append((weights[index], tuple(comp)))
        nodes.append(Functional(ref_el, shape, dict(pt_dict), {}, "node"))
    return DualSet(nodes, ref_el, el.entity_dofs())
