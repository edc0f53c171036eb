"""Bernstein elements on simplices (FIAT/bernstein.py).

Not a Ciarlet element: the basis is given by formula, B_k = n!/prod k_i! prod lambda_i^k_i for the multi-indices k in
mis(sd+1, n), evaluated directly in barycentric coordinates by the HIP kernels of csrc/bernstein.hpp
(fx_bernstein_tabulate_batch / _shared) -- no expansion set, no coefficient contraction.  The dual is the pointwise dual
at the GLL lattice (pointwise_dual.py).

One deliberate deviation from the reference: where the derivative order equals the degree (>= 2) the tables hold the
exact value n!/(n-o)! B^{n-o}_{k-beta} = n!; the reference returns 1 there."""
import numpy
import torch

from . import runtime
from ._lib import check, host_ptr, lib
from .dual_set import DualSet
from .finite_element import CiarletElement, FiniteElement
from .pointwise_dual import compute_pointwise_dual
from .polynomial_set import mis
from .reference_element import make_lattice


def bernstein_entity_ids(ref_el, degree):
    """{dim: {entity: [dofs]}}: dof i (multi-index ks = mis(sd+1, degree)[i]) lives on the sub-entity spanned by the
    vertices where ks is nonzero (host computation only).  Degree 0 (which the reference cannot build) puts its one dof
    on the cell."""
    topology = ref_el.get_topology()
    entity_ids = {dim: {entity: [] for entity in entities} for dim, entities in topology.items()}
    by_vertices = {tuple(sorted(vertices)): (dim, entity) for dim, entities in topology.items()
                   for entity, vertices in entities.items()}
    for i, ks in enumerate(mis(ref_el.get_spatial_dimension() + 1, degree)):
        support = tuple(v for v, k in enumerate(ks) if k)
        dim, entity = by_vertices[support] if support else (ref_el.get_spatial_dimension(), 0)
        entity_ids[dim][entity].append(i)
    return entity_ids


class BernsteinDualSet(DualSet):
    """The entity layout of the Bernstein basis; the functionals are filled in by the pointwise dual."""

    def __init__(self, ref_el, degree):
        entity_ids = bernstein_entity_ids(ref_el, degree)
        ndof = sum(len(dofs) for entities in entity_ids.values() for dofs in entities.values())
        super().__init__([None] * ndof, ref_el, entity_ids)


def _check_simplex(ref_el):
    sd = ref_el.get_spatial_dimension()
    if not ref_el.is_simplex() or len(ref_el.get_vertices()) != sd + 1 or not 1 <= sd <= 3:
        raise ValueError("Bernstein elements are defined on simplices of dimension 1..3")


class Bernstein(FiniteElement):
    """A finite element with Bernstein polynomials as basis functions."""

    entity_map = CiarletElement.entity_map

    def __init__(self, ref_el, degree):
        _check_simplex(ref_el)
        degree = int(degree)
        if degree < 0:
            raise ValueError("the degree of a Bernstein element is non-negative")
        super().__init__(ref_el, BernsteinDualSet(ref_el, degree), degree, 0)
        self._cell = numpy.ascontiguousarray(ref_el.get_vertices(), dtype=numpy.float64)
        self.dual = compute_pointwise_dual(self, make_lattice(ref_el.get_vertices(), degree, variant="gll"))

    def degree(self):
        return self.get_order()

    def value_shape(self):
        return ()

    def out_shape(self, order, nreq, npts):
        sd = self.ref_el.get_spatial_dimension()
        return (nreq, runtime.num_tables(sd, order), self.space_dimension(), npts)

    def _out(self, order, nreq, npts, out, ctx):
        shape = self.out_shape(order, nreq, npts)
        if out is None:
            return torch.empty(shape, dtype=torch.float64, device=ctx.device)
        if tuple(out.shape) != shape or out.dtype != torch.float64 or not out.is_contiguous() or out.device != ctx.device:
            raise ValueError("out has the wrong shape/dtype/layout")
        return out

    def tabulate(self, order, points, entity=None):
        """{alpha: (ndof, npts)} of all derivatives up to ``order`` (a single point tuple: (ndof,)); ``entity=(dim, id)``:
        the points are in the coordinates of that reference sub-entity."""
        points = numpy.asarray(points, dtype=float)
        sd = self.ref_el.get_spatial_dimension()
        edim = sd if entity is None else entity[0]
        if edim == 0:
            single = points.ndim == 0 or (points.ndim == 1 and points.size == 0)
            npts = 1 if single else len(points)
        else:
            single = points.ndim == 1
            npts = points.size // edim
        dev = self.tabulate_batch(order, points.reshape(1, npts, edim), entity=entity)
        out = runtime.fetch(dev)[0]
        keys = [a for k in range(order + 1) for a in mis(sd, k)]
        return {a: numpy.ascontiguousarray(out[t][..., 0] if single else out[t]) for t, a in enumerate(keys)}

    def tabulate_batch(self, order, points, verts=None, out=None, stream=None, pushforward=False, entity=None):
        """points (nreq, npts, sd) [+ per-request cells verts (nreq, sd+1, sd): the basis of Bernstein(verts[r], n) at
        physical points, physical derivatives] -> device tensor (nreq, ntab, ndof, npts), tables in mis() order.
        ``pushforward`` changes nothing (the map is affine).  ``entity=(dim, id)``: points (nreq, npts, dim) on that
        reference sub-entity."""
        ctx = runtime.Context.get()
        emap = self.entity_map(entity)
        if emap is not None:
            if verts is not None:
                raise NotImplementedError("sub-entity points with per-request cells: use tabulate_cells(..., entity=)")
            points = runtime.map_points(*emap, points, stream=stream)
        sd = self.ref_el.get_spatial_dimension()
        pts = runtime._as_device(points, ctx)
        if pts.dim() != 3 or pts.shape[2] != sd:
            raise ValueError(f"points must have shape (nreq, npts, {sd}), got {tuple(pts.shape)}")
        nreq, npts = pts.shape[0], pts.shape[1]
        if verts is not None:
            verts = runtime._as_device(verts, ctx)
            if tuple(verts.shape) != (nreq, sd + 1, sd):
                raise ValueError("verts must have shape (nreq, sd+1, sd)")
        out = self._out(order, nreq, npts, out, ctx)
        check(lib.fx_bernstein_tabulate_batch(ctx.handle, sd, self.degree(), host_ptr(self._cell), int(order), nreq, npts,
                                              runtime._dev_ptr(pts),
                                              None if verts is None else runtime._dev_ptr(verts),
                                              runtime._dev_ptr(out), runtime._stream_ptr(stream)))
        return out

    def tabulate_cells(self, order, ref_points, verts, out=None, stream=None, entity=None):
        """ONE point set (npts, sd) on this element's cell (or, ``entity=``, on a reference sub-entity) pushed to the
        cells ``verts`` (nreq, sd+1, sd) -> (nreq, ntab, ndof, npts), equal to tabulate_batch(order, F_r(ref_points),
        verts)."""
        ctx = runtime.Context.get()
        emap = self.entity_map(entity)
        if emap is not None:
            ref_points = runtime.map_points(*emap, ref_points, stream=stream)
        sd = self.ref_el.get_spatial_dimension()
        pts = runtime._as_device(ref_points, ctx)
        if pts.dim() != 2 or pts.shape[1] != sd:
            raise ValueError(f"reference points must have shape (npts, {sd}), got {tuple(pts.shape)}")
        verts = runtime._as_device(verts, ctx)
        if verts.dim() != 3 or tuple(verts.shape[1:]) != (sd + 1, sd):
            raise ValueError("verts must have shape (nreq, sd+1, sd)")
        nreq, npts = verts.shape[0], pts.shape[0]
        out = self._out(order, nreq, npts, out, ctx)
        check(lib.fx_bernstein_tabulate_shared(ctx.handle, sd, self.degree(), host_ptr(self._cell), int(order), nreq, npts,
                                               runtime._dev_ptr(pts), runtime._dev_ptr(verts), runtime._dev_ptr(out),
                                               runtime._stream_ptr(stream)))
        return out

