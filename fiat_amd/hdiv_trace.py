"""The H(div) trace element (FIAT/hdiv_trace.py): the DG-facet space behind hybridised mixed methods and HDG.

The element carries one discontinuous element per facet of its cell -- DiscontinuousLagrange, or Legendre for the
"integral" variants, a tensor product of them on quadrilateral facets -- and nothing in the interior.  Its table (ndof,
npts) holds, at a point on facet f, the facet element's values in the rows of f and zeros in every other row; derivatives
are not defined (``TraceError``).  Without an entity the element itself decides which facet a point is on (simplices only):
the one barycentric coordinate within 1e-10 of zero.  A call with a point that is on no facet, or on more than one, is NaN
throughout.

Two routes serve ``tabulate_batch``:

* the fused kernel of csrc/trace.hpp (fx_trace_tabulate_batch, include/fiat_amd_trace.h) where all facets carry the same
  element on a UFC simplex of dimension 0-2 and the degree is at most 12: the interval, the triangle, the tetrahedron and
  quadrilaterals of equal degrees.  One pass: identify the facet, form the facet coordinates, evaluate the facet simplex's
  expansion by recurrence, contract with the facet element's matrix, write the block, the zeros or the NaNs;
* the general route everywhere else (prisms, unequal degrees, degree > 12, ``route="general"``): per facet kind the facet
  element's own ``tabulate_batch`` on the requests of that kind, placed into a zeroed output.

The values are invariant under affine maps of the cell, so there are no per-request cells (``verts=``, ``pushforward=``,
``tabulate_cells``): a caller maps the points instead."""
from collections import defaultdict

import numpy as np
import torch

from . import runtime
from .barycentric_interpolation import get_lagrange_points
from .discontinuous_lagrange import DiscontinuousLagrange
from .dual_set import DualSet
from .finite_element import FiniteElement
from .functional import IntegralMoment, PointEvaluation
from .hierarchical import Legendre
from .polynomial_set import mis
from .quadrature import FacetQuadratureRule
from .reference_element import LINE, POINT, QUADRILATERAL, TENSORPRODUCT, TETRAHEDRON, TRIANGLE, ufc_simplex
from .tensor_product import TensorProductElement

# a point is on facet i where |lambda_i| < epsilon (csrc/trace.hpp TRACE_TOL is the same number)
epsilon = 1e-10

TRACE_KERNEL_MAXDEGREE = 12      # csrc/trace.hpp: compile-time instances 0..6, the run-time-degree instance to 12


class TraceError(Exception):
    """What a trace element has no answer to: values away from the facets, and derivatives anywhere.  ``tabulate`` stores
    instances of it in the dictionary slots concerned; ``tabulate_batch`` raises it.  The text is kept in ``msg``."""

    def __init__(self, msg):
        super().__init__(msg)
        self.msg = msg


_NOT_ON_FACETS = "The HDivTrace element can only be tabulated on facets."
_NO_DERIVATIVES = "Gradients on trace elements are not well-defined."


def _facet_degrees(ref_el, degree):
    """The degree argument as the facet elements take it: one degree per factor on a product cell (a single number is
    repeated), a single number elsewhere."""
    if ref_el.get_spatial_dimension() == 0:
        raise ValueError("a point has no facets to take a trace on")
    if ref_el.get_shape() == TENSORPRODUCT:
        degrees = tuple(degree) if hasattr(degree, "__iter__") else (degree,) * len(ref_el.cells)
        if len(degrees) != len(ref_el.cells):
            raise ValueError(f"{len(ref_el.cells)} factors need {len(ref_el.cells)} degrees, got {len(degrees)}")
        return degrees
    if ref_el.get_shape() not in (LINE, TRIANGLE, TETRAHEDRON, QUADRILATERAL):
        raise NotImplementedError(f"no trace element on {type(ref_el).__name__}")
    if isinstance(degree, tuple):
        raise ValueError("a tuple of degrees needs a tensor-product cell")
    return degree


def _flat_dim(dim):
    return sum(_flat_dim(d) for d in dim) if isinstance(dim, tuple) else dim


def _kernel_weights(fd, degree):
    """The normalisation the kernel's expansion leaves out (csrc/trace.hpp), by member."""
    if fd == 0:
        return np.ones(1)
    if fd == 1:
        return np.sqrt(2.0 * np.arange(degree + 1) + 1.0)
    w = np.zeros((degree + 1) * (degree + 2) // 2)
    for p in range(degree + 1):
        for q in range(degree + 1 - p):
            w[(p + q) * (p + q + 1) // 2 + q] = np.sqrt((2.0 * p + 1.0) * (p + q + 1.0))
    return w


def _kernel_matrix(element, fd, degree):
    """The facet element over the kernel's expansion, (nf, nf), or None where the kernel does not serve it."""
    if fd == 0:
        return np.ones((1, 1))
    if isinstance(element, TensorProductElement) or not hasattr(element, "get_nodal_basis"):
        return None
    cell = element.get_reference_element()
    if not np.array_equal(np.asarray(cell.get_vertices(), dtype=float), np.asarray(ufc_simplex(fd).get_vertices(), dtype=float)):
        return None
    ps = element.get_nodal_basis()
    es = ps.get_expansion_set()
    nf = element.space_dimension()
    if nf != len(_kernel_weights(fd, degree)):
        return None
    if hasattr(es, "device_line"):
        # the primal 1-D Lagrange basis at the nodes x: l_i = sum_k C[i, k] P_k(2 x - 1) with C V^T = 1, V[j, k] = P_k(2 x_j - 1)
        V = np.polynomial.legendre.legvander(2.0 * np.asarray(es.x, dtype=float) - 1.0, degree)
        return np.ascontiguousarray(np.linalg.inv(V).T)
    if getattr(es, "variant", None) is not None or getattr(es, "num_cells", 1) != 1 or ps.get_embedded_degree() != degree:
        return None
    coeffs = np.asarray(element.get_coeffs(), dtype=float)
    if coeffs.shape != (nf, nf):
        return None
    return np.ascontiguousarray(coeffs * float(es.get_scale(degree)) * _kernel_weights(fd, degree)[None, :])


class TraceDualSet(DualSet):
    """The dual set of the trace element.  A product cell keeps no table of sub-entities: the closure of an entity is
    what its vertices contain."""

    def __init__(self, nodes, ref_el, entity_ids):
        if getattr(ref_el, "sub_entities", None) is not None:
            super().__init__(nodes, ref_el, entity_ids)
            return
        self.nodes, self.ref_el, self.entity_ids, self.entity_permutations = nodes, ref_el, entity_ids, None
        top = ref_el.get_topology()
        self.entity_closure_ids = {
            dim: {e: sorted(i for d, subs in top.items() for s, vs in subs.items() if set(vs) <= set(verts)
                            for i in entity_ids[d][s]) for e, verts in entities.items()}
            for dim, entities in top.items()}


class HDivTrace(FiniteElement):
    """The trace of H(div) elements: a stand-alone family that produces a DG-facet field."""

    def __init__(self, ref_el, degree, variant=None):
        degree = _facet_degrees(ref_el, degree)
        sd = ref_el.get_spatial_dimension()
        facet_sd = sd - 1
        topology = ref_el.get_topology()
        # one discontinuous element per kind of facet
        dg_elements = {dim: construct_dg_element(ref_el.construct_subelement(dim), degree, variant)
                       for dim in topology if _flat_dim(dim) == facet_sd}
        # the facets in dof-block order, and the dofs and nodes on them
        entity_dofs = {dim: {entity: [] for entity in topology[dim]} for dim in topology}
        nodes, self._facets, self._offsets = [], [], []
        for facet_dim in sorted(dg_elements):
            facet_nodes = dg_elements[facet_dim].dual_basis()
            for i in sorted(topology[facet_dim]):
                self._facets.append((facet_dim, i))
                self._offsets.append(len(nodes))
                nodes.extend(transform_nodes(facet_nodes, ref_el, facet_dim, i))
                entity_dofs[facet_dim][i] = list(range(self._offsets[-1], len(nodes)))
        deg = max(e.degree() for e in dg_elements.values())
        super().__init__(ref_el, TraceDualSet(nodes, ref_el, entity_dofs), order=deg, formdegree=facet_sd, mapping="affine")
        self.dg_elements = dg_elements
        self.polydegree = deg
        self.variant = variant

        # the fused kernel: one element on a UFC facet simplex for all facets
        self._kernel = None
        kinds = list(dg_elements.values())
        if facet_sd <= 2 and deg <= TRACE_KERNEL_MAXDEGREE and len({e.space_dimension() for e in kinds}) == 1 \
                and len({e.degree() for e in kinds}) == 1:
            mats = [_kernel_matrix(e, facet_sd, deg) for e in kinds]
            if all(m is not None for m in mats) and all(np.array_equal(m, mats[0]) for m in mats):
                self._kernel = {"fd": facet_sd, "degree": deg, "nfac": len(self._facets), "C": mats[0], "dev": None}
        self._bary = None
        if ref_el.get_shape() in (LINE, TRIANGLE, TETRAHEDRON):
            # lambda = lam0 + G x: the inverse of the matrix of homogeneous vertex coordinates
            v = np.asarray(ref_el.get_vertices(), dtype=float)
            M = np.linalg.inv(np.vstack([v.T, np.ones(sd + 1)]))
            self._bary = (np.ascontiguousarray(M[:, sd]), np.ascontiguousarray(M[:, :sd]))

    def degree(self):
        """The largest degree among the facet elements."""
        return self.polydegree

    def get_nodal_basis(self):
        raise NotImplementedError("get_nodal_basis not implemented for the trace element.")

    def get_coeffs(self):
        raise NotImplementedError("get_coeffs not implemented for the trace element.")

    def dmats(self):
        raise NotImplementedError("dmats not implemented for the trace element.")

    def get_num_members(self, arg):
        raise NotImplementedError("get_num_members not implemented for the trace element.")

    def value_shape(self):
        return ()

    @staticmethod
    def is_nodal():
        return True

    # -- the batched API ------------------------------------------------------------------------------------
    def _mode(self, entity, facets):
        """("identify" | "facet" | "facets", flat facet number or None)."""
        sd = self.ref_el.get_spatial_dimension()
        if facets is not None:
            if entity is not None:
                raise ValueError("give entity= or facets=, not both")
            return "facets", None
        if entity is None or tuple(entity) == (sd, 0):
            if self._bary is None:
                raise NotImplementedError(f"facets are identified on simplices only: give entity= or facets= on "
                                          f"{type(self.ref_el).__name__}")
            return "identify", None
        entity = (entity[0], entity[1])
        if entity not in self._facets:
            raise TraceError(_NOT_ON_FACETS)
        return "facet", self._facets.index(entity)

    def _fused(self, mode, route):
        if route not in (None, "general"):
            raise ValueError(f"unknown route {route!r}")
        fused = self._kernel is not None and route is None
        if mode == "identify" and not fused:
            raise NotImplementedError("the facets of points are identified by the fused kernel only "
                                      f"(simplices, degree <= {TRACE_KERNEL_MAXDEGREE})")
        return fused

    def kernel(self, npts, mode="facets", route=None):
        """Kernel instance and output route of a request shape, ``"fxk::trace_kernel<fd,degree> image|stream P=<p>"``
        (fx_trace_kernel; degree -1: the run-time-degree instance), or the string of the general route.  ``mode``:
        "identify", "facet" or "facets"; the three share the instance and the route."""
        if mode not in runtime.TRACE_MODES:
            raise ValueError(f"unknown mode {mode!r}")
        if mode == "identify" and self._bary is None:
            raise NotImplementedError("facets are identified on simplices only")
        if not self._fused(mode, route):
            return "general route: the facet elements' tabulate_batch, placed (python composition)"
        k = self._kernel
        return runtime.trace_kernel(k["fd"], k["degree"], k["nfac"], npts)

    def tabulate_batch(self, order, points, entity=None, *, facets=None, out=None, stream=None, route=None):
        """-> device tensor (nreq, 1, ndof, npts).  Three modes:

        * identify (``entity`` and ``facets`` None; simplices): points (nreq, npts, sd) in cell coordinates; the verdict is per
          request -- one with a point that is not on exactly one facet is NaN throughout, its neighbours are untouched --
          and the points of one request may lie on different facets;
        * one facet (``entity=(facet dim, id)``): points (nreq, npts, sd - 1) in facet coordinates;
        * facet per request (``facets``: int32 array or tensor (nreq,) of flat facet numbers in dof-block order): points
          (nreq, npts, sd - 1); a number out of range is a ValueError, raised before anything is launched.

        ``order > 0`` raises TraceError (a tensor cannot hold the exception objects of ``tabulate``); ``route="general"``
        forces the composition of the facet elements' own kernels (facet modes only)."""
        if order != 0:
            raise TraceError(_NO_DERIVATIVES)
        mode, facet = self._mode(entity, facets)
        fused = self._fused(mode, route)
        ctx = runtime.Context.get()
        # uploads, the range check, allocations and the general route's torch work are ordered with the kernels on ``stream``
        with torch.cuda.stream(stream):
            return self._tabulate_on_stream(mode, facet, fused, ctx, points, facets, out, stream)

    def _tabulate_on_stream(self, mode, facet, fused, ctx, points, facets, out, stream):
        points = runtime._as_device(points, ctx)
        sd = self.ref_el.get_spatial_dimension()
        pd = sd if mode == "identify" else sd - 1
        if points.dim() != 3 or points.shape[2] != pd:
            raise ValueError(f"points must have shape (nreq, npts, {pd}), got {tuple(points.shape)}")
        nreq, npts = int(points.shape[0]), int(points.shape[1])
        if mode == "facets":
            # the range is checked on the numbers as given, before they are narrowed to the kernel's int32: on the host for a
            # host array, by one reduction and one copy to the host for a device tensor; nothing has been launched yet
            if isinstance(facets, torch.Tensor):
                if facets.dim() != 1 or facets.shape[0] != nreq or facets.dtype not in (torch.int32, torch.int64):
                    raise ValueError("facets must be an integer array of shape (nreq,)")
                lo, hi = torch.stack(torch.aminmax(facets)).tolist() if nreq else (0, 0)
            else:
                facets = np.asarray(facets)
                if facets.ndim != 1 or facets.shape[0] != nreq or facets.dtype.kind not in "iu":
                    raise ValueError("facets must be an integer array of shape (nreq,)")
                lo, hi = (int(facets.min()), int(facets.max())) if nreq else (0, 0)
                facets = torch.as_tensor(np.ascontiguousarray(facets, dtype=np.int64))
            if lo < 0 or hi >= len(self._facets):
                raise ValueError(f"facet numbers must lie in 0..{len(self._facets) - 1}")
            facets = facets.to(device=ctx.device, dtype=torch.int32).contiguous()
        if fused:
            k = self._kernel
            if k["dev"] is None or k["dev"].device != ctx.device:
                k["dev"] = runtime._as_device(k["C"], ctx)
            lam0, G = self._bary if mode == "identify" else (None, None)
            return runtime.trace_tabulate_batch(k["fd"], k["degree"], k["nfac"], k["dev"], mode, points, facet=facet or 0,
                                                facets=facets, lam0=lam0, G=G, out=out, stream=stream, ctx=ctx)
        return self._general(points, facet, facets, out, stream, ctx)

    def _general(self, points, facet, facets, out, stream, ctx):
        nreq, npts = int(points.shape[0]), int(points.shape[1])
        shape = (nreq, 1, self.space_dimension(), npts)
        if out is None:
            out = torch.zeros(shape, dtype=torch.float64, device=ctx.device)
        elif tuple(out.shape) != shape or out.dtype != torch.float64 or not out.is_contiguous() or out.device != ctx.device:
            raise ValueError("out has the wrong shape/dtype/layout")
        else:
            out.zero_()
        if nreq == 0 or npts == 0:
            return out
        number = torch.full((nreq,), facet, dtype=torch.int64, device=ctx.device) if facets is None else facets.to(torch.int64)
        kind_of = [sorted(self.dg_elements).index(dim) for dim, _ in self._facets]
        kinds = torch.as_tensor(kind_of, device=ctx.device)[number]
        offsets = torch.as_tensor(self._offsets, device=ctx.device)[number]
        for kind, dim in enumerate(sorted(self.dg_elements)):
            idx = torch.nonzero(kinds == kind).reshape(-1)
            if idx.numel() == 0:
                continue
            element = self.dg_elements[dim]
            nf = element.space_dimension()
            if _flat_dim(dim) == 0:
                block = torch.ones((idx.numel(), nf, npts), dtype=torch.float64, device=ctx.device)
            else:
                block = element.tabulate_batch(0, points[idx].contiguous(), stream=stream)[:, 0]
            rows = offsets[idx][:, None] + torch.arange(nf, device=ctx.device)[None, :]
            out[idx[:, None], 0, rows] = block
        return out

    # -- the reference's dictionary ---------------------------------------------------------------------------
    def tabulate(self, order, points, entity=None):
        """{alpha: (ndof, npts)}: the values under (0,) * sd, a TraceError instance under every derivative key.  ``entity=None``
        (simplices): the facet of every point is identified with tolerance 1e-10, and if any point fails every array is NaN;
        ``entity=(sd, 0)`` takes the same path and holds TraceError instances on failure; ``entity=(facet dim, id)``: points
        in facet coordinates; any other entity: TraceError in every slot."""
        sd = self.ref_el.get_spatial_dimension()
        evalkey = (0,) * sd
        npts = len(points)
        phivals = {}
        for i in range(order + 1):
            for alpha in mis(sd, i):
                phivals[alpha] = TraceError(_NO_DERIVATIVES)
        phivals[evalkey] = np.zeros((self.space_dimension(), npts))
        whole = entity is None or tuple(entity) == (sd, 0)
        try:
            self._mode(entity, None)
        except TraceError as err:
            return {key: TraceError(err.msg) for key in phivals}
        if npts == 0:
            return phivals
        pd = sd if whole else sd - 1
        pts = np.asarray(points, dtype=float).reshape(1, npts, pd)
        table = runtime.fetch(self.tabulate_batch(0, pts, entity=entity))[0, 0]
        if whole and np.isnan(table).any():
            if entity is None:
                phivals[evalkey] = table
            else:
                return {key: TraceError(_NOT_ON_FACETS) for key in phivals}
        else:
            phivals[evalkey] = np.ascontiguousarray(table)
        return phivals


def construct_dg_element(ref_el, degree, variant):
    """The discontinuous element a facet of shape ``ref_el`` carries: ``Legendre`` where the variant starts with "integral",
    ``DiscontinuousLagrange`` otherwise, on points, intervals and triangles; their tensor product on a quadrilateral (same
    degree twice) and on a product cell (``degree``: one per factor; point factors contribute nothing, and a single
    remaining factor is returned as it is)."""
    family = Legendre if (variant or "").startswith("integral") else DiscontinuousLagrange
    shape = ref_el.get_shape()
    if shape in (POINT, LINE, TRIANGLE):
        return family(ref_el, degree, variant)
    if shape == QUADRILATERAL:
        factors = [family(ufc_simplex(1), degree, variant)] * 2
    elif shape == TENSORPRODUCT:
        if len(degree) != len(ref_el.cells):
            raise ValueError(f"{len(ref_el.cells)} factors need {len(ref_el.cells)} degrees, got {len(degree)}")
        factors = [construct_dg_element(c, d, variant) for c, d in zip(ref_el.cells, degree) if c.get_shape() != POINT]
    else:
        raise NotImplementedError(f"no facet element on {type(ref_el).__name__}")
    return factors[0] if len(factors) == 1 else TensorProductElement(*factors)


def transform_nodes(ells, ref_el, facet_dim, facet_id):
    """The nodes ``ells`` of a facet element as nodes of the cell, on facet (facet_dim, facet_id).  Nodes of one point each
    become point evaluations at the images of their points under the facet's entity transform; otherwise they are integral
    moments sharing one rule, and become moments of the same test values on that rule mapped onto the facet."""
    if all(len(ell.get_point_dict()) == 1 for ell in ells):
        to_cell = ref_el.get_entity_transform(facet_dim, facet_id)
        return [PointEvaluation(ref_el, tuple(x)) for x in to_cell(get_lagrange_points(ells))]
    rules = {id(ell.Q): ell.Q for ell in ells}
    if len(rules) != 1:
        raise ValueError("the moments of a facet element share one quadrature rule")
    on_facet = FacetQuadratureRule(ref_el, facet_dim, facet_id, next(iter(rules.values())))
    return [IntegralMoment(ref_el, on_facet, ell.f_at_qpts) for ell in ells]


def extract_facets(coordinates, tolerance=epsilon):
    """({facet: point indices}, success) for points given in barycentric coordinates: a point is on facet i where exactly
    its i-th coordinate is within ``tolerance`` of zero; success is False (and the dict empty) as soon as a point is on no
    facet or on more than one.  On the interval the facet ids are swapped (facet i is vertex i there)."""
    facet_to_pts = defaultdict(list)
    for ipt, c in enumerate(coordinates):
        on_facet = [i for i, lam in enumerate(c) if abs(lam) < tolerance]
        if len(on_facet) != 1:
            return {}, False
        facet_to_pts[on_facet[0]].append(ipt)
    if len(coordinates[0]) == 2:
        facet_to_pts[0], facet_to_pts[1] = facet_to_pts[1], facet_to_pts[0]
    return facet_to_pts, True


def barycentric_coordinates(points, vertices):
    """(npts, nverts) barycentric coordinates of points relative to the simplex of the given vertices."""
    vertices = np.asarray(vertices, dtype=float)
    T = (vertices[:-1] - vertices[-1]).T
    bary = (np.asarray(points, dtype=float).reshape(-1, vertices.shape[1]) - vertices[-1]) @ np.linalg.inv(T).T
    return np.concatenate([bary, 1.0 - bary.sum(axis=1, keepdims=True)], axis=1)


def map_from_reference_facet(point, vertices):
    """The physical coordinates of a point of the reference facet simplex, on the facet with the given vertices."""
    vertices = np.asarray(vertices, dtype=float)
    coords = barycentric_coordinates([point], ufc_simplex(len(vertices) - 1).get_vertices())[0]
    return tuple(coords @ vertices)


def map_to_reference_facet(points, vertices, facet):
    """Points on facet ``facet`` of the simplex with the given vertices -> their coordinates on the reference facet simplex:
    the barycentric coordinates with the facet's own dropped, read on the UFC simplex of one dimension less."""
    all_coords = barycentric_coordinates(points, vertices)
    reference_vertices = np.asarray(ufc_simplex(len(vertices) - 2).get_vertices(), dtype=float).reshape(len(vertices) - 1, -1)
    keep = [j for j in range(all_coords.shape[1]) if j != facet]
    return [coords[keep] @ reference_vertices for coords in all_coords]
