"""DPC elements on quadrilaterals and hexahedra (FIAT/discontinuous_pc.py): the discontinuous space that closes the
serendipity complex.

A Ciarlet element: P_k over the expansion set of the *simplex* of the cell's dimension, dual to point evaluation at the
equispaced degree-k lattice of that simplex, which an affine map places over the cube (the hexahedron's mapped simplex has one
vertex outside the cell: the reference's recipe, mirrored).  Construction is the inherited one: the Vandermonde matrix is
assembled and solved on the device.  Tabulation of degree 1-6 with order 0-2 does not use the coefficients: the nodal basis
of an equispaced lattice has the closed form prod_i l_{alpha_i}(lambda_i(x)), evaluated by the HIP kernel of csrc/dpc.hpp
(fx_dpc_tabulate_batch, include/fiat_amd_dpc.h).  Everything else -- degree 0, degree >= 7, order >= 3 -- takes the general
route, the simplex contraction kernels on the cube's points.

Cells: UFCQuadrilateral, UFCHexahedron, and products of UFC intervals (entity ids keyed as the product cell keys them).  The
reference constructs DPC on such a product but its ``tabulate`` raises a TypeError there, so the tests take metadata and
nodes of product cells from the reference and check tables against the NumPy restatement only.  A product that does not
flatten to a UFC cell raises the reference's KeyError (its ``hypercube_simplex_map`` has no entry).  A bilinear cell is no
affine image, so there are no per-request cells (``verts=``) and no ``tabulate_cells``."""
import numpy

from . import runtime
from .finite_element import CiarletElement
from .functional import PointEvaluation
from .polynomial_set import ONPolynomialSet, mis
from .reference_element import (DefaultLine, Point, UFCHexahedron, UFCInterval, UFCQuadrilateral, UFCTetrahedron,
                                UFCTriangle, flatten_reference_cube, make_affine_mapping)
from .serendipity import SerendipityDualSet, _flat

hypercube_simplex_map = {Point(): Point(),
                         DefaultLine(): DefaultLine(),
                         UFCInterval(): UFCInterval(),
                         UFCQuadrilateral(): UFCTriangle(),
                         UFCHexahedron(): UFCTetrahedron()}

DPC_KERNEL_MAXK, DPC_KERNEL_MAXORDER = 6, 2     # the compile-time instances of csrc/dpc.hpp


def _cube(ref_el):
    """The flattened cell, or NotImplementedError where the reference's DPC is not a quadrilateral or hexahedron element."""
    if ref_el.get_spatial_dimension() not in (2, 3):
        raise NotImplementedError("DPC is implemented on quadrilaterals and hexahedra "
                                  "(equispaced DG on a line is DiscontinuousLagrange)")
    try:
        return flatten_reference_cube(ref_el)
    except TypeError:
        raise NotImplementedError(f"DPC is implemented on quadrilaterals and hexahedra, not on {type(ref_el).__name__}")


def _top_only(ref_el, ndof):
    """Entity ids on the cube's own topology keys: every dof on the cell itself."""
    topology = ref_el.get_topology()
    ids = {dim: {entity: [] for entity in sorted(topology[dim])} for dim in sorted(topology)}
    ids[sorted(topology)[-1]][0] = list(range(ndof))
    return ids


def simplex_on_cube(flat_el):
    """(A, b, v): the affine map x -> A x + b from the simplex of ``hypercube_simplex_map`` onto the simplex with vertices
    ``v`` over the cube (FIAT/discontinuous_pc.py:59-73): the first two vertices stay, every further one goes to the midpoint
    of an edge / beyond a face."""
    simplex = hypercube_simplex_map[flat_el]
    v_hypercube = flat_el.get_vertices()
    v = [v_hypercube[0], v_hypercube[int(-0.5 * len(v_hypercube))]]
    for d in range(1, flat_el.get_dimension()):
        v.append(tuple(numpy.asarray(v_hypercube[flat_el.get_dimension() - d]) + numpy.average(numpy.asarray(v_hypercube[::2]), axis=0)))
    A, b = make_affine_mapping(simplex.get_vertices(), tuple(v))
    return A, b, numpy.asarray(v, dtype=float)


class _DPC0Dual(SerendipityDualSet):
    """One node at the cell's barycentre, on the cell itself (P0Dual of the reference; ``entity_permutations`` is None)."""

    def __init__(self, ref_el):
        centre = tuple(numpy.average(numpy.asarray(ref_el.get_vertices(), dtype=float), axis=0))
        super().__init__([PointEvaluation(ref_el, centre)], ref_el, _top_only(ref_el, 1))


class DPCDualSet(SerendipityDualSet):
    """The dual basis for DPC elements: point evaluation at the equispaced lattice of the mapped simplex, in the order of the
    simplex's entities, every node topologically on the cell itself (FIAT/discontinuous_pc.py:49-97)."""

    def __init__(self, ref_el, flat_el, degree):
        A, b, _ = simplex_on_cube(flat_el)
        simplex = hypercube_simplex_map[flat_el]
        top = simplex.get_topology()
        nodes = []
        for dim in sorted(top):
            for entity in sorted(top[dim]):
                for x in simplex.make_points(dim, entity, degree):
                    nodes.append(PointEvaluation(flat_el, tuple(numpy.matmul(A, numpy.array(x)) + b)))
        super().__init__(nodes, ref_el, _top_only(ref_el, len(nodes)))


class _DPCBase(CiarletElement):
    """What DPC0 and HigherOrderDPC share: the cube as reference cell over a simplex's polynomial set, sub-entity points
    through the cube's entity transforms, and the routing of ``tabulate_batch``."""

    def __init__(self, ref_el, degree, dual):
        flat_el = _cube(ref_el)
        self.flat_el = flat_el
        poly_set = ONPolynomialSet(hypercube_simplex_map[flat_el], degree)
        super().__init__(poly_set=poly_set, dual=dual, order=degree, ref_complex=ref_el,
                         formdegree=flat_el.get_spatial_dimension())
        sd = flat_el.get_spatial_dimension()
        # lambda = lam0 + G x on the mapped simplex: the inverse of its matrix of homogeneous vertex coordinates
        _, _, v = simplex_on_cube(flat_el)
        M = numpy.linalg.inv(numpy.vstack([v.T, numpy.ones(sd + 1)]))
        self._lam0 = numpy.ascontiguousarray(M[:, sd])
        self._G = numpy.ascontiguousarray(M[:, :sd])

    def entity_map(self, entity):
        """(M, b) of x = M xi + b from the cell's get_entity_transform; None for the cell itself."""
        if entity is None:
            return None
        dim, number = entity
        sd = self.flat_el.get_spatial_dimension()
        edim = sum(_flat(dim))
        if edim == sd:
            if number != 0:
                raise ValueError("a cube has a single cell")
            return None
        f = self.ref_el.get_entity_transform(dim, number)
        b = numpy.asarray(f(numpy.zeros((1, edim))), dtype=float).reshape(sd)
        M = numpy.zeros((sd, edim))
        for i in range(edim):
            unit = numpy.zeros((1, edim))
            unit[0, i] = 1.0
            M[:, i] = numpy.asarray(f(unit), dtype=float).reshape(sd) - b
        return M, b

    def _direct(self, order):
        return 1 <= self.order <= DPC_KERNEL_MAXK and 0 <= order <= DPC_KERNEL_MAXORDER

    def kernel(self, order, npts, nreq=1):
        """Kernel instance and output route of a request shape: ``"fxk::dpc_kernel<sd,degree,order> image|stream P=<p>"``
        (fx_dpc_kernel), or the string of the general route beyond the direct kernel's instances: its kernel (fx_plan_kernel) for
        orders 0-2, the differentiation-matrix route above."""
        if self._direct(order):
            return runtime.dpc_kernel(self.flat_el.get_spatial_dimension(), self.order, order, npts)
        if order > 2:   # (fx_plan_kernel names the kernels of orders 0-2 only)
            return "general route: differentiation matrices (fx_tabulate_batch, order > 2)"
        return self.device_polyset().kernel_name(order, nreq, npts)

    def out_shape(self, order, nreq, npts):
        sd = self.flat_el.get_spatial_dimension()
        return (nreq, runtime.num_tables(sd, order), self.space_dimension(), npts)

    def tabulate(self, order, points, entity=None):
        """{alpha: (ndof, npts)} of all derivatives up to ``order``; ``entity=(dim, id)``: the points are in the coordinates
        of that sub-entity of the element's cell."""
        points = numpy.asarray(points, dtype=float)
        sd = self.flat_el.get_spatial_dimension()
        if points.ndim != 2:
            raise ValueError("points must have shape (npts, dimension of the entity)")
        dev = self.tabulate_batch(order, points[None], entity=entity)
        out = runtime.fetch(dev)[0]
        keys = [a for k in range(order + 1) for a in mis(sd, k)]
        return {a: numpy.ascontiguousarray(out[t]) for t, a in enumerate(keys)}

    def tabulate_batch(self, order, points, verts=None, out=None, stream=None, pushforward=False, entity=None, *, route=None):
        """points (nreq, npts, sd) -> device tensor (nreq, ntab, ndof, npts), tables in mis() order.  ``entity=(dim, id)``:
        points (nreq, npts, dim) on that sub-entity, mapped into the cell on the device (fx_map_points) before the same
        kernel runs.  ``verts`` must stay None (a bilinear cell is no affine image); ``pushforward`` changes nothing.
        Degree 1-6 with order 0-2 runs the closed-form kernel (fx_dpc_tabulate_batch); everything else, and
        ``route="general"`` (for tests and benchmarks), the inherited contraction of the nodal coefficients."""
        if verts is not None:
            raise NotImplementedError("DPC elements have no per-request cells")
        if route not in (None, "general"):
            raise ValueError(f"unknown route {route!r}")
        emap = self.entity_map(entity)
        if emap is not None:
            points = runtime.map_points(*emap, points, stream=stream)
        if route == "general" or not self._direct(order):
            return self.device_polyset().tabulate_batch(order, points, out=out, stream=stream)
        sd = self.flat_el.get_spatial_dimension()
        return runtime.dpc_tabulate_batch(sd, self.order, self._lam0, self._G, int(order), points, out=out, stream=stream)

    def tabulate_cells(self, order, ref_points, verts, out=None, stream=None, entity=None):
        raise NotImplementedError("DPC elements have no per-request cells")


class DPC0(_DPCBase):
    def __init__(self, ref_el):
        _cube(ref_el)
        super().__init__(ref_el, 0, _DPC0Dual(ref_el))


class HigherOrderDPC(_DPCBase):
    """The DPC finite element (FIAT/discontinuous_pc.py:100-112)."""

    def __init__(self, ref_el, degree):
        degree = int(degree)
        if degree < 1:
            raise ValueError("the degree of a HigherOrderDPC element is positive")
        super().__init__(ref_el, degree, DPCDualSet(ref_el, _cube(ref_el), degree))


def DPC(ref_el, degree):
    if degree == 0:
        return DPC0(ref_el)
    else:
        return HigherOrderDPC(ref_el, degree)
