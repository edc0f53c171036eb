"""Serendipity elements S_k on quadrilaterals and hexahedra (FIAT/serendipity.py).

Not a Ciarlet element: the basis is given by formula.  Every basis function is a signed product of one 1-D function per
direction of the flattened cell -- lambda0, lambda1 or lambda0 lambda1 L_j(2 x - (v0 + v1)) -- listed in the dof table
``runtime.serendipity_descriptor`` and evaluated directly by the HIP kernels of csrc/serendipity.hpp
(fx_serendipity_tabulate_batch, include/fiat_amd_serendipity.h): no sympy, no expansion set, no coefficient contraction.
The dual is the pointwise dual at ``unisolvent_pts`` (pointwise_dual.py).  The reference defines S_k on axis-aligned boxes
only, so there are no per-request cells (``verts=``) and no ``tabulate_cells``."""
import numpy

from . import runtime
from .dual_set import DualSet
from .finite_element import FiniteElement
from .functional import Functional
from .lagrange import Lagrange
from .pointwise_dual import compute_pointwise_dual
from .polynomial_set import mis
from .reference_element import flatten_reference_cube, make_lattice


def tr(n):
    """Face functions of S_n per face (FIAT/serendipity.py:26-30)."""
    return 0 if n <= 1 else ((n - 3) * (n - 2)) // 2


def serendipity_entity_ids(flat_el, degree):
    """{dim: {entity: [dofs]}} on the flattened cell: one dof per vertex, degree - 1 per edge, tr(degree) per face, the
    rest on the hexahedron's interior, numbered in that order (FIAT/serendipity.py:82-107; host computation only)."""
    sd = flat_el.get_spatial_dimension()
    topology = flat_el.get_topology()
    per_entity = {0: 1, 1: degree - 1, 2: tr(degree)}
    ids, cur = {dim: {} for dim in topology}, 0
    for dim in (0, 1, 2):
        for entity in sorted(topology[dim]):
            ids[dim][entity] = list(range(cur, cur + per_entity[dim]))
            cur += per_entity[dim]
    if sd == 3:
        ndof = len(runtime.serendipity_descriptor(3, degree))
        ids[3] = {0: list(range(cur, ndof))}
    return ids


def _unflatten(ref_el, flat_ids):
    """Entity ids keyed as ``ref_el`` keys its entities: a product cell's dimension tuples and numbers, counted per
    flattened dimension in the sorted order of the tuples (FIAT/dual_set.py:279-288)."""
    topology = ref_el.get_topology()
    out, counters = {dims: {} for dims in topology}, {}
    for dims in sorted(topology):
        flat = sum(_flat(dims))
        for number in sorted(topology[dims]):
            i = counters.get(flat, 0)
            counters[flat] = i + 1
            out[dims][number] = flat_ids[flat][i]
    return out


def _flat(d):
    return sum((_flat(x) for x in d), ()) if isinstance(d, tuple) else (d,)


class SerendipityDualSet(DualSet):
    """Nodes and entity ids on a hypercube or on a product cell (whose sub-entities the closure ids are found from by
    their vertex sets)."""

    def __init__(self, nodes, ref_el, entity_ids):
        self.nodes = nodes
        self.ref_el = ref_el
        self.entity_ids = entity_ids
        self.entity_permutations = None
        topology = ref_el.get_topology()
        self.entity_closure_ids = {}
        for dim, entities in topology.items():
            self.entity_closure_ids[dim] = {}
            for e, vids in entities.items():
                inside = frozenset(vids)
                self.entity_closure_ids[dim][e] = sorted(i for d, es in topology.items() for se, v in es.items()
                                                         if inside.issuperset(v) for i in entity_ids[d][se])


class _OnFlatCell:
    """The element as compute_pointwise_dual sees it: on the flattened cell, with that cell's entity numbering."""

    def __init__(self, el):
        self._el = el

    def get_reference_element(self):
        return self._el.flat_el

    def space_dimension(self):
        return self._el.space_dimension()

    def value_shape(self):
        return ()

    def entity_dofs(self):
        return self._el._flat_ids

    def tabulate_batch(self, order, points):
        return self._el.tabulate_batch(order, points)


class Serendipity(FiniteElement):
    """The scalar serendipity element S_degree (FIAT/serendipity.py:51-177)."""

    def __new__(cls, ref_el, degree):
        dim = ref_el.get_spatial_dimension()
        if dim == 1:
            return Lagrange(ref_el, degree)
        if dim == 0:
            raise IndexError("reference element cannot be dimension 0")
        return super().__new__(cls)

    def __init__(self, ref_el, degree):
        flat_el = flatten_reference_cube(ref_el)
        sd = flat_el.get_spatial_dimension()
        if sd not in (2, 3):
            raise NotImplementedError("Serendipity elements are defined on quadrilaterals and hexahedra")
        degree = int(degree)
        if degree < 1:
            raise ValueError("the degree of a Serendipity element is positive")
        verts = numpy.asarray(flat_el.get_vertices(), dtype=numpy.float64)
        self.flat_el = flat_el
        self._lo = numpy.ascontiguousarray(verts[0])      # first and last vertex: the box (FIAT/serendipity.py:69-80)
        self._hi = numpy.ascontiguousarray(verts[-1])
        self._flat_ids = serendipity_entity_ids(flat_el, degree)
        self._ndof = sum(len(dofs) for entities in self._flat_ids.values() for dofs in entities.values())
        product = ref_el.get_dimension() != max(self._flat_ids)
        entity_ids = _unflatten(ref_el, self._flat_ids) if product else self._flat_ids
        super().__init__(ref_el, SerendipityDualSet([None] * self._ndof, ref_el, entity_ids), degree, 0)
        flat_dual = compute_pointwise_dual(_OnFlatCell(self), unisolvent_pts(ref_el, degree))
        nodes = flat_dual.get_nodes()
        if product:
            nodes = [Functional(ref_el, (), n.get_point_dict(), {}, "node") for n in nodes]
        self.dual = SerendipityDualSet(nodes, ref_el, entity_ids)

    def degree(self):
        return self.order + 1

    def value_shape(self):
        return ()

    def space_dimension(self):
        return self._ndof

    def get_coeffs(self):
        raise NotImplementedError(f"get_coeffs not implemented for {type(self).__name__}")

    def kernel(self, order, npts):
        """Name of the kernel instance and output route of a request shape (fx_serendipity_kernel)."""
        return runtime.serendipity_kernel(self.flat_el.get_spatial_dimension(), self.order, order, npts)

    def out_shape(self, order, nreq, npts):
        sd = self.flat_el.get_spatial_dimension()
        return (nreq, runtime.num_tables(sd, order), self._ndof, npts)

    def tabulate(self, order, points, entity=None):
        """{alpha: (ndof, npts)} of all derivatives up to ``order``; ``entity=(dim, id)``: the points are in the coordinates
        of that sub-entity of the element's cell (FIAT/serendipity.py:134-174)."""
        points = numpy.asarray(points, dtype=float)
        sd = self.flat_el.get_spatial_dimension()
        if points.ndim != 2:
            raise ValueError("points must have shape (npts, dimension of the entity)")
        dev = self.tabulate_batch(order, points[None], entity=entity)
        out = runtime.fetch(dev)[0]
        keys = [a for k in range(order + 1) for a in mis(sd, k)]
        return {a: numpy.ascontiguousarray(out[t]) for t, a in enumerate(keys)}

    def tabulate_batch(self, order, points, verts=None, out=None, stream=None, pushforward=False, entity=None):
        """points (nreq, npts, sd) -> device tensor (nreq, ntab, ndof, npts), tables in mis() order.  ``entity=(dim, id)``:
        points (nreq, npts, dim) on that sub-entity, mapped into the cell on the device (fx_map_points) before the same
        kernel runs.  ``verts`` must stay None (S_k lives on axis-aligned boxes: a bilinear cell is no affine image);
        ``pushforward`` changes nothing (the mapping is affine on the element's own cell)."""
        if verts is not None:
            raise NotImplementedError("Serendipity elements have no per-request cells")
        sd = self.flat_el.get_spatial_dimension()
        if entity is not None and entity[0] != self.ref_el.get_dimension():
            points = runtime.map_points(*self._entity_affine(entity), points, stream=stream)
        return runtime.serendipity_tabulate_batch(sd, self.order, self._lo, self._hi, int(order), points, out=out, stream=stream)

    def _entity_affine(self, entity):
        """(M, b) of x = M xi + b, from the cell's get_entity_transform."""
        dim, number = entity
        sd = self.flat_el.get_spatial_dimension()
        f = self.ref_el.get_entity_transform(dim, number)
        edim = sum(_flat(dim))
        b = numpy.asarray(f(numpy.zeros((1, edim))), dtype=float).reshape(sd)
        M = numpy.zeros((sd, edim))
        for i in range(edim):
            unit = numpy.zeros((1, edim))
            unit[0, i] = 1.0
            M[:, i] = numpy.asarray(f(unit), dtype=float).reshape(sd) - b
        return M, b


def unisolvent_pts(K, deg):
    """Points at which S_deg is unisolvent (FIAT/serendipity.py:228-297): the vertices, deg - 1 points inside every edge,
    a triangular lattice inside every face (the cell itself for a quadrilateral) from degree 4, and a tetrahedral lattice
    inside the hexahedron from degree 6 (which, as in the reference, steps along the unit axes from the first vertex).
    The S basis is not dual to them; compute_pointwise_dual builds the dual basis."""
    flat_el = flatten_reference_cube(K)
    sd = flat_el.get_spatial_dimension()
    if sd not in (2, 3):
        raise ValueError("Serendipity only defined for quads and hexes")
    vs = numpy.asarray(flat_el.get_vertices(), dtype=float)
    pts = [tuple(v) for v in flat_el.get_vertices()]
    edge_pts = make_lattice(flat_el.construct_subelement(1).get_vertices(), deg, 1)
    for e in sorted(flat_el.get_topology()[1]):
        to_cell = flat_el.get_entity_transform(1, e)
        pts.extend(tuple(to_cell(p)) for p in edge_pts)

    def triangle_lattice(corners):
        d0, d1 = (corners[1] - corners[0]) / (deg - 2), (corners[2] - corners[0]) / (deg - 2)
        return [tuple(corners[0] + d0 * i + d1 * j) for i in range(1, deg - 2) for j in range(1, deg - 1 - i)]

    if deg > 3:
        if sd == 2:
            pts.extend(triangle_lattice(vs))
        else:
            face_pts = triangle_lattice(numpy.asarray(flat_el.construct_subelement(2).get_vertices(), dtype=float))
            for f in sorted(flat_el.get_topology()[2]):
                to_cell = flat_el.get_entity_transform(2, f)
                pts.extend(tuple(to_cell(p)) for p in face_pts)
    if sd == 3 and deg > 5:
        step = numpy.eye(3) / (deg - 4)
        pts.extend(tuple(vs[0] + step[0] * i + step[1] * j + step[2] * k)
                   for i in range(1, deg - 4) for j in range(1, deg - 3 - i) for k in range(1, deg - 2 - i - j))
    return pts
