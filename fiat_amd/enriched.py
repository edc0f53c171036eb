"""EnrichedElement (FIAT/enriched.py): the dofs of several elements on one cell, concatenated.

Construction checks and metadata as the reference (:26-76): the elements share the reference element, the mapping and the
value shape; order, form degree and degree are maxima (the form degree None if any element has none); entity dofs and dual
nodes are concatenated in order.  Tabulation (the reference's :88-112 fills the rows of each summand in turn) runs through the
composition walk of hdivcurl.py: the fused H(div) / H(curl) kernel where the summands are blocks of one quadrilateral /
hexahedral family, else one placement pass per leaf into the output."""
from itertools import chain

import numpy

from . import runtime
from .polynomial_set_util import mis


def concatenate_entity_dofs(ref_el, elements):
    """{dim: {entity: dofs}} of the concatenated dofs of ``elements`` (FIAT/mixed.py:97-109)."""
    entity_dofs = {dim: {i: [] for i in entities} for dim, entities in ref_el.get_topology().items()}
    offsets = numpy.cumsum([0] + [e.space_dimension() for e in elements], dtype=int)
    for i, d in enumerate(e.entity_dofs() for e in elements):
        for dim, dofs in d.items():
            for ent, off in dofs.items():
                entity_dofs[dim][ent] += [int(offsets[i]) + int(x) for x in off]
    return entity_dofs


def _dimension_total(dims):
    return sum(_dimension_total(d) for d in dims) if isinstance(dims, tuple) else dims


def point_columns(ref_el, entity):
    """Coordinates per point of ``tabulate(..., entity=)``: the cell's, or the sub-entity's (product entities: their sum)."""
    if entity is None:
        return ref_el.get_spatial_dimension()
    return _dimension_total(entity[0])


def tables_to_dict(element, order, points, entity):
    """FIAT's {alpha: (ndof, [vdim,] npts)} from one batched tabulation of ``points`` on the device."""
    ref_el = element.get_reference_element()
    cols = point_columns(ref_el, entity)
    pts = numpy.asarray(points, dtype=float).reshape(-1, cols)
    host = runtime.fetch(element.tabulate_batch(order, pts[None], entity=entity))[0]
    sd = ref_el.get_spatial_dimension()
    keys = [a for k in range(order + 1) for a in mis(sd, k)]
    return {a: numpy.ascontiguousarray(host[t]) for t, a in enumerate(keys)}


class EnrichedElement:
    """The dofs of ``elements``, concatenated (FIAT/enriched.py:19-118)."""

    def __init__(self, *elements):
        if len(set(e.get_reference_element() for e in elements)) > 1:
            raise ValueError("Elements must be defined on the same reference element")
        if len(set(m for e in elements for m in e.mapping())) > 1:
            raise ValueError("Elements must have same mapping")
        if len(set(e.value_shape() for e in elements)) > 1:
            raise ValueError("Elements must have the same value shape")
        self.order = max(e.get_order() for e in elements)
        if any(e.get_formdegree() is None for e in elements):
            self.formdegree = None
        else:
            self.formdegree = max(e.get_formdegree() for e in elements)
        self.ref_el = elements[0].get_reference_element()
        self._mapping, = set(m for e in elements for m in e.mapping())
        self.entity_ids = concatenate_entity_dofs(self.ref_el, elements)
        self.nodes = list(chain.from_iterable(e.dual_basis() for e in elements))
        self.polydegree = max(e.degree() for e in elements)
        self._elements = tuple(elements)

    def elements(self):
        return self._elements

    def get_reference_element(self):
        return self.ref_el

    def get_order(self):
        return self.order

    def get_formdegree(self):
        return self.formdegree

    def degree(self):
        return self.polydegree

    def space_dimension(self):
        return sum(e.space_dimension() for e in self._elements)

    def value_shape(self):
        result, = set(e.value_shape() for e in self._elements)
        return result

    def mapping(self):
        return [self._mapping] * self.space_dimension()

    def entity_dofs(self):
        return self.entity_ids

    def dual_basis(self):
        return self.nodes

    def is_nodal(self):
        return False

    def get_nodal_basis(self):
        raise NotImplementedError("get_nodal_basis not implemented")

    def get_coeffs(self):
        raise NotImplementedError("get_coeffs not implemented")

    def dmats(self):
        raise NotImplementedError("dmats not implemented")

    def get_num_members(self, arg):
        raise NotImplementedError("get_num_members not implemented")

    def tabulate_batch(self, order, points, out=None, stream=None, grid=False, entity=None):
        """points (nreq, npts, sd) -> (nreq, ntab, ndof, [vdim,] npts) on the device (hdivcurl.tabulate_composite)."""
        from .hdivcurl import tabulate_composite
        return tabulate_composite(self, order, points, out=out, stream=stream, grid=grid, entity=entity)

    def tabulate(self, order, points, entity=None):
        """{alpha: (ndof, [vdim,] npts)} for all derivative multi-indices up to ``order``."""
        return tables_to_dict(self, order, points, entity)
