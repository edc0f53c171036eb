"""Hdiv / Hcurl (FIAT/hdivcurl.py:13-254) and the tabulation of their compositions with EnrichedElement and
FlattenedDimensions.

Hdiv(e) / Hcurl(e) turn a product of two elements into a vector field: the product's table moves into components of the
result, with a sign (both factors affine), as a block of components (the factor of the same Piola map), or rotated by 90
degrees (a factor of the other Piola map on a triangle).  Tabulation walks a composition down to its LEAVES -- the products
and elements that are tabulated -- each with its dof offset in the final table and, per output component, the source
component (or none) and a sign, and takes one of two routes:

- fused: RTCF / RTCE / NCF / NCE as Firedrake composes them, and their summands -- one block per component, each the signed
  row-major product of C (K+1 nodes) and D (K nodes) 1-D Lagrange factors -- on fx_hdivcurl_tabulate_batch, one launch;
- general: every leaf is tabulated by its own routes (TensorProductElement.tabulate_batch, a Ciarlet element's kernels) and
  placed into the output by fx_table_place_batch, all components of its rows, zeros included (one pass per leaf)."""
import numpy
import torch

from . import functional, runtime
from .enriched import EnrichedElement, point_columns
from .reference_element import LINE
from .tensor_product import FlattenedDimensions, TensorProductElement, _is_line_lagrange

_SAME = {"div": "contravariant piola", "curl": "covariant piola"}


class HdivCurlElement(TensorProductElement):
    """The product of A and B as the vector field Hdiv / Hcurl make of it; still a TensorProductElement, as in the
    reference (which patches a copy of the product)."""

    def __init__(self, A, B, kind):
        super().__init__(A, B)
        self.kind = kind
        self._oldmapping = self._mapping
        self._mapping = _SAME[kind]
        self.formdegree = A.get_formdegree() + B.get_formdegree()
        self._inner = TensorProductElement(A, B)      # the product whose table is placed
        self._leaves = None

    def value_shape(self):
        return (self.ref_el.get_spatial_dimension(),)

    def dual_basis(self):
        """The product's nodes; with an affine product every point evaluation becomes an undefined functional
        (FIAT/hdivcurl.py:118-128)."""
        nodes = self._inner.dual_basis()
        if self._oldmapping == "affine":
            nodes = [functional.Functional(None, None, None, {}, "Undefined")
                     if isinstance(n, functional.PointEvaluation) else n for n in nodes]
        return nodes

    def leaves(self):
        if self._leaves is None:
            self._leaves = self._make_leaves()
        return self._leaves

    def _make_leaves(self):
        sd = self.ref_el.get_spatial_dimension()
        A, B, old, name = self.A, self.B, self._oldmapping, "Hdiv" if self.kind == "div" else "Hcurl"
        comp, sign = [-1] * sd, [0] * sd
        if old == "affine":
            # Hdiv: the 0-form factor's table, (-x, 0, ...) from A or (..., 0, x) from B; Hcurl: the 1-form factor's, no sign
            form = 0 if self.kind == "div" else 1
            if A.get_formdegree() == form:
                c, s = 0, (-1 if self.kind == "div" else 1)
            elif B.get_formdegree() == form:
                c, s = sd - 1, 1
            else:
                raise Exception(f"{name} affine/affine form degrees broke")
            comp[c], sign[c] = 0, s
            return [(self._inner, 0, tuple(comp), tuple(sign))]
        Asd = A.get_reference_element().get_spatial_dimension()
        if old == self._mapping:
            if A.mapping()[0] == old:      # (x1, ..., xn, 0, ...): a composite A is walked, its leaves times B
                if isinstance(A, (EnrichedElement, HdivCurlElement, FlattenedDimensions)):
                    nb = B.space_dimension()
                    return [(TensorProductElement(leaf, B), off * nb, tuple(lc) + (-1,) * (sd - len(lc)), tuple(ls) + (0,) * (sd - len(ls)))
                            for leaf, off, lc, ls in leaves(A)]
                return [(self._inner, 0, tuple(range(Asd)) + (-1,) * (sd - Asd), (1,) * Asd + (0,) * (sd - Asd))]
            if B.mapping()[0] == old:      # (..., 0, x1, ..., xn)
                n = sd - Asd
                return [(self._inner, 0, (-1,) * Asd + tuple(range(n)), (0,) * Asd + (1,) * n)]
            raise ValueError(f"{name} couldn't find a sub-element with the {old} mapping")
        if A.mapping()[0] == old:
            if Asd != 2:
                raise ValueError("Must be 2d shape to automatically convert between the Piola maps")
            # Hdiv: (x2, -x1, 0, ...); Hcurl: (-x2, x1, 0, ...)
            comp[0], comp[1] = 1, 0
            sign[0], sign[1] = (1, -1) if self.kind == "div" else (-1, 1)
            return [(self._inner, 0, tuple(comp), tuple(sign))]
        if B.mapping()[0] == old:
            raise NotImplementedError(f"{name} of a product whose second factor has the {old} mapping: the reference cannot "
                                      "tabulate it either (INTEGRATION.md)")
        raise ValueError(f"{name} couldn't find a sub-element with the {old} mapping")

    def tabulate_batch(self, order, points, out=None, stream=None, grid=False, entity=None):
        """points (nreq, npts, sd) -> (nreq, ntab, ndof, sd, npts) on the device."""
        return tabulate_composite(self, order, points, out=out, stream=stream, grid=grid, entity=entity)


def _wrap(element, kind):
    if not isinstance(element, TensorProductElement):
        raise NotImplementedError
    name = "Hdiv" if kind == "div" else "Hcurl"
    if element.A.get_formdegree() is None or element.B.get_formdegree() is None:
        raise ValueError(f"form degree of sub-element was None (not set during initialisation), {name} cannot be done "
                         "without this information")
    formdegree = element.A.get_formdegree() + element.B.get_formdegree()
    want = element.get_reference_element().get_spatial_dimension() - 1 if kind == "div" else 1
    if formdegree != want:
        raise ValueError(f"Tried to use {name} on a non-{'(n-1)' if kind == 'div' else '1'}-form element")
    return HdivCurlElement(element.A, element.B, kind)


def Hdiv(element):
    """The product ``element`` as an H(div) vector field (contravariant Piola)."""
    return _wrap(element, "div")


def Hcurl(element):
    """The product ``element`` as an H(curl) vector field (covariant Piola)."""
    return _wrap(element, "curl")


def leaves(element):
    """[(leaf element, dof offset, source component per output component (-1: zero), sign per output component)]."""
    if isinstance(element, FlattenedDimensions):
        return leaves(element.element)
    if isinstance(element, EnrichedElement):
        cache = element.__dict__.setdefault("_hdc", {})
        if "leaves" not in cache:
            out, off = [], 0
            for e in element.elements():
                out += [(leaf, o + off, c, s) for leaf, o, c, s in leaves(e)]
                off += e.space_dimension()
            cache["leaves"] = out
        return cache["leaves"]
    if isinstance(element, HdivCurlElement):
        return element.leaves()
    shape = element.value_shape()
    n = int(numpy.prod(shape)) if shape else 1
    return [(element, 0, tuple(range(n)), (1,) * n)]


def _line_nodes(element):
    """The 1-D node sets of a product of scalar 1-D Lagrange factors (a P0 factor: one node at the midpoint, as
    TensorProductElement._prism_factors), left to right, or None."""
    if isinstance(element, TensorProductElement):
        if element.value_shape() != ():
            return None
        a, b = _line_nodes(element.A), _line_nodes(element.B)
        return None if a is None or b is None else a + b
    if isinstance(element, (FlattenedDimensions, EnrichedElement)):
        return None
    if element.get_reference_element().get_shape() != LINE or element.value_shape() != ():
        return None
    if _is_line_lagrange(element):
        return [numpy.asarray(element.get_nodal_basis().get_expansion_set().x, dtype=float)]
    if element.space_dimension() == 1 and element.degree() == 0:
        v = element.get_reference_element().get_vertices()
        return [numpy.array([0.5 * (v[0][0] + v[1][0])])]
    return None


def fused_descriptor(element):
    """(sd, kind, C nodes, D nodes, offsets, signs) when the fused kernel's rule describes ``element`` (one block per
    component; block c the product over the directions d of C -- K+1 nodes -- or D -- K nodes --, H(div): C where d == c,
    H(curl): D where d == c; one sign per block), else None."""
    sd = element.get_reference_element().get_spatial_dimension()
    if sd not in (2, 3) or tuple(element.value_shape()) != (sd,):
        return None
    kind = K = None
    nodes_of = {}                                   # True: C, False: D
    offsets, signs = [-1] * sd, [0] * sd
    for leaf, off, comp, sign in leaves(element):
        nz = [c for c in range(sd) if comp[c] >= 0]
        if len(nz) != 1 or comp[nz[0]] != 0:
            return None
        c = nz[0]
        nodes = _line_nodes(leaf)
        if nodes is None or len(nodes) != sd or offsets[c] >= 0 or sign[c] not in (1, -1):
            return None
        others = {len(nodes[d]) for d in range(sd) if d != c}
        if len(others) != 1:
            return None
        other, = others
        if len(nodes[c]) == other + 1:
            this = (runtime.HDIV, other)
        elif len(nodes[c]) + 1 == other:
            this = (runtime.HCURL, len(nodes[c]))
        else:
            return None
        if kind is None:
            kind, K = this
        elif this != (kind, K):
            return None
        for d in range(sd):
            is_c = (d == c) == (kind == runtime.HDIV)
            if is_c not in nodes_of:
                nodes_of[is_c] = nodes[d]
            elif not numpy.array_equal(nodes_of[is_c], nodes[d]):
                return None
        offsets[c], signs[c] = int(off), int(sign[c])
    if kind is None or len(nodes_of) != 2:
        return None
    return sd, kind, nodes_of[True], nodes_of[False], tuple(offsets), tuple(signs)


def _cache(element):
    return element.__dict__.setdefault("_hdc", {})


def tabulate_composite(element, order, points, out=None, stream=None, grid=False, entity=None):
    """Tables of a composition of Hdiv / Hcurl / EnrichedElement: the fused kernel where the element fits its rule (whole
    cell, order <= 2), else the general route."""
    ref_el = element.get_reference_element()
    cache = _cache(element)
    if "desc" not in cache:
        cache["desc"] = fused_descriptor(element)
    desc = cache["desc"]
    whole = entity is None or entity[0] == ref_el.get_dimension()
    if desc is not None and whole and order <= 2:
        sd, kind, cn, dn, offsets, signs = desc
        if "lines" not in cache:
            cache["lines"] = (runtime.LineLagrange(cn), runtime.LineLagrange(dn))
        C, D = cache["lines"]
        res = runtime.hdivcurl_tabulate_batch(sd, kind, C, D, offsets, signs, order, points, out=out, stream=stream, grid=grid)
        if res is not None:
            return res
    if grid:
        raise NotImplementedError("grid input is served on the fused H(div) / H(curl) route only")
    return tabulate_general(element, order, points, out=out, stream=stream, entity=entity)


def tabulate_general(element, order, points, out=None, stream=None, entity=None):
    """Every leaf tabulated by its own routes and placed into the output (fx_table_place_batch)."""
    ctx = runtime.Context.get()
    points = runtime._as_device(points, ctx)
    ref_el = element.get_reference_element()
    cols = point_columns(ref_el, entity)
    if points.dim() != 3 or points.shape[2] != cols:
        raise ValueError(f"points must have shape (nreq, npts, {cols}), got {tuple(points.shape)}")
    nreq, npts = int(points.shape[0]), int(points.shape[1])
    shape = (nreq, runtime.num_tables(ref_el.get_spatial_dimension(), order), element.space_dimension()) \
        + tuple(element.value_shape()) + (npts,)
    if out is None:
        out = torch.empty(shape, dtype=torch.float64, device=ctx.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float64 or not out.is_contiguous():
        raise ValueError("out has the wrong shape/dtype/layout")
    for leaf, off, comp, sign in leaves(element):
        tab = leaf.tabulate_batch(order, points, stream=stream, entity=entity)
        runtime.table_place(tab, out, off, comp, sign, ctx=ctx, stream=stream)
    return out
