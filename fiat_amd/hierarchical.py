"""The Legendre and IntegratedLegendre elements (FIAT/hierarchical.py).

``Legendre``: the discontinuous space P_k whose degrees of freedom are the mean values of f times the orthonormal polynomials
of the cell.  Its nodal basis is therefore the orthogonal basis itself, normalised to unit mean square -- sqrt(2p + 1) P_p on
the interval.  Here it is one dof block (dof_layout.py) over ``ONPolynomialSet``: the test functions are the orthonormal set
in its "L2 piola" scaling (divided by the cell's volume), tabulated once at a rule exact for the product, and every cell of
the complex gets them as integral moments on its averaged copy of that rule.  Construction (Vandermonde solve) and tabulation
are the inherited device paths; there is no kernel of its own.  Degree 0 is P0.  The H(div) trace element takes it as facet
element for its "integral" variants (hdiv_trace.py).

``IntegratedLegendre``: the continuous hierarchical H1 basis, P_k over the bubble-variant expansion set.  Its degrees of
freedom are, entity by entity, integral moments against the L2-duals of that entity's interior C0 members, so its nodal basis
is the C0 hierarchy itself: the coefficient matrix is diagonal, with one value per entity dimension.  Construction is the
inherited one.  Tabulation of degree 1-6 with order 0-2 on a UFC simplex does not use the coefficients: the HIP kernel of
csrc/hierarchical.hpp (fx_hier_tabulate_batch, include/fiat_amd_hier.h) runs the recurrence, applies the C0 corrections and
scales every row by the value of its entity dimension.  Everything else -- per-request cells, degree >= 7, order >= 3 --
takes the general route, the contraction kernels of the nodal coefficients."""
import numpy

from . import runtime
from .check_format_variant import check_format_variant, parse_quadrature_scheme
from .dof_layout import DofLayout
from .dual_set import DualSet
from .finite_element import CiarletElement
from .functional import IntegralMoment
from .P0 import P0
from .polynomial_set import ONPolynomialSet, make_bubbles, mis
from .quadrature import FacetQuadratureRule
from .reference_element import UFCInterval, UFCTetrahedron, UFCTriangle, make_affine_mapping, symmetric_simplex

HIER_KERNEL_MAXK, HIER_KERNEL_MAXORDER = 6, 2     # the compile-time instances of csrc/hierarchical.hpp


class LegendreDual(DualSet):
    """Mean values against the orthonormal polynomials of degree <= ``degree`` on every sub-entity of codimension ``codim``
    (the cells themselves by default); the rule is exact to ``degree + interpolant_deg``."""

    def __init__(self, ref_el, degree, codim=0, interpolant_deg=None, quad_scheme=None):
        layout = DofLayout(ref_el)
        dim = layout.sd - codim
        shape = ref_el.construct_subelement(dim)
        rule = parse_quadrature_scheme(shape, degree + (degree if interpolant_deg is None else interpolant_deg), quad_scheme)
        tests = ONPolynomialSet(shape, degree, scale="L2 piola").tabulate(rule.get_points())[(0,) * dim]
        for entity in layout.entities(dim):
            mean = FacetQuadratureRule(ref_el, dim, entity, rule, avg=True)      # reference weights: an average, not an integral
            layout.place(dim, entity, (IntegralMoment(ref_el, mean, test) for test in tests))
        super().__init__(*layout.parts())


class Legendre(CiarletElement):
    """``Legendre(ref_el, degree, variant=None, quad_scheme=None)``; ``variant``: "integral" or "integral(q)" (q extra degrees
    of exactness of the rule), optionally with a macro-element splitting."""

    def __new__(cls, ref_el, degree, variant=None, quad_scheme=None):
        if degree == 0:
            splitting, _, exactness = check_format_variant(variant, degree)
            if splitting is None and exactness == 0:
                return P0(ref_el)
        return super().__new__(cls)

    def __init__(self, ref_el, degree, variant=None, quad_scheme=None):
        splitting, _, exactness = check_format_variant(variant, degree)
        cell = ref_el if splitting is None else splitting(ref_el)
        dual = LegendreDual(cell, degree, interpolant_deg=exactness, quad_scheme=quad_scheme)
        super().__init__(ONPolynomialSet(cell, degree), dual, degree, formdegree=cell.get_spatial_dimension())


def make_dual_bubbles(ref_el, degree, codim=0, interpolant_deg=None, quad_scheme=None, scale="orthonormal"):
    """(rule, tests): the L2-duals of the C0 members that belong to the entities of co-dimension ``codim`` of ``ref_el``,
    tabulated at a rule exact to ``degree + interpolant_deg`` -- the inverse mass matrix of the whole hierarchy applied to its
    table, rows of those members.  On a point the rule has no scheme and degree 0."""
    if ref_el.get_spatial_dimension() == 0:
        quad_scheme = None
        degree = 0
    if interpolant_deg is None:
        interpolant_deg = degree
    rule = parse_quadrature_scheme(ref_el, degree + interpolant_deg, quad_scheme)
    bubbles = make_bubbles(ref_el, degree, codim=codim, scale=scale)
    table = numpy.asarray(bubbles.get_expansion_set().tabulate(degree, rule.get_points()), dtype=float)
    mass = (table * rule.get_weights()) @ table.T
    return rule, bubbles.get_coeffs() @ numpy.linalg.solve(mass, table)


class IntegratedLegendreDual(DualSet):
    """For every entity dimension ``dim < degree``: moments against the L2-duals of the interior C0 members of
    ``symmetric_simplex(dim)``, placed on every entity of that dimension with its averaged rule."""

    def __init__(self, ref_el, degree, interpolant_deg=None, quad_scheme=None):
        layout = DofLayout(ref_el)
        if interpolant_deg is None:
            interpolant_deg = degree
        for dim in sorted(layout.topology):
            if degree <= dim:
                continue
            rule, tests = make_dual_bubbles(symmetric_simplex(dim), degree, interpolant_deg=interpolant_deg,
                                            quad_scheme=quad_scheme)
            for entity in layout.entities(dim):
                mean = FacetQuadratureRule(ref_el, dim, entity, rule, avg=True)
                layout.place(dim, entity, (IntegralMoment(ref_el, mean, test) for test in tests))
        super().__init__(*layout.parts())


class IntegratedLegendre(CiarletElement):
    """``IntegratedLegendre(ref_el, degree, variant=None, quad_scheme=None)``; ``variant`` as for ``Legendre``."""

    def __init__(self, ref_el, degree, variant=None, quad_scheme=None):
        splitting, _, exactness = check_format_variant(variant, degree)
        cell = ref_el if splitting is None else splitting(ref_el)
        if degree < 1:
            raise ValueError(f"{type(self).__name__} elements only valid for k >= 1")
        dual = IntegratedLegendreDual(cell, degree, interpolant_deg=exactness, quad_scheme=quad_scheme)
        super().__init__(ONPolynomialSet(cell, degree, variant="bubble"), dual, degree, formdegree=0)
        sd = cell.get_spatial_dimension()
        ufc = {1: UFCInterval, 2: UFCTriangle, 3: UFCTetrahedron}.get(sd)
        self._hier_cell = (splitting is None and ufc is not None and not cell.is_macrocell()
                           and numpy.array_equal(numpy.asarray(cell.get_vertices(), dtype=float),
                                                 numpy.asarray(ufc().get_vertices(), dtype=float)))
        if self._hier_cell:
            # the cell onto the (-1, 1)^sd simplex, and the diagonal of the coefficients per entity dimension
            A, b = make_affine_mapping(cell.get_vertices(), tuple(tuple(1.0 if i == j + 1 else -1.0 for j in range(sd))
                                                                   for i in range(sd + 1)))
            self._A = numpy.ascontiguousarray(A, dtype=float)
            self._b = numpy.ascontiguousarray(b, dtype=float)
            diag = numpy.diag(numpy.asarray(self.get_coeffs(), dtype=float))
            ids = self.entity_dofs()
            self._scales = numpy.ones(4)
            for dim in ids:
                dofs = [i for entity in ids[dim] for i in ids[dim][entity]]
                if dofs:
                    self._scales[dim] = float(numpy.median(diag[dofs]))

    def _direct(self, order, verts=None):
        return (self._hier_cell and verts is None and 1 <= self.order <= HIER_KERNEL_MAXK
                and 0 <= order <= HIER_KERNEL_MAXORDER)

    def kernel(self, order, npts, nreq=1):
        """Kernel instance and output route of a request shape: ``"fxk::hier_kernel<sd,degree,order> image|stream P=<p>"``
        (fx_hier_kernel), or the string of the general route beyond the direct kernel's instances: its kernel
        (fx_plan_kernel) for orders 0-2, the differentiation-matrix route above."""
        if self._direct(order):
            return runtime.hier_kernel(self.ref_el.get_spatial_dimension(), self.order, order, npts)
        if order > 2:   # (fx_plan_kernel names the kernels of orders 0-2 only)
            return "general route: differentiation matrices (fx_tabulate_batch, order > 2)"
        return self.device_polyset().kernel_name(order, nreq, npts)

    def tabulate(self, order, points, entity=None):
        """{alpha: (ndof, npts)} of all derivatives up to ``order``; ``entity=(dim, id)``: the points are in the coordinates
        of that sub-entity of the element's cell."""
        points = numpy.asarray(points, dtype=float)
        sd = self.ref_el.get_spatial_dimension()
        pd = sd if entity is None else entity[0]
        if points.ndim != 2 or pd == 0 or points.shape[1] != pd:
            return super().tabulate(order, points, entity)       # (single points and vertex entities: the inherited forms)
        out = runtime.fetch(self.tabulate_batch(order, points[None], entity=entity))[0]
        keys = [a for k in range(order + 1) for a in mis(sd, k)]
        return {a: numpy.ascontiguousarray(out[t]) for t, a in enumerate(keys)}

    def tabulate_batch(self, order, points, verts=None, out=None, stream=None, pushforward=False, entity=None, *, route=None):
        """points (nreq, npts, sd) -> device tensor (nreq, ntab, ndof, npts), tables in mis() order.  ``entity=(dim, id)``:
        points (nreq, npts, dim) on that sub-entity, mapped into the cell on the device (fx_map_points) before the same
        kernel runs.  Degree 1-6 with order 0-2 on the element's own UFC cell runs the direct kernel
        (fx_hier_tabulate_batch); per-request cells (``verts``), everything beyond those instances, and ``route="general"``
        (for tests and benchmarks) take the inherited contraction of the nodal coefficients.  ``pushforward`` changes
        nothing on the direct route (the mapping is affine and the cell is the element's own)."""
        if route not in (None, "general"):
            raise ValueError(f"unknown route {route!r}")
        if route == "general" or not self._direct(order, verts):
            return super().tabulate_batch(order, points, verts=verts, out=out, stream=stream, pushforward=pushforward,
                                          entity=entity)
        emap = self.entity_map(entity)
        if emap is not None:
            points = runtime.map_points(*emap, points, stream=stream)
        sd = self.ref_el.get_spatial_dimension()
        return runtime.hier_tabulate_batch(sd, self.order, int(order), self._scales, self._A, self._b, points, out=out,
                                           stream=stream)
