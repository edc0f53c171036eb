"""The Legendre element (FIAT/hierarchical.py, ``Legendre`` and ``LegendreDual``).

Definition: the discontinuous space P_k whose degrees of freedom are the mean values of f times the orthonormal polynomials
of the cell.  Its nodal basis is therefore the orthogonal basis itself, normalised to unit mean square -- sqrt(2p + 1) P_p on
the interval.  Here it is one dof block (dof_layout.py) over ``ONPolynomialSet``: the test functions are the orthonormal set
in its "L2 piola" scaling (divided by the cell's volume), tabulated once at a rule exact for the product, and every cell of
the complex gets them as integral moments on its averaged copy of that rule.  Construction (Vandermonde solve) and tabulation
are the inherited device paths; there is no kernel of its own.  Degree 0 is P0.  The H(div) trace element takes it as facet
element for its "integral" variants (hdiv_trace.py).  ``IntegratedLegendre`` of the same reference module is not provided."""
from .check_format_variant import check_format_variant, parse_quadrature_scheme
from .dof_layout import DofLayout
from .dual_set import DualSet
from .finite_element import CiarletElement
from .functional import IntegralMoment
from .P0 import P0
from .polynomial_set import ONPolynomialSet
from .quadrature import FacetQuadratureRule


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
