"""Trimmed serendipity edge and face elements (FIAT/Sminus.py).  The bases are the term tables of sforms.py, evaluated by
the HIP kernel of csrc/sforms.hpp."""
from .sforms import SFormElement


class TrimmedSerendipityEdge(SFormElement):
    """S^-_degree Lambda^1 on quadrilaterals (degrees 1-6) and hexahedra (degrees 1-3; FIAT/Sminus.py:408-459)."""

    _family = "SminusE"
    _mapping_name = "covariant piola"


class TrimmedSerendipityFace(SFormElement):
    """The rotation of TrimmedSerendipityEdge on quadrilaterals (FIAT/Sminus.py:462-488)."""

    _family = "SminusF"
    _mapping_name = "contravariant piola"
    _hex = False
