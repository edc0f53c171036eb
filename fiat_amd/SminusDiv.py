"""Trimmed serendipity H(div) elements (FIAT/SminusDiv.py).  The bases are the term tables of sforms.py, evaluated by the
HIP kernel of csrc/sforms.hpp."""
from .sforms import SFormElement


class TrimmedSerendipityDiv(SFormElement):
    """S^-_degree Lambda^(d-1) on quadrilaterals (degrees 1-6) and hexahedra (degrees 1-5; FIAT/SminusDiv.py:27-177)."""

    _family = "SminusDiv"
    _mapping_name = "contravariant piola"
