"""Trimmed serendipity H(curl) elements (FIAT/SminusCurl.py).  The bases are the term tables of sforms.py, evaluated by the
HIP kernel of csrc/sforms.hpp."""
from .sforms import SFormElement


class TrimmedSerendipityCurl(SFormElement):
    """S^-_degree Lambda^1 on quadrilaterals (degrees 1-6) and hexahedra (degrees 1-5; FIAT/SminusCurl.py:27-195)."""

    _family = "SminusCurl"
    _mapping_name = "covariant piola"
