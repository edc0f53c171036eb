"""Brezzi-Douglas-Marini elements on quadrilaterals (FIAT/brezzi_douglas_marini_cube.py): BDMCE (H(curl)) and its rotation
BDMCF (H(div)).  The bases are the term tables of sforms.py, evaluated by the HIP kernel of csrc/sforms.hpp."""
from .sforms import SFormElement


class BrezziDouglasMariniCube(SFormElement):
    """The Brezzi-Douglas-Marini element on quadrilateral cells (FIAT/brezzi_douglas_marini_cube.py:37-137)."""

    _hex = False

    def __init__(self, ref_el, degree):
        if degree < 1:
            raise Exception("BDMc_k elements only valid for k >= 1")
        super().__init__(ref_el, degree)


class BrezziDouglasMariniCubeEdge(BrezziDouglasMariniCube):
    """The H(curl) element BDMCE_degree (FIAT/brezzi_douglas_marini_cube.py:216-229)."""

    _family = "BDMCE"
    _mapping_name = "covariant piola"


class BrezziDouglasMariniCubeFace(BrezziDouglasMariniCube):
    """The H(div) element BDMCF_degree: (a0, a1) -> (-a1, a0) of BDMCE (FIAT/brezzi_douglas_marini_cube.py:232-248)."""

    _family = "BDMCF"
    _mapping_name = "contravariant piola"
