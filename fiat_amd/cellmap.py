"""Tabulation on physical quadrilaterals and hexahedra through the multilinear (Q1) map.

The families on quadrilaterals and hexahedra live on axis-aligned boxes; their ``tabulate_batch`` has no ``verts`` (a bilinear
cell is no affine image of the box).  ``tabulate_on_cells`` is that step: per request the images ``corners`` of the box's
vertices define

    xi_d = (X_d - lo_d) / (hi_d - lo_d),   x(X) = sum_i N_i(xi) corners[i],   N_i = prod_d (bit_d(i) ? xi_d : 1 - xi_d),
    J_ad = dx_a / dX_d,   G = J^-1,

vertex i in the order of ``get_vertices()`` of the flattened cell (the last coordinate fastest).  Table 0 of the result holds
values, table 1 + d the derivative with respect to the PHYSICAL coordinate x_d: component by component
``sum_e d_e Phi G_ed`` without a push-forward (or for the affine mapping); with ``pushforward`` the Piola image
``phi = M Phi`` (M = G^T covariant, J / det J contravariant, signed determinant) and the full gradient of the mapped field,
``sum_e G_ed (d_e M Phi + M d_e Phi)``: on a cell that is no parallelogram d_e M does not vanish.

Two routes: products of 1-D Lagrange factors with the same node count <= 5 run on a fused kernel that
writes the physical tables directly (fx_cellmap_tensor_batch); everything else tabulates on its own box with its own kernel
and runs one general pass in place over the result (fx_cellmap_apply)."""
import contextlib
import inspect

import numpy

from . import runtime
from .reference_element import LINE, Hypercube, TensorProductCell, flatten_reference_cube
from .tensor_product import FlattenedDimensions, TensorProductElement

MAX_ORDER = 1                      # csrc/cellmap.hpp CM_MAXORDER
FUSED_NODES = (2, 5)               # csrc/cellmap.hpp CM_MINNN, CM_MAXNN
_MAPPINGS = {"affine": 0, "covariant piola": 1, "contravariant piola": 2}      # include/fiat_amd.h FX_MAP_*


def _intervals_only(cell):
    if isinstance(cell, TensorProductCell):
        return all(_intervals_only(c) for c in cell.cells)
    return isinstance(cell, Hypercube) or cell.get_shape() == LINE


def box_of(cell):
    """(sd, lo, hi) of a reference cell whose flattened form is an axis-aligned box of dimension 2 or 3 with vertices in
    lexicographic order; NotImplementedError with the reason for every other cell."""
    sd = cell.get_spatial_dimension()
    if not isinstance(cell, (TensorProductCell, Hypercube)):
        if cell.is_simplex() and sd >= 2:
            raise NotImplementedError("simplices are affine images of their reference cell: use tabulate_batch(verts=) "
                                      "(tabulate_on_cells maps quadrilaterals and hexahedra)")
        raise NotImplementedError(f"tabulate_on_cells maps quadrilaterals and hexahedra, not cells of dimension {sd}")
    if not _intervals_only(cell):
        raise NotImplementedError("prisms have no multilinear cell map here (quadrilaterals and hexahedra only)")
    if sd not in (2, 3):
        raise NotImplementedError(f"tabulate_on_cells maps quadrilaterals and hexahedra, not cells of dimension {sd}")
    verts = numpy.asarray(flatten_reference_cube(cell).get_vertices(), dtype=numpy.float64)
    lo, hi = verts.min(0), verts.max(0)
    bits = numpy.array([[(i >> (sd - 1 - d)) & 1 for d in range(sd)] for i in range(2 ** sd)])
    if verts.shape != (2 ** sd, sd) or not numpy.array_equal(verts, numpy.where(bits == 1, hi, lo)) or not (hi > lo).all():
        raise NotImplementedError("the element's own cell is no axis-aligned box with vertices in lexicographic order")
    return sd, numpy.ascontiguousarray(lo), numpy.ascontiguousarray(hi)


def _fused_lines(element):
    """The 1-D Lagrange factors of a scalar product element, or None."""
    while isinstance(element, FlattenedDimensions):
        element = element.element
    return element._lines if isinstance(element, TensorProductElement) else None


def fused_refusal(element):
    """None where the fused kernel applies to ``element``, else the reason it does not."""
    lines = _fused_lines(element)
    if lines is None:
        return "no product of scalar 1-D Lagrange factors"
    counts = sorted({f.space_dimension() for f in lines})
    if len(counts) != 1:
        return f"factors of unequal node counts {counts}"
    if not FUSED_NODES[0] <= counts[0] <= FUSED_NODES[1]:
        return f"factors of {counts[0]} nodes (the kernel has {FUSED_NODES[0]}..{FUSED_NODES[1]})"
    return None


def _nodes(element):
    return numpy.ascontiguousarray([f.get_nodal_basis().get_expansion_set().x for f in _fused_lines(element)], dtype=numpy.float64)


def _accepts_grid(element):
    params = inspect.signature(element.tabulate_batch).parameters
    return "grid" in params or any(p.kind is inspect.Parameter.VAR_KEYWORD for p in params.values())


def _mapping(element, pushforward):
    """FX_MAP_* code of the pass; the double Piola maps are refused."""
    name = element.mapping()[0] if pushforward else "affine"
    if name not in _MAPPINGS:
        raise NotImplementedError(f"the {name} map has no multilinear form here (affine and the single Piola maps)")
    return _MAPPINGS[name]


def _plan(element, order, pushforward, grid):
    """Validation that needs no shapes: (sd, lo, hi, mapping code, value shape)."""
    sd, lo, hi = box_of(element.get_reference_element())
    order = int(order)
    if order < 0:
        raise ValueError("negative derivative order")
    if order > MAX_ORDER:
        raise NotImplementedError(f"derivative order {order} > {MAX_ORDER} on a mapped cell: it needs more derivatives of the cell "
                                  "map than order 1 does")
    code = _mapping(element, pushforward)
    vshape = tuple(element.value_shape())
    if vshape not in ((), (sd,)):
        raise NotImplementedError(f"value shape {vshape}: scalars and vectors of {sd} components")
    if code != 0 and vshape != (sd,):
        raise ValueError("a Piola map needs a vector-valued element")
    if grid and not _accepts_grid(element):
        raise NotImplementedError(f"{type(element).__name__}.tabulate_batch takes no grid input")
    return sd, lo, hi, code, vshape


def _route(element, route):
    """Why the fused kernel is not taken, or None where it is; called after the cell, order and mapping are validated, so a
    simplex, prism or interval gets its own refusal whatever the route."""
    why = fused_refusal(element) if route != "general" else "route='general'"
    if route == "fused" and why is not None:
        raise NotImplementedError(f"the fused cell-map kernel does not apply: {why}")
    return why


def kernel(element, order, npts, pushforward=False, grid=False):
    """What ``tabulate_on_cells`` runs for a request shape (host only): ``"fused: fxk::cellmap_tensor_kernel<sd,nn,order,grid>
    image|stream P=<requests per item>"`` or ``"general: <Element>.tabulate_batch + fxk::cellmap_apply_kernel<sd,order,mapping>
    <map> P=<p> (<why not fused>)"``; with ``grid`` npts is the number of 1-D coordinates per direction."""
    sd, lo, hi, code, vshape = _plan(element, order, pushforward, grid)
    why = fused_refusal(element)
    if why is None:
        return "fused: " + runtime.cellmap_kernel(sd, _fused_lines(element)[0].space_dimension(), 0, order, 0, 1, npts, grid)
    total = int(npts) ** sd if grid else int(npts)
    return (f"general: {type(element).__name__}.tabulate_batch + "
            + runtime.cellmap_kernel(sd, 0, code, order, element.space_dimension(), sd if vshape else 1, total) + f" ({why})")


def _shapes(points, corners, sd, grid):
    import torch
    pshape = tuple(points.shape) if hasattr(points, "shape") else numpy.shape(points)
    if grid:
        if len(pshape) != 3 or pshape[1] != sd:
            raise ValueError(f"grid coordinates must have shape (nreq, {sd}, q), got {pshape}")
        nreq, npts = int(pshape[0]), int(pshape[2]) ** sd
    else:
        if len(pshape) != 3 or pshape[2] != sd:
            raise ValueError(f"points must have shape (nreq, npts, {sd}), got {pshape}")
        nreq, npts = int(pshape[0]), int(pshape[1])
    cshape = tuple(corners.shape) if hasattr(corners, "shape") else numpy.shape(corners)
    if cshape != (nreq, 2 ** sd, sd):
        raise ValueError(f"corners must have shape ({nreq}, {2 ** sd}, {sd}), got {cshape}")
    for name, arr in (("points", points), ("corners", corners)):
        dtype = arr.dtype if isinstance(arr, torch.Tensor) else numpy.asarray(arr).dtype
        if dtype != (torch.float64 if isinstance(arr, torch.Tensor) else numpy.float64):
            raise ValueError(f"{name} must be float64, got {dtype}")
    return nreq, npts


def tabulate_on_cells(element, order, points, corners, out=None, stream=None, pushforward=False, grid=False, *, route=None):
    """``element`` on per-request physical quadrilaterals / hexahedra: points (nreq, npts, sd) in the element's own reference
    coordinates (``grid=True``: per-request 1-D coordinates (nreq, sd, q) of a tensor grid, points row-major), corners
    (nreq, 2**sd, sd) the images of the cell's vertices in the order of ``get_vertices()`` of the flattened cell (float64, host
    or device) -> device tensor (nreq, ntab, ndof, *value_shape, npts), ntab = 1 + sd * [order >= 1], tables in mis() order,
    table 1 + d the derivative with respect to the physical x_d (the module docstring has the formulas).

    ``route=None`` takes the fused kernel where it applies (scalar products of 1-D Lagrange factors with one node count
    <= 5) and otherwise the general route, the element's own ``tabulate_batch`` followed by one pass in place;
    ``route="general"`` forces that, ``route="fused"`` the kernel (NotImplementedError with the reason where it does not apply).
    Order >= 2, the double Piola maps, prisms, simplices and intervals raise NotImplementedError; everything else is validated
    before anything is launched (ValueError).  A cell whose map is singular at a point gives non-finite entries there;
    nothing inspects the cells.  The work is ordered on ``stream``."""
    import torch
    if route not in (None, "fused", "general"):
        raise ValueError(f"unknown route {route!r}")
    order = int(order)
    sd, lo, hi, code, vshape = _plan(element, order, pushforward, grid)
    why = _route(element, route)
    nreq, npts = _shapes(points, corners, sd, grid)
    ndof = element.space_dimension()
    ntab = 1 + sd * order
    vdim = sd if vshape else 1
    shape = (nreq, ntab, ndof) + vshape + (npts,)
    ctx = runtime.Context.get()
    if out is not None and (not isinstance(out, torch.Tensor) or tuple(out.shape) != shape or out.dtype != torch.float64
                            or not out.is_contiguous() or out.device != ctx.device):
        raise ValueError(f"out must be a contiguous float64 device tensor of shape {shape}")
    if ntab * ndof * vdim * npts >= 2 ** 31 or nreq * ntab * ndof * vdim * npts >= 2 ** 62:
        raise ValueError("the request or the batch does not fit the index arithmetic of the kernels")
    points = runtime._as_device(points, ctx)
    corners = runtime._as_device(corners, ctx)
    if why is None:
        if out is None:
            out = torch.empty(shape, dtype=torch.float64, device=ctx.device)
        return runtime.cellmap_tensor_batch(sd, _nodes(element), lo, hi, order, points, corners, out, stream=stream, grid=grid, ctx=ctx)
    kwargs = {"grid": True} if grid else {}
    tab = element.tabulate_batch(order, points, out=out, stream=stream, **kwargs)
    if tuple(tab.shape) != shape:
        raise ValueError(f"{type(element).__name__}.tabulate_batch returned {tuple(tab.shape)}, expected {shape}")
    if grid:
        # the pass reads explicit points: row-major (j0, j1[, j2]) over the 1-D coordinates
        with (torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()):
            q = points.shape[2]
            idx = torch.cartesian_prod(*[torch.arange(q, device=ctx.device)] * sd)
            points = torch.stack([points[:, d, idx[:, d]] for d in range(sd)], -1).contiguous()
    apart = out is not None and out.data_ptr() != tab.data_ptr()       # (an element that did not write into ``out`` itself)
    return runtime.cellmap_apply(sd, code, order, lo, hi, points, corners, tab, out=out if apart else None, stream=stream, ctx=ctx)


def cell_geometry_batch(cell, points, corners, out=None, stream=None):
    """The Q1 map of per-request cells at points: ``cell`` a reference quadrilateral / hexahedron (or a product of
    intervals), points (nreq, npts, sd) in its coordinates, corners (nreq, 2**sd, sd) -> device tensors
    ``(x (nreq, npts, sd), J (nreq, npts, sd, sd), detJ (nreq, npts))``, J[..., a, d] = dx_a / dX_d, detJ signed: what a
    consumer multiplies into quadrature weights.  ``out``: a triple of such tensors to write."""
    import torch
    sd, lo, hi = box_of(cell)
    nreq, npts = _shapes(points, corners, sd, False)
    ctx = runtime.Context.get()
    shapes = ((nreq, npts, sd), (nreq, npts, sd, sd), (nreq, npts))
    if out is None:
        out = tuple(torch.empty(s, dtype=torch.float64, device=ctx.device) for s in shapes)
    else:
        out = tuple(out)
        if len(out) != 3 or any(not isinstance(t, torch.Tensor) or tuple(t.shape) != s or t.dtype != torch.float64
                                or not t.is_contiguous() or t.device != ctx.device for t, s in zip(out, shapes)):
            raise ValueError(f"out must be three contiguous float64 device tensors of shapes {shapes}")
    points = runtime._as_device(points, ctx)
    corners = runtime._as_device(corners, ctx)
    runtime.cellmap_geometry(sd, lo, hi, points, corners, *out, stream=stream, ctx=ctx)
    return out
