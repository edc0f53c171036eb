"""FiniteElement / CiarletElement facade.

Mirrors FIAT/finite_element.py (FiniteElement :20-121, CiarletElement :124-219).
Construction assembles V = dual.to_riesz(P) . coeffs^T and solves V^T X = B on
the device (fx_vandermonde_solve_batch); tabulate() runs the HIP tabulation
kernel.  A singular Vandermonde matrix raises numpy.linalg.LinAlgError, as in the
reference (:151-156)."""
import contextlib

import numpy

from . import runtime
from .polynomial_set import PolynomialSet, mis


class FiniteElement:
    def __init__(self, ref_el, dual, order, formdegree=None, mapping="affine", ref_complex=None):
        self.order = order
        self.formdegree = formdegree
        self.ref_el = ref_el
        self.dual = dual
        self.ref_complex = ref_complex or ref_el
        self._mapping = mapping

    def get_reference_element(self):
        return self.ref_el

    def get_reference_complex(self):
        return self.ref_complex

    def get_dual_set(self):
        return self.dual

    def get_order(self):
        return self.order

    def dual_basis(self):
        return self.dual.get_nodes()

    def entity_dofs(self):
        return self.dual.get_entity_ids()

    def entity_closure_dofs(self):
        return self.dual.get_entity_closure_ids()

    def entity_permutations(self):
        return self.dual.get_entity_permutations()

    def get_formdegree(self):
        return self.formdegree

    def mapping(self):
        return [self._mapping] * self.space_dimension()

    def num_sub_elements(self):
        return 1

    def space_dimension(self):
        return len(self.get_dual_set())

    def tabulate(self, order, points, entity=None):
        raise NotImplementedError("Must be specified in the element subclass of FiniteElement.")

    @staticmethod
    def is_nodal():
        return False

    def is_macroelement(self):
        return self.ref_el is not self.ref_complex

    def evaluate_batch(self, order, points, dofs, verts=None, out=None, stream=None, pushforward=False, *, route=None):
        """``sum_i dofs[r, (j,) i] D^alpha phi_i(x_rq)`` for every request: see the module's ``evaluate_batch``."""
        return evaluate_batch(self, order, points, dofs, verts=verts, out=out, stream=stream, pushforward=pushforward,
                              route=route)

    def evaluate_kernel(self, order, npts, nrhs=1, has_verts=False, pushforward=False):
        """Kernel instance and route ``evaluate_batch`` takes for a request shape, as text: see ``evaluate_kernel``."""
        return evaluate_kernel(self, order, npts, nrhs=nrhs, has_verts=has_verts, pushforward=pushforward)


class CiarletElement(FiniteElement):
    def __init__(self, poly_set, dual, order, formdegree=None, mapping="affine", ref_complex=None):
        ref_el = dual.get_reference_element()
        ref_complex = ref_complex or poly_set.get_reference_element()
        super().__init__(ref_el, dual, order, formdegree, mapping, ref_complex)
        if len(poly_set) != len(dual):
            raise ValueError(f"Dimension of function space is {len(poly_set)}, but got {len(dual)} nodes.")

        old_coeffs = poly_set.get_coeffs()
        dualmat = dual.to_riesz(poly_set)
        shp = dualmat.shape
        A = dualmat.reshape((shp[0], -1))
        B = old_coeffs.reshape((shp[0], -1))
        X, V = runtime.vandermonde_solve_batch(A, B, return_V=True)   # LinAlgError if singular
        self.V = V.cpu().numpy()[0]
        new_coeffs = X.cpu().numpy()[0].reshape((shp[0],) + shp[1:])
        self.poly_set = PolynomialSet(poly_set.get_reference_element(), poly_set.get_degree(),
                                      poly_set.get_embedded_degree(), poly_set.get_expansion_set(), new_coeffs)
        if hasattr(poly_set.get_expansion_set(), "device_line"):
            # 1-D Lagrange primal basis: keep the specialised tabulate
            from .barycentric_interpolation import LagrangePolynomialSet
            ps = LagrangePolynomialSet.__new__(LagrangePolynomialSet)
            PolynomialSet.__init__(ps, poly_set.get_reference_element(), poly_set.get_degree(),
                                   poly_set.get_embedded_degree(), poly_set.get_expansion_set(), new_coeffs)
            self.poly_set = ps
        es = poly_set.get_expansion_set()
        self._expansion_variant = getattr(es, "variant", None)
        self._expansion_scale = es.get_scale(poly_set.get_embedded_degree())

    def degree(self):
        return self.poly_set.get_embedded_degree()

    def get_nodal_basis(self):
        return self.poly_set

    def get_coeffs(self):
        return self.poly_set.get_coeffs()

    def device_polyset(self):
        """Device-resident nodal basis for the batched API (fx_tabulate_batch)."""
        return self.poly_set.device_polyset()

    def entity_map(self, entity):
        """(M, b) of the affine map from the coordinates of the reference sub-entity ``(dim, id)`` into this
        element's cell, x = M xi + b (reference_element.py:570-609); None for the cell itself."""
        sd = self.ref_el.get_spatial_dimension()
        if entity is None or entity[0] == sd:
            if entity is not None and entity[1] != 0:
                raise ValueError("a simplex has a single cell")
            return None
        dim, number = entity
        f = self.ref_el.get_entity_transform(dim, number)
        b = numpy.asarray(f(numpy.zeros((1, dim))), dtype=float).reshape(sd)
        M = numpy.zeros((sd, dim))
        for i in range(dim):
            unit = numpy.zeros((1, dim))
            unit[0, i] = 1.0
            M[:, i] = numpy.asarray(f(unit), dtype=float).reshape(sd) - b
        return M, b

    def tabulate(self, order, points, entity=None):
        """{alpha: (ndof, *value_shape, npts)} of all derivatives up to ``order``; ``entity=(dim, id)``: the points
        are given in the coordinates of that reference sub-entity (FIAT/finite_element.py:181-197)."""
        points = numpy.asarray(points, dtype=float)
        emap = self.entity_map(entity)
        if emap is None:
            return self.poly_set.tabulate(points, order)
        sd = self.ref_el.get_spatial_dimension()
        single = points.ndim == 1 and entity[0] > 0
        npts = (len(points) if points.ndim == 2 else 1) if entity[0] == 0 else points.size // entity[0]
        dev = self.tabulate_batch(order, points.reshape(1, npts, entity[0]), entity=entity)
        out = runtime.fetch(dev)[0]
        keys = [a for k in range(order + 1) for a in mis(sd, k)]
        return {a: (numpy.ascontiguousarray(out[t][..., 0]) if single else numpy.ascontiguousarray(out[t]))
                for t, a in enumerate(keys)}

    def tabulate_batch(self, order, points, verts=None, out=None, stream=None, pushforward=False, entity=None):
        """Batched form of tabulate(): points (nreq, npts, sd) [+ per-request cell
        vertices (nreq, sd+1, sd)] -> device tensor (nreq, ntab, ndof, *value_shape, npts)
        with tables in mis() order.  ``pushforward=True`` (needs ``verts``) applies this element's
        mapping() -- affine pull-back, covariant or contravariant Piola -- so that the tables are
        the basis functions ON the physical cells.  ``entity=(dim, id)``: points (nreq, npts, dim) in the
        coordinates of that reference sub-entity, mapped into the cell on the device (fx_map_points)."""
        emap = self.entity_map(entity)
        if emap is not None:
            if verts is not None:
                raise NotImplementedError("sub-entity points with per-request cells: use tabulate_cells(..., entity=)")
            points = runtime.map_points(*emap, points, stream=stream)
        mapping = self._mapping if pushforward else None
        return self.device_polyset().tabulate_batch(order, points, verts=verts, out=out, stream=stream, mapping=mapping)

    def tabulate_cells(self, order, ref_points, verts, out=None, stream=None, entity=None):
        """The quadrature-rule case: ONE point set on this element's reference cell (or, ``entity=(dim, id)``, on one
        of its reference sub-entities: a facet rule), pushed forward (with mapping()) to the physical cells ``verts``
        (nreq, sd+1, sd) -> device tensor (nreq, ntab, ndof, *value_shape, npts).  Same result as
        ``tabulate_batch(order, F_r(ref_points), verts, pushforward=True)``."""
        emap = self.entity_map(entity)
        if emap is not None:
            ref_points = runtime.map_points(*emap, ref_points, stream=stream)
        return self.device_polyset().tabulate_batch_shared(order, ref_points, verts, mapping=self._mapping, out=out,
                                                           stream=stream)

    def value_shape(self):
        return self.poly_set.get_shape()

    def get_num_members(self, arg):
        return self.get_nodal_basis().get_expansion_set().get_num_members(arg)

    @staticmethod
    def is_nodal():
        return True


EVAL_KERNEL_MAXK, EVAL_KERNEL_MAXORDER, EVAL_MAXRHS = 6, 2, 8     # the instance set of csrc/evaluate.hpp
_EVAL_MAPPINGS = ("affine", "covariant piola", "contravariant piola")


def fused_evaluation_refusal(element, order):
    """None where the fused evaluation kernel (csrc/evaluate.hpp) applies to ``element`` at derivative order ``order``,
    otherwise the reason it does not, as text."""
    if not isinstance(element, CiarletElement):
        return f"{type(element).__name__} is not a Ciarlet element over a simplex expansion set"
    poly_set = element.poly_set
    es = poly_set.get_expansion_set()
    if hasattr(es, "device_line"):
        return "the nodal basis is the 1-D primal Lagrange basis, not a simplex polynomial set"
    if getattr(es, "num_cells", None) != 1:
        return "the nodal basis lives on a macro cell"
    if poly_set.get_reference_element().get_shape() != element.ref_el.get_shape():
        return "the element's cell is not the cell of its polynomial set"
    sd = element.ref_el.get_spatial_dimension()
    if sd not in (1, 2, 3):
        return f"spatial dimension {sd}"
    if element._expansion_variant not in (None, "bubble"):
        return f"expansion variant {element._expansion_variant!r}"
    degree = poly_set.get_embedded_degree()
    if not 1 <= degree <= EVAL_KERNEL_MAXK:
        return f"embedded degree {degree} (the kernel covers 1..{EVAL_KERNEL_MAXK})"
    if not 0 <= order <= EVAL_KERNEL_MAXORDER:
        return f"derivative order {order} (the kernel covers 0..{EVAL_KERNEL_MAXORDER})"
    shape = tuple(poly_set.get_shape())
    if shape not in ((), (sd,)):
        return f"value shape {shape} (the kernel covers () and ({sd},))"
    if element._mapping not in _EVAL_MAPPINGS:
        return f"mapping {element._mapping!r}"
    if not isinstance(element.device_polyset(), runtime.SimplexPolySet):
        return "the nodal basis is not a SimplexPolySet on the device"
    return None


def _eval_element(element):
    """The element's device form for the fused kernel (fx_eval_element), created at first use."""
    dev = element.__dict__.get("_eval_dev")
    if dev is None:
        poly_set = element.poly_set
        dev = runtime.EvalElement(element.ref_el.get_spatial_dimension(), poly_set.get_embedded_degree(),
                                  element._expansion_variant, element._expansion_scale,
                                  numpy.asarray(poly_set.get_reference_element().get_vertices(), dtype=float),
                                  poly_set.get_coeffs(), value_shape=poly_set.get_shape())
        element._eval_dev = dev
    return dev


def _general_tables(element, order, points, verts, pushforward, stream):
    kwargs = {}
    if verts is not None:
        kwargs["verts"] = verts
    if pushforward:
        kwargs["pushforward"] = True
    if stream is not None:
        kwargs["stream"] = stream
    return element.tabulate_batch(order, points, **kwargs)


def evaluate_kernel(element, order, npts, nrhs=1, has_verts=False, pushforward=False):
    """What ``evaluate_batch`` runs for a request shape: ``"fused: fxk::eval_kernel<sd,order,vdim> degree=<n> P=<requests per
    item> chunks=<point chunks per request>"`` (fx_eval_kernel), or ``"general: tabulate_batch + einsum (<why not fused>)"``."""
    why = fused_evaluation_refusal(element, int(order))
    if why is None and pushforward and not has_verts:
        raise ValueError("a push-forward needs the physical cells (verts)")
    if why is not None:
        return f"general: tabulate_batch + einsum ({why})"
    poly_set = element.poly_set
    shape = tuple(poly_set.get_shape())
    sd = element.ref_el.get_spatial_dimension()
    return "fused: " + runtime.eval_kernel(sd, poly_set.get_embedded_degree(), order, sd if shape else 1, len(poly_set.get_coeffs()),
                                           npts, nrhs)


def evaluate_batch(element, order, points, dofs, verts=None, out=None, stream=None, pushforward=False, *, route=None):
    """Finite element functions at points, batched: points (nreq, npts, sd), dofs (nreq, ndof) or (nreq, nrhs, ndof) with
    1 <= nrhs <= 8 (float64, host or device) -> device tensor (nreq, ntab, [nrhs,] *value_shape, npts), tables in mis() order,

        out[r, t, j, ..., q] = sum_i dofs[r, j, i] * tabulate_batch(order, points, verts=verts, pushforward=pushforward)[r, t, i, ..., q].

    ``verts`` and ``pushforward`` mean what they mean for ``tabulate_batch``.  ``route=None`` takes the fused kernel
    (fx_eval_batch: the table is never formed in device memory) where it applies -- Ciarlet elements over a simplex polynomial
    set, expansion variant default or "bubble", embedded degree 1-6, order 0-2, value shape () or (sd,), affine or single Piola
    map -- and otherwise the general route, ``tabulate_batch`` followed by ``torch.einsum``; ``route="general"`` forces that
    composition, ``route="fused"`` the kernel (NotImplementedError with the reason where it does not apply).  Everything is
    validated before anything is launched (ValueError); the work is ordered on ``stream``."""
    import torch
    if route not in (None, "fused", "general"):
        raise ValueError(f"unknown route {route!r}")
    order = int(order)
    if order < 0:
        raise ValueError("negative derivative order")
    sd = element.get_reference_element().get_spatial_dimension()
    ndof = element.space_dimension()
    pshape = tuple(points.shape) if hasattr(points, "shape") else numpy.shape(points)
    if len(pshape) != 3 or pshape[2] != sd:
        raise ValueError(f"points must have shape (nreq, npts, {sd}), got {pshape}")
    nreq, npts = int(pshape[0]), int(pshape[1])
    if isinstance(dofs, torch.Tensor):
        if dofs.dtype != torch.float64:
            raise ValueError(f"dofs must be float64, got {dofs.dtype}")
    else:
        dofs = numpy.asarray(dofs)
        if dofs.dtype != numpy.float64:
            raise ValueError(f"dofs must be float64, got {dofs.dtype}")
    dshape = tuple(dofs.shape)
    if len(dshape) not in (2, 3) or dshape[0] != nreq or dshape[-1] != ndof:
        raise ValueError(f"dofs must have shape ({nreq}, {ndof}) or ({nreq}, nrhs, {ndof}), got {dshape}")
    squeeze = len(dshape) == 2
    nrhs = 1 if squeeze else int(dshape[1])
    if not 1 <= nrhs <= EVAL_MAXRHS:
        raise ValueError(f"{nrhs} right-hand sides: evaluate_batch takes 1..{EVAL_MAXRHS} per call")
    if verts is not None:
        vshape = tuple(verts.shape) if hasattr(verts, "shape") else numpy.shape(verts)
        if vshape != (nreq, sd + 1, sd):
            raise ValueError(f"verts must have shape ({nreq}, {sd + 1}, {sd}), got {vshape}")
    if pushforward and verts is None:
        raise ValueError("a push-forward needs the physical cells (verts)")
    vshape_el = tuple(element.value_shape())
    ntab = runtime.num_tables(sd, order)
    shape = (nreq, ntab) + (() if squeeze else (nrhs,)) + vshape_el + (npts,)
    ctx = runtime.Context.get()
    if out is not None and (not isinstance(out, torch.Tensor) or tuple(out.shape) != shape or out.dtype != torch.float64
                            or not out.is_contiguous() or out.device != ctx.device):
        raise ValueError(f"out must be a contiguous float64 device tensor of shape {shape}")
    vdim = int(numpy.prod(vshape_el, dtype=int)) if vshape_el else 1
    if ntab * nrhs * vdim * npts >= 2 ** 31 or nreq * ntab * nrhs * vdim * npts >= 2 ** 62:
        raise ValueError("the request or the batch does not fit the index arithmetic of the kernels")
    why = fused_evaluation_refusal(element, order) if route != "general" else "route='general'"
    if route == "fused" and why is not None:
        raise NotImplementedError(f"the fused evaluation kernel does not apply: {why}")
    if why is None:
        dev = _eval_element(element)
        d3 = runtime._as_device(dofs, ctx).reshape(nreq, nrhs, ndof)
        o5 = None if out is None else out.view((nreq, ntab, nrhs) + vshape_el + (npts,))
        res = runtime.eval_batch(dev, order, points, d3, verts=verts, out=o5, stream=stream,
                                 mapping=element._mapping if pushforward else None)
        return out if out is not None else res.view(shape)
    # the composition a user can write: the table, then the contraction
    with (torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()):
        tables = _general_tables(element, order, points, verts, pushforward, stream)
        d3 = runtime._as_device(dofs, ctx).reshape(nreq, nrhs, ndof)
        res = torch.einsum("rji,rti...->rtj...", d3, tables)
        res = res.reshape(shape)
        if out is not None:
            out.copy_(res)
            return out
        return res.contiguous()


def entity_support_dofs(elem, entity_dim):
    """{entity id: dofs whose basis functions do not vanish on that entity} for the sub-entities of dimension
    ``entity_dim`` (FIAT/finite_element.py:222-264; FInAT stands on the same computation,
    finat/finiteelementbase.py:85-119): the default rule of degree max(2 degree, 1) on the reference sub-entity, mapped
    onto every entity of that dimension, ONE batched order-0 tabulation of all of them on the device, the squared norm of
    every basis function against the weights on the device (fx_tables_squared_norm), cut at 1e-8."""
    import torch
    from .quadrature import create_quadrature
    cache = elem.__dict__.setdefault("_entity_support_dofs", {})
    if entity_dim in cache:
        return cache[entity_dim]
    ref_el = elem.get_reference_element()
    entity_cell = ref_el.construct_subelement(entity_dim)
    quad = create_quadrature(entity_cell, max(2 * elem.degree(), 1))
    weights = numpy.asarray(quad.get_weights(), dtype=float)
    qpts = numpy.asarray(quad.get_points(), dtype=float).reshape(len(weights), -1)
    ids = list(elem.entity_dofs()[entity_dim].keys())
    eps = 1.e-8
    if hasattr(elem, "entity_map"):
        # simplex elements: every entity is one request of the same batch, the entity transform runs on the device
        sd = ref_el.get_spatial_dimension()
        blocks = []
        for f in ids:
            emap = elem.entity_map((entity_dim, f))
            blocks.append(runtime._as_device(qpts, runtime.Context.get()) if emap is None else runtime.map_points(*emap, qpts))
        pts = torch.stack(blocks).reshape(len(ids), len(weights), sd)
        tabs = elem.tabulate_batch(0, pts)[:, 0]                        # (nent, ndof, *value_shape, npts)
    else:
        # tensor-product elements: the factors' entity transforms differ per entity (tabulate_batch(..., entity=))
        tabs = torch.cat([elem.tabulate_batch(0, qpts[None], entity=(entity_dim, f))[:, 0] for f in ids])
    ints = runtime.fetch(runtime.tables_squared_norm(tabs, weights))
    result = {f: [dof for dof, i in enumerate(ints[k]) if i > eps] for k, f in enumerate(ids)}
    cache[entity_dim] = result
    return result
