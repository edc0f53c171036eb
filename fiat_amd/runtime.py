"""Device runtime: contexts, element handles and the batched entry points.

PyTorch-ROCm is used only as the owner of device memory and streams; every
computation goes through the C ABI (include/fiat_amd.h) into the HIP kernels.
"""
import contextlib
import ctypes
import math
from ctypes import c_float, c_int, c_void_p

import numpy as np
import torch

from . import _lib
from ._lib import VARIANTS, check, host_ptr, lib

_contexts = {}


class Context:
    """One per GPU (fx_ctx).  ``Context.get()`` returns the context of the
    current torch device; creation fails loudly when no GPU is present."""

    def __init__(self, device_index):
        h = c_void_p()
        check(lib.fx_ctx_create(int(device_index), ctypes.byref(h)))
        self.handle = h
        self.device = torch.device("cuda", device_index)
        ncu, lds = c_int(0), c_int(0)
        name = ctypes.create_string_buffer(64)
        check(lib.fx_ctx_info(h, ctypes.byref(ncu), ctypes.byref(lds), name, 64))
        self.num_cu, self.lds_per_cu, self.arch = ncu.value, lds.value, name.value.decode()

    def check(self, stream=None):
        """Synchronise ``stream`` and raise FiatAmdError if a kernel of this context reported a scheduling failure."""
        check(lib.fx_ctx_check(self.handle, _stream_ptr(stream)))

    def set_policy(self, *names):
        """Kernel-selection policy (fx_ctx_set_policy): names from ``_lib.POLICY``; no names = the default."""
        flags = 0
        for n in names:
            flags |= _lib.POLICY[n]
        check(lib.fx_ctx_set_policy(self.handle, flags))

    def get_policy(self):
        flags = ctypes.c_uint(0)
        check(lib.fx_ctx_get_policy(self.handle, ctypes.byref(flags)))
        return {n for n, bit in _lib.POLICY.items() if flags.value & bit}

    @contextlib.contextmanager
    def policy(self, *names):
        """``with ctx.policy("no_fixed"): ...`` -- reach an A/B partner kernel through the same entry points."""
        before = self.get_policy()
        self.set_policy(*names)
        try:
            yield self
        finally:
            self.set_policy(*before)

    @staticmethod
    def get(device=None):
        if device is None:
            if not torch.cuda.is_available():
                # let the C library produce the error message
                idx = 0
            else:
                idx = torch.cuda.current_device()
        else:
            idx = torch.device(device).index or 0
        if idx not in _contexts:
            _contexts[idx] = Context(idx)
        return _contexts[idx]


def fetch(tensor, stream=None):
    """Device tensor -> NumPy array, then ``fx_ctx_check``: a dynamically scheduled kernel that gave up waiting for its
    work queue (csrc/work_queue.hpp) leaves incomplete tables -- the facade raises instead of returning them."""
    host = tensor.cpu().numpy()
    if tensor.is_cuda:
        Context.get(tensor.device).check(stream)
    return host


def _stream_ptr(stream):
    if stream is None:
        stream = torch.cuda.current_stream()
    return c_void_p(stream.cuda_stream)


def _dev_ptr(t):
    return c_void_p(t.data_ptr())


def _as_device(x, ctx):
    if isinstance(x, torch.Tensor):
        if x.device != ctx.device or x.dtype != torch.float64 or not x.is_contiguous():
            x = x.to(device=ctx.device, dtype=torch.float64).contiguous()
        return x
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64)).to(ctx.device)


def num_tables(sd, order):
    return math.comb(sd + order, sd)


class SimplexPolySet:
    """Device-resident polynomial set over a simplex expansion set (fx_element):
    coeffs (ndof, *value_shape, nexp) over the Dubiner basis of degree n."""

    def __init__(self, sd, n, variant=None, scale=None, verts=None, coeffs=None, ndof=None,
                 value_shape=(), ctx=None):
        self.ctx = ctx or Context.get()
        self.sd, self.n, self.variant = sd, n, variant
        self.nexp = math.comb(n + sd, sd)
        self.value_shape = tuple(value_shape)
        self.vdim = int(np.prod(self.value_shape, dtype=int)) if self.value_shape else 1
        self.verts = None if verts is None else np.ascontiguousarray(verts, dtype=np.float64).reshape(sd + 1, sd)
        if coeffs is not None:
            coeffs = np.ascontiguousarray(coeffs, dtype=np.float64)
            ndof = coeffs.shape[0]
            assert coeffs.size == ndof * self.vdim * self.nexp
        elif ndof is None:
            ndof = self.nexp
        self.ndof = ndof
        h = c_void_p()
        check(lib.fx_element_create(self.ctx.handle, sd, n, VARIANTS[variant],
                                    -1.0 if scale is None else float(scale),
                                    None if self.verts is None else host_ptr(self.verts),
                                    ndof, self.vdim, None if coeffs is None else host_ptr(coeffs),
                                    ctypes.byref(h)))
        self.handle = h

    def set_coeffs(self, coeffs):
        coeffs = np.ascontiguousarray(coeffs, dtype=np.float64)
        ndof = coeffs.shape[0]
        assert coeffs.size == ndof * self.vdim * self.nexp
        check(lib.fx_element_set_coeffs(self.handle, ndof, self.vdim, host_ptr(coeffs)))
        self.ndof = ndof

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                lib.fx_element_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def out_shape(self, order, nreq, npts):
        return (nreq, num_tables(self.sd, order), self.ndof) + self.value_shape + (npts,)

    MAPPINGS = {"affine": 0, "covariant piola": 1, "contravariant piola": 2, "double covariant piola": 3,
                "double contravariant piola": 4, "covariant contravariant piola": 5}

    def tabulate_batch(self, order, pts, verts=None, out=None, stream=None, mapping=None):
        """pts (nreq, npts, sd) -> (nreq, ntab, ndof, *value_shape, npts) on the GPU.

        With per-request cells ``verts`` the derivatives are taken with respect to the physical
        coordinates; ``mapping`` ("affine", "covariant piola", "contravariant piola": the names
        of FiniteElement.mapping()) additionally pushes vector-valued functions forward to the
        physical cells (fx_pushforward_batch)."""
        ctx = self.ctx
        pts = _as_device(pts, ctx)
        if pts.dim() != 3 or pts.shape[2] != self.sd:
            raise ValueError(f"points must have shape (nreq, npts, {self.sd}), got {tuple(pts.shape)}")
        nreq, npts = pts.shape[0], pts.shape[1]
        if verts is not None:
            verts = _as_device(verts, ctx)
            if tuple(verts.shape) != (nreq, self.sd + 1, self.sd):
                raise ValueError("verts must have shape (nreq, sd+1, sd)")
        shape = self.out_shape(order, nreq, npts)
        if out is None:
            out = torch.empty(shape, dtype=torch.float64, device=ctx.device)
        elif tuple(out.shape) != shape or out.dtype != torch.float64 or not out.is_contiguous():
            raise ValueError("out has the wrong shape/dtype/layout")
        if mapping is not None and mapping not in self.MAPPINGS:
            raise ValueError(f"unknown mapping {mapping!r}")
        if mapping not in (None, "affine") and verts is None:
            raise ValueError("a Piola push-forward needs the physical cells (verts)")
        if mapping in (None, "affine"):
            check(lib.fx_tabulate_batch(ctx.handle, self.handle, int(order), nreq, npts, _dev_ptr(pts),
                                        None if verts is None else _dev_ptr(verts), _dev_ptr(out), _stream_ptr(stream)))
        else:   # fused into the kernel's output stage where the shape allows, else a second pass
            check(lib.fx_tabulate_batch_mapped(ctx.handle, self.handle, self.MAPPINGS[mapping], int(order), nreq, npts,
                                               _dev_ptr(pts), _dev_ptr(verts), _dev_ptr(out), _stream_ptr(stream)))
        return out

    def pushforward_batch(self, order, out, verts, mapping):
        """In-place push-forward of tables produced by ``tabulate_batch(order, pts, verts=verts)``
        (fx_pushforward_batch: the separate pass; ``tabulate_batch(..., mapping=...)`` fuses it where it can)."""
        if mapping not in self.MAPPINGS:
            raise ValueError(f"unknown mapping {mapping!r}")
        verts = _as_device(verts, self.ctx)
        nreq, npts = out.shape[0], out.shape[-1]
        check(lib.fx_pushforward_batch(self.ctx.handle, self.handle, self.MAPPINGS[mapping], int(order), nreq, npts,
                                       _dev_ptr(verts), _dev_ptr(out), _stream_ptr(None)))
        return out

    def tabulate_batch_shared(self, order, ref_pts, verts, mapping="affine", out=None, stream=None):
        """One point set ``ref_pts`` (npts, sd) on the element's own cell, pushed forward to the
        cells ``verts`` (nreq, sd+1, sd): (nreq, ntab, ndof, *value_shape, npts) on the GPU, equal to
        ``tabulate_batch(order, F_r(ref_pts), verts, mapping=mapping)`` (fx_tabulate_batch_shared)."""
        ctx = self.ctx
        ref_pts = _as_device(ref_pts, ctx)
        verts = _as_device(verts, ctx)
        if ref_pts.dim() != 2 or ref_pts.shape[1] != self.sd:
            raise ValueError(f"reference points must have shape (npts, {self.sd})")
        if verts.dim() != 3 or tuple(verts.shape[1:]) != (self.sd + 1, self.sd):
            raise ValueError("verts must have shape (nreq, sd+1, sd)")
        if mapping not in self.MAPPINGS:
            raise ValueError(f"unknown mapping {mapping!r}")
        nreq, npts = verts.shape[0], ref_pts.shape[0]
        shape = self.out_shape(order, nreq, npts)
        if out is None:
            out = torch.empty(shape, dtype=torch.float64, device=ctx.device)
        elif tuple(out.shape) != shape or out.dtype != torch.float64 or not out.is_contiguous():
            raise ValueError("out has the wrong shape/dtype/layout")
        check(lib.fx_tabulate_batch_shared(ctx.handle, self.handle, self.MAPPINGS[mapping], int(order), nreq, npts,
                                           _dev_ptr(ref_pts), _dev_ptr(verts), _dev_ptr(out), _stream_ptr(stream)))
        return out

    def kernel_name(self, order, nreq, npts, has_verts=False, instance=False, mapping=None, digest=False):
        """Device kernel ``tabulate_batch`` launches for this request shape (fx_plan_kernel); ``instance``: with the
        registry instance of the stacked-matrix kernel; ``mapping``: the Piola map asked for with the tabulation;
        ``digest``: followed by ``{...}``, the planned launch itself -- family, registry row, grid, LDS bytes, every
        integer the launcher reads and a hash of the floating-point arguments."""
        size = 1024 if digest else 96
        buf = ctypes.create_string_buffer(size)
        code = self.MAPPINGS[mapping] if mapping else 0
        flags = int(bool(has_verts)) | (2 if instance else 0) | ((code << 2) if code in (1, 2) else 0) | (16 if digest else 0)
        check(lib.fx_plan_kernel(self.ctx.handle, self.handle, int(order), int(nreq), int(npts), flags, buf, size))
        return buf.value.decode()

    def time_tabulate_batch(self, order, pts, verts, out, reps, stream=None):
        """Average kernel milliseconds over ``reps`` launches (HIP events on the launch stream)."""
        ms = c_float(0.0)
        check(lib.fx_time_tabulate_batch(self.ctx.handle, self.handle, int(order), pts.shape[0], pts.shape[1],
                                         _dev_ptr(pts), None if verts is None else _dev_ptr(verts), _dev_ptr(out),
                                         _stream_ptr(stream), int(reps), ctypes.byref(ms)))
        return ms.value


class MacroPolySet:
    """Device-resident polynomial set over the expansion set of a macro cell (fx_macro_element):
    coeffs (ndof, *value_shape, nmacro) over the members of the complex; the kernel bins every point to
    its sub-cell(s), runs the sub-cell's recurrence and contracts (FIAT/expansions.py:449-490)."""

    def __init__(self, sd, n, variant, scale, parent_verts, cell_verts, cell_node_map, nmacro, cell_scale=None,
                 coeffs=None, value_shape=(), ctx=None):
        self.ctx = ctx or Context.get()
        self.sd, self.n, self.variant = sd, n, variant
        self.nexp = math.comb(n + sd, sd)
        self.nmacro = int(nmacro)
        self.value_shape = tuple(value_shape)
        self.vdim = int(np.prod(self.value_shape, dtype=int)) if self.value_shape else 1
        parent = np.ascontiguousarray(parent_verts, dtype=np.float64).reshape(sd + 1, sd)
        cells = np.ascontiguousarray(cell_verts, dtype=np.float64)
        ncell = cells.shape[0]
        if cells.shape != (ncell, sd + 1, sd):
            raise ValueError("cell_verts must have shape (ncell, sd+1, sd)")
        cmap = np.ascontiguousarray(cell_node_map, dtype=np.int32)
        if cmap.shape != (ncell, self.nexp):
            raise ValueError(f"cell_node_map must have shape ({ncell}, {self.nexp}), got {cmap.shape}")
        cs = None if cell_scale is None else np.ascontiguousarray(cell_scale, dtype=np.float64).reshape(ncell)
        if coeffs is not None:
            coeffs = np.ascontiguousarray(coeffs, dtype=np.float64)
            self.ndof = coeffs.shape[0]
            assert coeffs.size == self.ndof * self.vdim * self.nmacro
        else:
            self.ndof = self.nmacro
        self.ncell = ncell
        h = c_void_p()
        check(lib.fx_macro_element_create(self.ctx.handle, sd, n, VARIANTS[variant], float(scale), host_ptr(parent), ncell,
                                          host_ptr(cells), self.nmacro, host_ptr(cmap),
                                          None if cs is None else host_ptr(cs), self.ndof, self.vdim,
                                          None if coeffs is None else host_ptr(coeffs), ctypes.byref(h)))
        self.handle = h

    def set_coeffs(self, coeffs):
        coeffs = np.ascontiguousarray(coeffs, dtype=np.float64)
        ndof = coeffs.shape[0]
        assert coeffs.size == ndof * self.vdim * self.nmacro
        check(lib.fx_macro_element_set_coeffs(self.handle, ndof, self.vdim, host_ptr(coeffs)))
        self.ndof = ndof

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                lib.fx_macro_element_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def out_shape(self, order, nreq, npts):
        return (nreq, num_tables(self.sd, order), self.ndof) + self.value_shape + (npts,)

    def tabulate_batch(self, order, pts, verts=None, out=None, stream=None, mapping=None):
        """pts (nreq, npts, sd) -> (nreq, ntab, ndof, *value_shape, npts) on the GPU; ``verts``: per-request
        parent cells (points are binned after pulling them back to the element's parent cell)."""
        if mapping not in (None, "affine"):
            raise NotImplementedError("Piola push-forwards of macro elements")
        ctx = self.ctx
        pts = _as_device(pts, ctx)
        if pts.dim() != 3 or pts.shape[2] != self.sd:
            raise ValueError(f"points must have shape (nreq, npts, {self.sd}), got {tuple(pts.shape)}")
        nreq, npts = pts.shape[0], pts.shape[1]
        if verts is not None:
            verts = _as_device(verts, ctx)
            if tuple(verts.shape) != (nreq, self.sd + 1, self.sd):
                raise ValueError("verts must have shape (nreq, sd+1, sd)")
        shape = self.out_shape(order, nreq, npts)
        if out is None:
            out = torch.empty(shape, dtype=torch.float64, device=ctx.device)
        elif tuple(out.shape) != shape or out.dtype != torch.float64 or not out.is_contiguous():
            raise ValueError("out has the wrong shape/dtype/layout")
        check(lib.fx_macro_tabulate_batch(ctx.handle, self.handle, int(order), nreq, npts, _dev_ptr(pts),
                                          None if verts is None else _dev_ptr(verts), _dev_ptr(out), _stream_ptr(stream)))
        return out

    _SMALL = {(2, 1): 2, (2, 2): 2, (2, 3): 2, (3, 1): 2, (3, 2): 2, (3, 3): 1}   # (sd, n): highest order (api.hip)

    def kernel_name(self, order, nreq, npts, has_verts=False):
        """Kernel a request shape maps to (mirrors the selection in fx_macro_tabulate_batch)."""
        small = (order <= self._SMALL.get((self.sd, self.n), -1) and npts <= 64
                 and "no_macro_small" not in self.ctx.get_policy())
        return "fxk::tabulate_macro_small" if small else "fxk::tabulate_simplex_kernel<MACRO>"


def collapsed_quadrature(sd, m, verts=None, ctx=None, stream=None):
    """Collapsed Gauss-Jacobi rule with ``m`` points per direction on the simplex ``verts``
    ((sd+1, sd) array, default: the UFC simplex), produced on the device:
    (points (m**sd, sd), weights (m**sd,)) as CUDA tensors (fx_collapsed_quadrature)."""
    ctx = ctx or Context.get()
    n = int(m) ** int(sd)
    pts = torch.empty((n, sd), dtype=torch.float64, device=ctx.device)
    wts = torch.empty((n,), dtype=torch.float64, device=ctx.device)
    hv = None
    if verts is not None:
        hv = np.ascontiguousarray(verts, dtype=np.float64)
        if hv.shape != (sd + 1, sd):
            raise ValueError("verts must have shape (sd+1, sd)")
    check(lib.fx_collapsed_quadrature(ctx.handle, int(sd), int(m), None if hv is None else host_ptr(hv), _dev_ptr(pts),
                                      _dev_ptr(wts), _stream_ptr(stream)))
    return pts, wts


def classify_tables(tables, rtol=1e-5, ctx=None, stream=None):
    """Per table of a device tensor ``tables[..., rows, npts]``: (max |x|, max(|x - x[..., :1]| - rtol |x[..., :1]|))
    as a device tensor ``[..., 2]`` (fx_classify_tables; what finat/fiat_elements.py:92-111 asserts)."""
    ctx = ctx or Context.get()
    tables = _as_device(tables, ctx)
    if tables.dim() < 2:
        raise ValueError("tables must have shape (..., rows, npts)")
    rows, npts = tables.shape[-2:]
    lead = tuple(tables.shape[:-2])
    ntables = int(np.prod(lead, dtype=np.int64)) if lead else 1
    stats = torch.empty(lead + (2,), dtype=torch.float64, device=ctx.device)
    check(lib.fx_classify_tables(ctx.handle, ntables, int(rows), int(npts), float(rtol), _dev_ptr(tables), _dev_ptr(stats),
                                 _stream_ptr(stream)))
    return stats


def tables_squared_norm(tables, weights, ctx=None, stream=None):
    """``tables[n, rows, *value_shape, npts]`` (order-0 tables at the points of one rule) and the rule's ``weights[npts]``
    -> device tensor ``[n, rows]`` of squared L2 norms (fx_tables_squared_norm; FIAT/finite_element.py:250-260)."""
    ctx = ctx or Context.get()
    tables = _as_device(tables, ctx)
    weights = _as_device(weights, ctx)
    if tables.dim() < 3 or weights.dim() != 1 or weights.shape[0] != tables.shape[-1]:
        raise ValueError("tables must have shape (n, rows, ..., npts) and weights (npts,)")
    n, rows, npts = int(tables.shape[0]), int(tables.shape[1]), int(tables.shape[-1])
    vdim = int(np.prod(tables.shape[2:-1], dtype=np.int64)) if tables.dim() > 3 else 1
    out = torch.empty((n, rows), dtype=torch.float64, device=ctx.device)
    check(lib.fx_tables_squared_norm(ctx.handle, n, rows, vdim, npts, _dev_ptr(tables), _dev_ptr(weights), _dev_ptr(out),
                                     _stream_ptr(stream)))
    return out


def tables_point_major(tables, out=None, ctx=None, stream=None):
    """``tables[..., rows, npts]`` -> a new contiguous device tensor ``[..., npts, rows]`` (fx_tables_point_major)."""
    ctx = ctx or Context.get()
    tables = _as_device(tables, ctx)
    if tables.dim() < 2:
        raise ValueError("tables must have shape (..., rows, npts)")
    rows, npts = tables.shape[-2:]
    lead = tuple(tables.shape[:-2])
    ntables = int(np.prod(lead, dtype=np.int64)) if lead else 1
    if out is None:
        out = torch.empty(lead + (npts, rows), dtype=torch.float64, device=ctx.device)
    check(lib.fx_tables_point_major(ctx.handle, ntables, int(rows), int(npts), _dev_ptr(tables), _dev_ptr(out),
                                    _stream_ptr(stream)))
    return out


def map_points(M, b, pts, ctx=None, stream=None):
    """Affine image of a batch of points on the device: pts (..., din) -> (..., dout) = pts M^T + b
    (fx_map_points; the entity transform of ``tabulate(..., entity=)``)."""
    ctx = ctx or Context.get()
    b = np.ascontiguousarray(b, dtype=np.float64).reshape(-1)
    dout = b.shape[0]
    M = np.ascontiguousarray(M, dtype=np.float64).reshape(dout, -1)
    din = M.shape[1]
    if isinstance(pts, torch.Tensor):
        lead = tuple(pts.shape[:-1])
        if pts.shape[-1] != din:
            raise ValueError(f"points must have {din} coordinates, got {pts.shape[-1]}")
        src = _as_device(pts, ctx) if din else None
    else:
        pts = np.asarray(pts, dtype=np.float64)
        lead = tuple(pts.shape[:-1])
        if pts.shape[-1] != din:
            raise ValueError(f"points must have {din} coordinates, got {pts.shape[-1]}")
        src = _as_device(pts, ctx) if din else None
    n = int(np.prod(lead, dtype=np.int64)) if lead else 1
    out = torch.empty(lead + (dout,), dtype=torch.float64, device=ctx.device)
    check(lib.fx_map_points(ctx.handle, din, dout, host_ptr(M) if din else None, host_ptr(b), n,
                            None if src is None else _dev_ptr(src), _dev_ptr(out), _stream_ptr(stream)))
    return out


def table_outer(order, sdA, sdB, tabA, tabB, out=None, ctx=None, stream=None):
    """Tensor product of two tabulated factors (fx_table_outer_batch): tabA (nreq, ntabA, ndofA, [vdimA,] npts),
    tabB (nreq, ntabB, ndofB, [vdimB,] npts) -> (nreq, ntab, ndofA * ndofB, [vdim,] npts), the tables of all
    |alpha| <= order of the product in mis() order."""
    ctx = ctx or Context.get()
    tabA, tabB = _as_device(tabA, ctx), _as_device(tabB, ctx)
    nreq, npts = tabA.shape[0], tabA.shape[-1]
    if tabB.shape[0] != nreq or tabB.shape[-1] != npts:
        raise ValueError("factor tables must share the request and point axes")
    vdimA = tabA.shape[3] if tabA.dim() == 5 else 1
    vdimB = tabB.shape[3] if tabB.dim() == 5 else 1
    if vdimA > 1 and vdimB > 1:
        raise NotImplementedError("tabulate does not support two vector-valued inputs")
    rowsA, rowsB = tabA.shape[2], tabB.shape[2]
    if tabA.shape[1] != num_tables(sdA, order) or tabB.shape[1] != num_tables(sdB, order):
        raise ValueError("factor tables must hold all derivative tables up to the product's order")
    vshape = (max(vdimA, vdimB),) if max(tabA.dim(), tabB.dim()) == 5 else ()
    shape = (nreq, num_tables(sdA + sdB, order), rowsA * rowsB) + vshape + (npts,)
    if out is None:
        out = torch.empty(shape, dtype=torch.float64, device=ctx.device)
    elif tuple(out.shape) != shape or not out.is_contiguous():
        raise ValueError("out has the wrong shape/layout")
    check(lib.fx_table_outer_batch(ctx.handle, int(order), int(sdA), int(sdB), nreq, npts, rowsA, vdimA, rowsB, vdimB,
                                   _dev_ptr(tabA), _dev_ptr(tabB), _dev_ptr(out), _stream_ptr(stream)))
    return out


def riesz_assemble(wts, expvals, ctx=None):
    """mat[i, k] = sum_q wts[i, q] expvals[k, q] on the device."""
    ctx = ctx or Context.get()
    wts = _as_device(wts, ctx)
    expvals = _as_device(expvals, ctx)
    nrows, nq = wts.shape
    nexp = expvals.shape[0]
    assert expvals.shape[1] == nq
    mat = torch.empty((nrows, nexp), dtype=torch.float64, device=ctx.device)
    check(lib.fx_riesz_assemble(ctx.handle, nrows, nq, nexp, _dev_ptr(wts), _dev_ptr(expvals), _dev_ptr(mat),
                                _stream_ptr(None)))
    return mat


def vandermonde_solve_batch(A, B, ctx=None, return_V=False):
    """X = solve((A B^T)^T, B) per system; raises LinAlgError on a zero pivot
    ("Singular Vandermonde matrix", finite_element.py:156)."""
    ctx = ctx or Context.get()
    A = _as_device(A, ctx)
    B = _as_device(B, ctx)
    if A.dim() == 2:
        A, B = A[None], B[None]
    nsys, ndof, m = A.shape
    assert B.shape == A.shape
    X = torch.empty_like(A)
    V = torch.empty((nsys, ndof, ndof), dtype=torch.float64, device=ctx.device) if return_V else None
    info = torch.zeros((nsys,), dtype=torch.int32, device=ctx.device)
    check(lib.fx_vandermonde_solve_batch(ctx.handle, nsys, ndof, m, _dev_ptr(A), _dev_ptr(B), _dev_ptr(X),
                                         None if V is None else _dev_ptr(V), _dev_ptr(info), _stream_ptr(None)))
    if int(info.abs().max().item()) != 0:
        raise _lib.LinAlgError("Singular Vandermonde matrix")
    return (X, V) if return_V else X


class LineLagrange:
    """1-D Lagrange basis on given nodes (fx_line_element)."""

    def __init__(self, nodes, ctx=None):
        self.ctx = ctx or Context.get()
        self.nodes = np.ascontiguousarray(nodes, dtype=np.float64).reshape(-1)
        h = c_void_p()
        check(lib.fx_line_element_create(self.ctx.handle, len(self.nodes), host_ptr(self.nodes), ctypes.byref(h)))
        self.handle = h
        self.nn = len(self.nodes)

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                lib.fx_line_element_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def tabulate_batch(self, order, pts, out=None, stream=None):
        """pts (nreq, npts) -> (nreq, order+1, nn, npts)."""
        ctx = self.ctx
        pts = _as_device(pts, ctx)
        nreq, npts = pts.shape
        if out is None:
            out = torch.empty((nreq, order + 1, self.nn, npts), dtype=torch.float64, device=ctx.device)
        check(lib.fx_line_tabulate_batch(ctx.handle, self.handle, int(order), nreq, npts, _dev_ptr(pts), _dev_ptr(out),
                                         _stream_ptr(stream)))
        return out


def prism_tabulate_batch(tri, line, order, pts, out=None, stream=None):
    """(element on a triangle) x (1-D Lagrange element) on the fused prism kernel (fx_prism_tabulate_batch): ``tri`` a
    SimplexPolySet of spatial dimension 2, ``line`` a LineLagrange, pts (nreq, npts, 3) ->
    (nreq, ntab, ndofA * ndofB, [vdim,] npts); None when the shape has no instance (the caller takes the general route)."""
    ctx = tri.ctx
    pts = _as_device(pts, ctx)
    if pts.dim() != 3 or pts.shape[2] != 3:
        raise ValueError(f"points must have shape (nreq, npts, 3), got {tuple(pts.shape)}")
    nreq, npts = int(pts.shape[0]), int(pts.shape[1])
    shapeA = tri.out_shape(order, nreq, npts)                      # (nreq, ntabA, ndofA, [vdim,] npts)
    shape = (nreq, num_tables(3, order), shapeA[2] * line.nn) + tuple(shapeA[3:])
    if out is None:
        out = torch.empty(shape, dtype=torch.float64, device=ctx.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float64 or not out.is_contiguous():
        raise ValueError("out has the wrong shape/dtype/layout")
    rc = lib.fx_prism_tabulate_batch(ctx.handle, tri.handle, line.handle, int(order), nreq, npts, _dev_ptr(pts), _dev_ptr(out),
                                     _stream_ptr(stream))
    if rc == _lib.FX_ENOTIMPL:
        return None
    check(rc)
    return out


def tensor_tabulate_batch(factors, order, pts, out=None, stream=None, grid=False):
    """Tensor-product tabulation of 1..3 LineLagrange factors.
    grid=False: pts (nreq, npts, nf); grid=True: pts (nreq, nf, q) 1-D coordinates."""
    ctx = factors[0].ctx
    nf = len(factors)
    pts = _as_device(pts, ctx)
    arr = (c_void_p * nf)(*[f.handle for f in factors])
    nbf = int(np.prod([f.nn for f in factors]))
    ntab = num_tables(nf, order)
    if grid:
        nreq, nf_, q = pts.shape
        assert nf_ == nf
        npts = q ** nf
    else:
        nreq, npts, nf_ = pts.shape
        assert nf_ == nf
    if out is None:
        out = torch.empty((nreq, ntab, nbf, npts), dtype=torch.float64, device=ctx.device)
    if grid:
        check(lib.fx_tensor_tabulate_grid_batch(ctx.handle, nf, arr, int(order), nreq, q, _dev_ptr(pts), _dev_ptr(out),
                                                _stream_ptr(stream)))
    else:
        check(lib.fx_tensor_tabulate_batch(ctx.handle, nf, arr, int(order), nreq, npts, _dev_ptr(pts), _dev_ptr(out),
                                           _stream_ptr(stream)))
    return out


HDIV, HCURL = 0, 1          # include/fiat_amd.h FX_HDIV / FX_HCURL


def hdivcurl_tabulate_batch(sd, kind, C, D, offsets, signs, order, pts, out=None, stream=None, grid=False):
    """H(div) / H(curl) elements of quadrilaterals and hexahedra on the fused kernel (fx_hdivcurl_tabulate_batch): ``C``,
    ``D`` LineLagrange factors of K+1 and K nodes, ``offsets[c]`` the first dof of component c's block (-1: none),
    ``signs[c]`` its sign.  grid=False: pts (nreq, npts, sd); grid=True: pts (nreq, sd, q) 1-D coordinates.  ->
    (nreq, ntab, ndof, sd, npts) on the device, or None when the shape has no instance (the caller takes the general route)."""
    ctx = C.ctx
    pts = _as_device(pts, ctx)
    if grid:
        if pts.dim() != 3 or pts.shape[1] != sd:
            raise ValueError(f"grid coordinates must have shape (nreq, {sd}, q), got {tuple(pts.shape)}")
        nreq, q = int(pts.shape[0]), int(pts.shape[2])
        npts = q ** sd
    else:
        if pts.dim() != 3 or pts.shape[2] != sd:
            raise ValueError(f"points must have shape (nreq, npts, {sd}), got {tuple(pts.shape)}")
        nreq, npts = int(pts.shape[0]), int(pts.shape[1])
    offs = np.ascontiguousarray(offsets, dtype=np.int32)
    sgn = np.ascontiguousarray(signs, dtype=np.int32)
    if offs.shape != (sd,) or sgn.shape != (sd,):
        raise ValueError("offsets and signs need one entry per component")
    K = D.nn
    nb = (K + 1) * K ** (sd - 1) if kind == HDIV else K * (K + 1) ** (sd - 1)
    shape = (nreq, num_tables(sd, order), nb * int((offs >= 0).sum()), sd, npts)
    if out is None:
        out = torch.empty(shape, dtype=torch.float64, device=ctx.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float64 or not out.is_contiguous():
        raise ValueError("out has the wrong shape/dtype/layout")
    if grid:
        rc = lib.fx_hdivcurl_tabulate_grid_batch(ctx.handle, int(sd), int(kind), C.handle, D.handle, host_ptr(offs),
                                                 host_ptr(sgn), int(order), nreq, q, _dev_ptr(pts), _dev_ptr(out),
                                                 _stream_ptr(stream))
    else:
        rc = lib.fx_hdivcurl_tabulate_batch(ctx.handle, int(sd), int(kind), C.handle, D.handle, host_ptr(offs), host_ptr(sgn),
                                            int(order), nreq, npts, _dev_ptr(pts), _dev_ptr(out), _stream_ptr(stream))
    if rc == _lib.FX_ENOTIMPL:
        return None
    check(rc)
    return out


def table_place(src, dst, row_offset, comp_src, comp_sign, ctx=None, stream=None):
    """The general route's placement pass (fx_table_place_batch): src (nreq, ntab, rows, *value_shape, npts) into the rows
    [row_offset, row_offset + rows) of dst (nreq, ntab, rows_dst, *value_shape_dst, npts); component c of dst is
    comp_sign[c] * component comp_src[c] of src, or zero where comp_src[c] < 0."""
    ctx = ctx or Context.get()
    src = _as_device(src, ctx)
    nreq, ntab, rows, npts = int(src.shape[0]), int(src.shape[1]), int(src.shape[2]), int(src.shape[-1])
    vdim_src = int(np.prod(src.shape[3:-1], dtype=np.int64))
    vdim_dst = int(np.prod(dst.shape[3:-1], dtype=np.int64))
    if (dst.shape[0], dst.shape[1], dst.shape[-1]) != (nreq, ntab, npts) or not dst.is_contiguous() or dst.dtype != torch.float64:
        raise ValueError("dst must share the request, table and point axes of src (contiguous float64)")
    comp = np.ascontiguousarray(comp_src, dtype=np.int32)
    sgn = np.ascontiguousarray(comp_sign, dtype=np.int32)
    if comp.shape != (vdim_dst,) or sgn.shape != (vdim_dst,):
        raise ValueError("one source component and sign per component of dst")
    check(lib.fx_table_place_batch(ctx.handle, ntab, nreq, npts, rows, vdim_src, _dev_ptr(src), int(dst.shape[2]), vdim_dst,
                                   int(row_offset), host_ptr(comp), host_ptr(sgn), _dev_ptr(dst), _stream_ptr(stream)))
    return dst


def _route(entry, *shape):
    """Route string of an ``fx_*_kernel`` entry of a companion library (host only); shapes without an instance raise."""
    buf = ctypes.create_string_buffer(160)
    _lib.companion_check(entry(*(int(v) for v in shape), buf, len(buf)))
    return buf.value.decode()


def _out_or_new(out, shape, ctx, plan):
    """``out`` if given and fit to be written, else a new tensor.  ``plan()`` is asked first: a shape without an instance
    raises before anything is allocated."""
    if out is None:
        plan()
        return torch.empty(shape, dtype=torch.float64, device=ctx.device)
    if tuple(out.shape) != shape or out.dtype != torch.float64 or not out.is_contiguous() or out.device != ctx.device:
        raise ValueError("out has the wrong shape/dtype/layout")
    return out


def serendipity_descriptor(sd, degree):
    """The dof table of S_degree the kernels are compiled from (fx_serendipity_descriptor; host only): rows (sign, code_x,
    code_y[, code_z])."""
    ndof = c_int(0)
    _lib.companion_check(_lib.serlib.fx_serendipity_dims(int(sd), int(degree), ctypes.byref(ndof)))
    rows = np.zeros((ndof.value, 1 + sd), dtype=np.int32)
    _lib.companion_check(_lib.serlib.fx_serendipity_descriptor(int(sd), int(degree), host_ptr(rows)))
    return rows


def serendipity_kernel(sd, degree, order, npts):
    """Name of the kernel instance and output route a shape takes (fx_serendipity_kernel; host only)."""
    return _route(_lib.serlib.fx_serendipity_kernel, sd, degree, order, npts)


def serendipity_tabulate_batch(sd, degree, lo, hi, order, pts, out=None, stream=None, ctx=None):
    """Serendipity S_degree on the box [lo, hi] (fx_serendipity_tabulate_batch): pts (nreq, npts, sd) -> (nreq, ntab,
    ndof, npts) on the device.  Shapes beyond the generic instance raise NotImplementedError; there is no other route."""
    ctx = ctx or Context.get()
    pts = _as_device(pts, ctx)
    if pts.dim() != 3 or pts.shape[2] != sd:
        raise ValueError(f"points must have shape (nreq, npts, {sd}), got {tuple(pts.shape)}")
    nreq, npts = int(pts.shape[0]), int(pts.shape[1])
    lo = np.ascontiguousarray(lo, dtype=np.float64).reshape(-1)
    hi = np.ascontiguousarray(hi, dtype=np.float64).reshape(-1)
    if lo.shape != (sd,) or hi.shape != (sd,):
        raise ValueError("the box needs one lower and one upper coordinate per direction")
    ndof = c_int(0)
    _lib.companion_check(_lib.serlib.fx_serendipity_dims(int(sd), int(degree), ctypes.byref(ndof)))
    if order < 0:
        raise ValueError("negative derivative order")
    shape = (nreq, num_tables(sd, order), ndof.value, npts)
    out = _out_or_new(out, shape, ctx, lambda: serendipity_kernel(sd, degree, order, npts))
    _lib.companion_check(_lib.serlib.fx_serendipity_tabulate_batch(
        ctx.handle, int(sd), int(degree), host_ptr(lo), host_ptr(hi), int(order), nreq, npts, _dev_ptr(pts), _dev_ptr(out),
        _stream_ptr(stream)))
    return out


def dpc_descriptor(sd, degree):
    """The dof table of DPC_degree the kernels are compiled from (fx_dpc_descriptor; host only): rows alpha, sd + 1 entries of
    sum ``degree``, in the order of the reference's nodes."""
    rows = np.zeros((math.comb(int(degree) + int(sd), int(sd)), sd + 1), dtype=np.int32)
    _lib.companion_check(_lib.dpclib.fx_dpc_descriptor(int(sd), int(degree), host_ptr(rows)))
    return rows


def dpc_kernel(sd, degree, order, npts):
    """Kernel instance, output route and requests per item of a shape (fx_dpc_kernel; host only):
    ``"fxk::dpc_kernel<sd,degree,order> image|stream P=<p>"``."""
    return _route(_lib.dpclib.fx_dpc_kernel, sd, degree, order, npts)


def dpc_tabulate_batch(sd, degree, lam0, G, order, pts, out=None, stream=None, ctx=None):
    """DPC_degree in closed form (fx_dpc_tabulate_batch): lambda = lam0 + G x are the barycentric coordinates of the mapped
    simplex; pts (nreq, npts, sd) -> (nreq, ntab, ndof, npts) on the device.  Shapes beyond the compile-time instances raise
    NotImplementedError (the element routes them to the general kernels before it gets here)."""
    ctx = ctx or Context.get()
    pts = _as_device(pts, ctx)
    if pts.dim() != 3 or pts.shape[2] != sd:
        raise ValueError(f"points must have shape (nreq, npts, {sd}), got {tuple(pts.shape)}")
    nreq, npts = int(pts.shape[0]), int(pts.shape[1])
    lam0 = np.ascontiguousarray(lam0, dtype=np.float64).reshape(-1)
    G = np.ascontiguousarray(G, dtype=np.float64)
    if lam0.shape != (sd + 1,) or G.shape != (sd + 1, sd):
        raise ValueError("the barycentric map needs lam0 (sd + 1,) and G (sd + 1, sd)")
    if order < 0:
        raise ValueError("negative derivative order")
    shape = (nreq, num_tables(sd, order), math.comb(int(degree) + sd, sd), npts)
    out = _out_or_new(out, shape, ctx, lambda: dpc_kernel(sd, degree, order, npts))
    _lib.companion_check(_lib.dpclib.fx_dpc_tabulate_batch(
        ctx.handle, int(sd), int(degree), host_ptr(lam0), host_ptr(G), int(order), nreq, npts, _dev_ptr(pts), _dev_ptr(out),
        _stream_ptr(stream)))
    return out


def hier_descriptor(sd, degree):
    """The dof table of IntegratedLegendre(degree) the kernels are compiled from (fx_hier_descriptor; host only): rows
    (p, q, r, entity dimension), in the order of the reference's dofs."""
    rows = np.zeros((math.comb(int(degree) + int(sd), int(sd)), 4), dtype=np.int32)
    _lib.companion_check(_lib.hierlib.fx_hier_descriptor(int(sd), int(degree), host_ptr(rows)))
    return rows


def hier_kernel(sd, degree, order, npts):
    """Kernel instance, output route and requests per item of a shape (fx_hier_kernel; host only):
    ``"fxk::hier_kernel<sd,degree,order> image|stream P=<p>"``."""
    return _route(_lib.hierlib.fx_hier_kernel, sd, degree, order, npts)


def hier_tabulate_batch(sd, degree, order, scales, A, b, pts, out=None, stream=None, ctx=None):
    """IntegratedLegendre(degree) from the C0 hierarchy (fx_hier_tabulate_batch): X = A x + b maps the cell onto the
    (-1, 1)^sd simplex, ``scales`` holds one factor per entity dimension; pts (nreq, npts, sd) -> (nreq, ntab, ndof, npts) on
    the device.  Shapes beyond the compile-time instances raise NotImplementedError (the element routes them to the general
    kernels before it gets here)."""
    ctx = ctx or Context.get()
    pts = _as_device(pts, ctx)
    if pts.dim() != 3 or pts.shape[2] != sd:
        raise ValueError(f"points must have shape (nreq, npts, {sd}), got {tuple(pts.shape)}")
    nreq, npts = int(pts.shape[0]), int(pts.shape[1])
    A = np.ascontiguousarray(A, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64).reshape(-1)
    scales = np.ascontiguousarray(scales, dtype=np.float64).reshape(-1)
    if A.shape != (sd, sd) or b.shape != (sd,) or scales.shape != (4,):
        raise ValueError("the cell map needs A (sd, sd) and b (sd,), the scales four entries")
    if order < 0:
        raise ValueError("negative derivative order")
    shape = (nreq, num_tables(sd, order), math.comb(int(degree) + sd, sd), npts)
    out = _out_or_new(out, shape, ctx, lambda: hier_kernel(sd, degree, order, npts))
    _lib.companion_check(_lib.hierlib.fx_hier_tabulate_batch(
        ctx.handle, int(sd), int(degree), int(order), host_ptr(scales), _dev_ptr(pts), nreq, npts, _dev_ptr(out),
        _stream_ptr(stream), host_ptr(A), host_ptr(b)))
    return out


class EvalElement:
    """Device form of a polynomial set for the fused evaluation kernel (fx_eval_element): the coefficients folded over the
    raw recurrence in the order of the kernel's walk, and the walk's step table."""

    def __init__(self, sd, degree, variant, scale, cell, coeffs, value_shape=(), ctx=None):
        self.ctx = ctx or Context.get()
        self.sd, self.degree, self.variant = int(sd), int(degree), variant
        self.value_shape = tuple(value_shape)
        self.vdim = int(np.prod(self.value_shape, dtype=int)) if self.value_shape else 1
        coeffs = np.ascontiguousarray(coeffs, dtype=np.float64)
        self.ndof = coeffs.shape[0]
        self.nexp = math.comb(self.degree + self.sd, self.sd)
        if coeffs.size != self.ndof * self.vdim * self.nexp:
            raise ValueError(f"coefficients must have shape (ndof, *value_shape, {self.nexp})")
        cell = None if cell is None else np.ascontiguousarray(cell, dtype=np.float64).reshape(self.sd + 1, self.sd)
        h = c_void_p()
        _lib.companion_check(_lib.evallib.fx_eval_element_create(self.ctx.handle, self.sd, self.degree, VARIANTS[variant],
                                                                  -1.0 if scale is None else float(scale),
                                                                  None if cell is None else host_ptr(cell), self.ndof, self.vdim,
                                                                  host_ptr(coeffs), ctypes.byref(h)))
        self.handle = h

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                _lib.evallib.fx_eval_element_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def kernel(self, order, npts, nrhs=1):
        return eval_kernel(self.sd, self.degree, order, self.vdim, self.ndof, npts, nrhs)


def eval_kernel(sd, degree, order, vdim, ndof, npts, nrhs=1):
    """Kernel instance and item scheme of a shape (fx_eval_kernel; host only):
    ``"fxk::eval_kernel<sd,order,vdim> degree=<n> P=<requests per item> chunks=<point chunks per request>"``."""
    return _route(_lib.evallib.fx_eval_kernel, sd, degree, order, vdim, ndof, npts, nrhs)


def eval_batch(elem, order, pts, dofs, verts=None, out=None, stream=None, mapping=None):
    """sum_i dofs[r, j, i] D^alpha phi_i(x_rq) by the fused kernel (fx_eval_batch): pts (nreq, npts, sd), dofs
    (nreq, nrhs, ndof), verts (nreq, sd + 1, sd) or None -> out (nreq, ntab, nrhs, *value_shape, npts) on the device, tables in
    mis() order.  Everything is validated here or in the C entry before anything is launched; shapes beyond the instance set
    raise NotImplementedError."""
    ctx = elem.ctx
    sd = elem.sd
    pts = _as_device(pts, ctx)
    dofs = _as_device(dofs, ctx)
    if pts.dim() != 3 or pts.shape[2] != sd:
        raise ValueError(f"points must have shape (nreq, npts, {sd}), got {tuple(pts.shape)}")
    nreq, npts = int(pts.shape[0]), int(pts.shape[1])
    if dofs.dim() != 3 or dofs.shape[0] != nreq or dofs.shape[2] != elem.ndof:
        raise ValueError(f"dofs must have shape ({nreq}, nrhs, {elem.ndof}), got {tuple(dofs.shape)}")
    nrhs = int(dofs.shape[1])
    if verts is not None:
        verts = _as_device(verts, ctx)
        if tuple(verts.shape) != (nreq, sd + 1, sd):
            raise ValueError("verts must have shape (nreq, sd+1, sd)")
    if mapping is not None and mapping not in SimplexPolySet.MAPPINGS:
        raise ValueError(f"unknown mapping {mapping!r}")
    code = SimplexPolySet.MAPPINGS[mapping] if mapping else 0
    if order < 0:
        raise ValueError("negative derivative order")
    shape = (nreq, num_tables(sd, order), nrhs) + elem.value_shape + (npts,)
    out = _out_or_new(out, shape, ctx, lambda: elem.kernel(order, npts, nrhs))
    _lib.companion_check(_lib.evallib.fx_eval_batch(ctx.handle, elem.handle, code, int(order), nreq, npts, nrhs, _dev_ptr(pts),
                                                     None if verts is None else _dev_ptr(verts), _dev_ptr(dofs), _dev_ptr(out),
                                                     _stream_ptr(stream)))
    return out


TRACE_MODES = {"identify": 0, "facet": 1, "facets": 2}      # include/fiat_amd_trace.h FX_TRACE_*


def trace_kernel(fd, degree, nfac, npts):
    """Kernel instance, output route and requests per item of a shape (fx_trace_kernel; host only):
    ``"fxk::trace_kernel<fd,degree> image|stream P=<p>"``, degree -1 for the run-time-degree instance."""
    return _route(_lib.tracelib.fx_trace_kernel, fd, degree, nfac, npts)


def trace_tabulate_batch(fd, degree, nfac, C, mode, pts, facet=0, facets=None, lam0=None, G=None, out=None, stream=None,
                         ctx=None):
    """The H(div) trace table in one pass (fx_trace_tabulate_batch): ``C`` (nf, nf), a device tensor, is the facet element over
    the kernel's expansion; pts (nreq, npts, fd + 1) in cell coordinates (mode "identify", with the barycentric map lam0, G of
    the cell) or (nreq, npts, fd) in facet coordinates (mode "facet" with ``facet``, mode "facets" with the int32 device
    tensor ``facets`` (nreq,), which the caller has checked) -> (nreq, 1, nfac * nf, npts) on the device."""
    ctx = ctx or Context.get()
    pts = _as_device(pts, ctx)
    pd = fd + 1 if mode == "identify" else fd
    if pts.dim() != 3 or pts.shape[2] != pd:
        raise ValueError(f"points must have shape (nreq, npts, {pd}), got {tuple(pts.shape)}")
    nreq, npts = int(pts.shape[0]), int(pts.shape[1])
    nf = (1, int(degree) + 1, (int(degree) + 1) * (int(degree) + 2) // 2)[fd]
    if tuple(C.shape) != (nf, nf) or C.dtype != torch.float64 or not C.is_contiguous() or C.device != ctx.device:
        raise ValueError("the facet element's matrix must be a contiguous float64 device tensor (nf, nf)")
    if mode == "facets":
        if (facets is None or tuple(facets.shape) != (nreq,) or facets.dtype != torch.int32 or not facets.is_contiguous()
                or facets.device != ctx.device):
            raise ValueError("facets must be a contiguous int32 device tensor (nreq,)")
    if mode == "identify":
        lam0 = np.ascontiguousarray(lam0, dtype=np.float64).reshape(-1)
        G = np.ascontiguousarray(G, dtype=np.float64)
        if lam0.shape != (fd + 2,) or G.shape != (fd + 2, fd + 1):
            raise ValueError("the barycentric map needs lam0 (sd + 1,) and G (sd + 1, sd)")
    shape = (nreq, 1, nfac * nf, npts)
    out = _out_or_new(out, shape, ctx, lambda: trace_kernel(fd, degree, nfac, npts))
    _lib.companion_check(_lib.tracelib.fx_trace_tabulate_batch(
        ctx.handle, int(fd), int(degree), int(nfac), TRACE_MODES[mode], int(facet),
        _dev_ptr(facets) if mode == "facets" else None, _dev_ptr(C),
        host_ptr(lam0) if mode == "identify" else None, host_ptr(G) if mode == "identify" else None,
        nreq, npts, _dev_ptr(pts), _dev_ptr(out), _stream_ptr(stream)))
    return out


class SFormsTable:
    """Device-resident term table of a BDMCE / BDMCF / trimmed serendipity element (fx_sforms_element): coef (nrows, sd),
    codes (nrows, sd, sd), see fiat_amd/sforms.py."""

    def __init__(self, sd, degree, coef, codes, ctx=None):
        self.ctx = ctx or Context.get()
        coef = np.ascontiguousarray(coef, dtype=np.float64)
        codes = np.ascontiguousarray(codes, dtype=np.int32)
        if coef.ndim != 2 or coef.shape[1] != sd or codes.shape != coef.shape + (sd,):
            raise ValueError("coef must have shape (nrows, sd) and codes (nrows, sd, sd)")
        self.sd, self.degree, self.nrows = int(sd), int(degree), int(coef.shape[0])
        h = c_void_p()
        _lib.companion_check(_lib.sflib.fx_sforms_element_create(
            self.ctx.handle, self.sd, self.degree, self.nrows, host_ptr(coef), host_ptr(codes), ctypes.byref(h)))
        self.handle = h

    def __del__(self):
        h = getattr(self, "handle", None)
        if h:
            try:
                _lib.sflib.fx_sforms_element_destroy(h)
            except Exception:
                pass
            self.handle = None


def sforms_kernel(sd, degree, nrows, order, npts):
    """Kernel instance, output route, requests per item and image budget of a shape (fx_sforms_kernel; host only):
    ``"fxk::sforms_kernel<sd,order> image|stream P=<p> budget=<bytes>"``."""
    return _route(_lib.sflib.fx_sforms_kernel, sd, degree, nrows, order, npts)


def sforms_tabulate_batch(table, lo, hi, order, pts, out=None, stream=None):
    """The element of ``table`` (SFormsTable) on the box [lo, hi] (fx_sforms_tabulate_batch): pts (nreq, npts, sd) ->
    (nreq, ntab, nrows, sd, npts) on the device.  Shapes beyond the kernel raise NotImplementedError; there is no other
    route."""
    ctx, sd = table.ctx, table.sd
    pts = _as_device(pts, ctx)
    if pts.dim() != 3 or pts.shape[2] != sd:
        raise ValueError(f"points must have shape (nreq, npts, {sd}), got {tuple(pts.shape)}")
    nreq, npts = int(pts.shape[0]), int(pts.shape[1])
    lo = np.ascontiguousarray(lo, dtype=np.float64).reshape(-1)
    hi = np.ascontiguousarray(hi, dtype=np.float64).reshape(-1)
    if lo.shape != (sd,) or hi.shape != (sd,):
        raise ValueError("the box needs one lower and one upper coordinate per direction")
    if order < 0:
        raise ValueError("negative derivative order")
    shape = (nreq, num_tables(sd, order), table.nrows, sd, npts)
    out = _out_or_new(out, shape, ctx, lambda: sforms_kernel(sd, table.degree, table.nrows, order, npts))
    _lib.companion_check(_lib.sflib.fx_sforms_tabulate_batch(
        ctx.handle, table.handle, host_ptr(lo), host_ptr(hi), int(order), nreq, npts, _dev_ptr(pts), _dev_ptr(out),
        _stream_ptr(stream)))
    return out


def cellmap_kernel(sd, nn, mapping, order, nrows, vdim, npts, grid=False):
    """Kernel instance and route of a shape on physical quadrilaterals / hexahedra (fx_cellmap_kernel; host only): ``nn`` 0
    names the general pass, ``"fxk::cellmap_apply_kernel<sd,order,mapping> <map> P=<p>"``, ``nn`` >= 1 the fused kernel of
    1-D Lagrange products, ``"fxk::cellmap_tensor_kernel<sd,nn,order,grid> image|stream P=<p>"`` (``grid``: npts is q)."""
    return _route(_lib.cellmaplib.fx_cellmap_kernel, sd, nn, mapping, order, nrows, vdim, npts, bool(grid))


def cellmap_geometry(sd, lo, hi, pts, corners, x, J, detJ, stream=None, ctx=None):
    """fx_cellmap_geometry: pts (nreq, npts, sd), corners (nreq, 2**sd, sd) -> x, J, detJ (device tensors, written)."""
    ctx = ctx or Context.get()
    _lib.companion_check(_lib.cellmaplib.fx_cellmap_geometry(
        ctx.handle, int(sd), host_ptr(lo), host_ptr(hi), int(pts.shape[0]), int(pts.shape[1]), _dev_ptr(pts), _dev_ptr(corners),
        _dev_ptr(x), _dev_ptr(J), _dev_ptr(detJ), _stream_ptr(stream)))


def cellmap_apply(sd, mapping, order, lo, hi, pts, corners, tab, out=None, stream=None, ctx=None):
    """The general pass (fx_cellmap_apply) over reference tables ``tab`` (nreq, ntab, nrows, [sd,] npts) at the points they
    were tabulated at; ``out`` None: in place."""
    ctx = ctx or Context.get()
    out = tab if out is None else out
    vdim = 1 if tab.dim() == 4 else int(tab.shape[3])
    _lib.companion_check(_lib.cellmaplib.fx_cellmap_apply(
        ctx.handle, int(sd), int(mapping), int(order), int(tab.shape[0]), int(tab.shape[-1]), int(tab.shape[2]), vdim,
        host_ptr(lo), host_ptr(hi), _dev_ptr(pts), _dev_ptr(corners), _dev_ptr(tab), _dev_ptr(out), _stream_ptr(stream)))
    return out


def cellmap_tensor_batch(sd, nodes, lo, hi, order, pts, corners, out, stream=None, grid=False, ctx=None):
    """The fused kernel of products of sd 1-D Lagrange factors (fx_cellmap_tensor_batch / _grid_batch): ``nodes`` host
    (sd, nn); pts (nreq, npts, sd), or with ``grid`` (nreq, sd, q); ``out`` (nreq, ntab, nn**sd, npts), written."""
    ctx = ctx or Context.get()
    entry = _lib.cellmaplib.fx_cellmap_tensor_grid_batch if grid else _lib.cellmaplib.fx_cellmap_tensor_batch
    _lib.companion_check(entry(ctx.handle, int(sd), int(nodes.shape[1]), host_ptr(nodes), host_ptr(lo), host_ptr(hi), int(order),
                               int(pts.shape[0]), int(pts.shape[2] if grid else pts.shape[1]), _dev_ptr(pts), _dev_ptr(corners),
                               _dev_ptr(out), _stream_ptr(stream)))
    return out
