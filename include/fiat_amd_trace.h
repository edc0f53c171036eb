/* fiat_amd_trace.h -- C ABI of libfiat_amd_trace.so: the H(div) trace element (FIAT/hdiv_trace.py), one fused HIP kernel for
 * gfx950 that identifies the facet of every point, evaluates the facet element there and writes the whole table.
 *
 * A companion of libfiat_amd.so (fiat_amd.h): it links against it, so contexts (fx_ctx_create) and the error text
 * (fx_last_error) are shared, and the status codes are those of fiat_amd.h.  Plain C99.
 *
 * The element: a cell with nfac facets that all carry the same discontinuous element of nf dofs on the facet simplex of
 * dimension fd (0: point, 1: interval, 2: triangle).  The table of a request is [nfac * nf][npts]: at a point on facet f the
 * rows f nf .. (f + 1) nf hold the facet element's values, every other row is zero.  The facet element is given by its
 * matrix C[nf][nf] over the kernel's expansion of the UFC facet simplex, nf = 1, degree + 1, (degree + 1)(degree + 2) / 2:
 *   fd 1: member p = P_p(2 x - 1), the Legendre polynomials;
 *   fd 2: member (p, q) at (p + q)(p + q + 1) / 2 + q = Dubiner's basis on the triangle WITHOUT its normalisation
 *         sqrt((2 p + 1)(p + q + 1)) (csrc/trace.hpp states the recurrence);
 *   fd 0: the constant 1. */
#ifndef FIAT_AMD_TRACE_H
#define FIAT_AMD_TRACE_H

#include <stdint.h>

#include "fiat_amd.h" /* fx_ctx, FX_OK / FX_E* */

#ifdef __cplusplus
extern "C" {
#endif

/* how the facet of a point is given */
#define FX_TRACE_IDENTIFY 0  /* by the kernel, from the point's barycentric coordinates on the cell, tolerance 1e-10 */
#define FX_TRACE_ONE_FACET 1 /* one facet for the whole call */
#define FX_TRACE_FACETS 2    /* one facet per request */

/* 1 */
int fx_trace_abi_version(void);

/* Name of the kernel instance, the output route and the requests per item fx_trace_tabulate_batch takes for a shape:
 * "fxk::trace_kernel<fd,degree> image P=<requests per item>" or "... stream P=..."; degree 7..12 run the run-time-degree
 * instance "fxk::trace_kernel<fd,-1>".  Host only.  FX_ENOTIMPL where no instance covers the shape. */
int fx_trace_kernel(int fd, int degree, int nfac, int npts, char* buf, int n);

/* HDivTrace.tabulate for nreq point sets at once -> out device [nreq][nfac * nf][npts].
 *   FX_TRACE_IDENTIFY:  pts device [nreq][npts][fd + 1] in cell coordinates, nfac = fd + 2 (simplices); lam0 (host, [fd + 2])
 *                       and G (host, [fd + 2][fd + 1]) give the barycentric coordinates lambda_i = lam0[i] + sum_d G[i][d] x_d,
 *                       vertex i opposite facet i (on the interval: the point where lambda_i vanishes is facet 1 - i).  A
 *                       request with a point that is not on exactly one facet is NaN throughout.
 *   FX_TRACE_ONE_FACET: pts device [nreq][npts][fd] in the coordinates of facet `facet`.
 *   FX_TRACE_FACETS:    the same with the facet of request r in facets[r] (device, 0 <= facets[r] < nfac: the caller checks;
 *                       a request whose number is out of range is written as NaN).
 * Arguments that a mode does not use may be null.  Compile-time instances cover degree 0..6, the run-time-degree instance
 * 7..12 (fd 0: degree 0); FX_ENOTIMPL beyond, and for a request of 2^31 entries or more; FX_EINVAL for bad arguments.
 * Nothing is launched on an error. */
int fx_trace_tabulate_batch(fx_ctx* ctx, int fd, int degree, int nfac, int mode, int facet, const int* facets, const double* C,
                            const double* lam0, const double* G, int64_t nreq, int npts, const double* pts, double* out,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif
