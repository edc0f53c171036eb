/* fiat_amd_hier.h -- C ABI of libfiat_amd_hier.so: IntegratedLegendre on intervals, triangles and tetrahedra
 * (FIAT/hierarchical.py), tabulated directly from the C0 hierarchy by HIP kernels for gfx950.
 *
 * A companion of libfiat_amd.so (fiat_amd.h): it links against it, so contexts (fx_ctx_create) and the error text
 * (fx_last_error) are shared, and the status codes are those of fiat_amd.h.  Plain C99.
 *
 * The element: the nodal basis of IntegratedLegendre(k) is the C0 hierarchy of the bubble-variant expansion set
 * (FIAT/expansions.py:140-322), member by member, times a scale that depends on the dimension of the dof's entity only.  A
 * dof is a member, named by its lattice index (p, q, r) with p + q + r <= k (trailing entries 0 below three dimensions).
 * Rows come in the reference's order: vertices, edges, faces, interior. */
#ifndef FIAT_AMD_HIER_H
#define FIAT_AMD_HIER_H

#include <stdint.h>

#include "fiat_amd.h" /* fx_ctx, FX_OK / FX_E* */

#ifdef __cplusplus
extern "C" {
#endif

/* 1 */
int fx_hier_abi_version(void);

/* The dof table: rows[ndof][4] = (p, q, r, dimension of the dof's entity), ndof = C(degree + sd, sd), the table the
 * kernels are compiled from.  Host only, sd 1..3, 1 <= degree <= 64. */
int fx_hier_descriptor(int sd, int degree, int* rows);

/* Name of the kernel instance, the output route and the requests per item fx_hier_tabulate_batch takes for a shape:
 * "fxk::hier_kernel<sd,degree,order> image P=<requests per item>" or "... stream P=...".  Host only.  FX_ENOTIMPL where
 * no instance covers the shape. */
int fx_hier_kernel(int sd, int degree, int order, int npts, char* buf, int n);

/* IntegratedLegendre.tabulate for nreq point sets at once: scales (host, [4]) per entity dimension (entries beyond sd are
 * not read); pts device [nreq][npts][sd] -> out device [nreq][ntab][ndof][npts], tables in mis() order,
 * ntab = C(sd + order, sd); X = A x + b (host, A [sd][sd] row-major, b [sd]) maps the element's cell onto the simplex with
 * vertices (-1, ..., -1), (1, -1, ..., -1), ...  Compile-time instances cover sd 1..3, degree 1..6 and order 0..2;
 * FX_ENOTIMPL beyond, and for a request of 2^31 entries or more; FX_EINVAL for bad arguments.  Nothing is launched on an
 * error. */
int fx_hier_tabulate_batch(fx_ctx* ctx, int sd, int degree, int order, const double* scales, const double* pts, int64_t nreq,
                           int npts, double* out, void* stream, const double* A, const double* b);

#ifdef __cplusplus
}
#endif
#endif
