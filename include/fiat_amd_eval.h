/* fiat_amd_eval.h -- C ABI of libfiat_amd_eval.so: finite element functions evaluated at points,
 *   out[r][t][j][v][q] = sum_i dofs[r][j][i] D^t phi_i[v](x_rq),
 * by a fused HIP kernel for gfx950 that never forms the table of the basis functions in device memory.
 *
 * A companion of libfiat_amd.so (fiat_amd.h): it links against it, so contexts (fx_ctx_create) and the error text
 * (fx_last_error) are shared, and the status codes and FX_MAP_* are those of fiat_amd.h.  Plain C99.
 *
 * The element: a polynomial set over the Dubiner expansion set of one simplex, coeffs[ndof][vdim][nexp] as fx_element_create
 * takes them (FIAT/polynomial_set.py:42-66).  The instance set: intervals, triangles and tetrahedra, degree 1..6, expansion
 * variant default or bubble, vdim 1 or sd, derivative order 0..2, 1..8 right-hand sides, the affine map and the covariant and
 * contravariant Piola maps.  Outside it the calls answer FX_ENOTIMPL, for malformed arguments FX_EINVAL. */
#ifndef FIAT_AMD_EVAL_H
#define FIAT_AMD_EVAL_H

#include <stdint.h>

#include "fiat_amd.h" /* fx_ctx, FX_OK / FX_E*, FX_VARIANT_*, FX_MAP_* */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fx_eval_element fx_eval_element;

/* 1 */
int fx_eval_abi_version(void);

/* The order in which the kernel's depth-first walk of the recurrence meets the members: members[k] = index in the expansion set
 * of the k-th member of the walk, k < nexp = C(degree + sd, sd).  Host only. */
int fx_eval_walk_order(int sd, int degree, int* members);

/* The coefficients the kernel reads, folded[ndof][vdim][nexp]: over the raw recurrence (bubble variant: coeffs times the C0
 * transform of fx_plan_c0_transform), columns in the order of the walk.  Host only. */
int fx_eval_fold(int sd, int degree, int variant, int ndof, int vdim, const double* coeffs, double* folded);

/* An element on the device: scale is the first-member scale of the expansion set (<= 0: the default), cell the host vertices
 * [(sd + 1)][sd] of the element's own cell (NULL: the UFC simplex), coeffs host [ndof][vdim][nexp].  The folded coefficients
 * and the step table of the walk are uploaded here. */
int fx_eval_element_create(fx_ctx* ctx, int sd, int degree, int variant, double scale, const double* cell, int ndof, int vdim,
                           const double* coeffs, fx_eval_element** elem);
int fx_eval_element_destroy(fx_eval_element* elem);

/* Name of the kernel instance and the item scheme fx_eval_batch takes for a shape:
 * "fxk::eval_kernel<sd,order,vdim> degree=<n> P=<whole requests per item> chunks=<point chunks per request>".  Host only. */
int fx_eval_kernel(int sd, int degree, int order, int vdim, int ndof, int npts, int nrhs, char* buf, int n);

/* pts device [nreq][npts][sd]; verts device [nreq][sd + 1][sd], the requests' cells, or NULL for the element's own cell;
 * dofs device [nreq][nrhs][ndof] -> out device [nreq][ntab][nrhs][vdim][npts], tables in mis() order, ntab = C(sd + order, sd).
 * With verts the derivatives are taken with respect to the physical coordinates; mapping FX_MAP_COVARIANT_PIOLA /
 * FX_MAP_CONTRAVARIANT_PIOLA (vdim == sd >= 2, needs verts) pushes the values forward as fx_pushforward_batch does.
 * FX_ENOTIMPL outside the instance set and for a request of 2^31 entries or more; FX_EINVAL for bad arguments.  Nothing is
 * launched on an error.  The work is ordered on `stream`. */
int fx_eval_batch(fx_ctx* ctx, const fx_eval_element* elem, int mapping, int order, int64_t nreq, int npts, int nrhs,
                  const double* pts, const double* verts, const double* dofs, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
