/* fiat_amd_serendipity.h -- C ABI of libfiat_amd_serendipity.so: Serendipity elements S_k on quadrilaterals and
 * hexahedra (FIAT/serendipity.py), evaluated directly by HIP kernels for gfx950.
 *
 * A companion of libfiat_amd.so (fiat_amd.h): it links against it, so contexts (fx_ctx_create) and the error text
 * (fx_last_error) are shared, and the status codes are those of fiat_amd.h.  Plain C99.
 *
 * The element: every basis function of S_k is a signed product of one 1-D function per direction of the flattened cell
 * (FIAT/serendipity.py:180-225).  With v0, v1 the first and last vertex coordinate of a direction and h = v1 - v0:
 *   code 0      lambda0 = (v1 - x) / h
 *   code 1      lambda1 = (x - v0) / h
 *   code 2 + j  lambda0 lambda1 L_j(2 x - (v0 + v1)),  0 <= j <= k - 2   (L_j Legendre; the argument is the reference's
 *               x_mid, :73-77, which is not divided by h)
 * and a dof is a row (sign; code_x, code_y[, code_z]).  Rows come in the reference's order: vertices (v_lambda_0 :180-187),
 * edges (e_lambda_0 :190-200), faces (f_lambda_0 :203-216), interior (i_lambda_0 :219-225). */
#ifndef FIAT_AMD_SERENDIPITY_H
#define FIAT_AMD_SERENDIPITY_H

#include <stdint.h>

#include "fiat_amd.h" /* fx_ctx, FX_OK / FX_E* */

#ifdef __cplusplus
extern "C" {
#endif

/* 1 */
int fx_serendipity_abi_version(void);

/* Number of dofs of S_degree on the quadrilateral (sd 2) or hexahedron (sd 3); the length of the reference's s_list
 * (FIAT/serendipity.py:109-113).  Host only.  degree >= 1. */
int fx_serendipity_dims(int sd, int degree, int* ndof);

/* The dof table: rows[ndof][1 + sd] = (sign +1 / -1, code_x, code_y[, code_z]), the table the kernels are compiled
 * from (FIAT/serendipity.py:180-225).  Host only, any degree >= 1. */
int fx_serendipity_descriptor(int sd, int degree, int* rows);

/* Name of the kernel instance and the output route fx_serendipity_tabulate_batch takes for a shape:
 * "fxk::serendipity_kernel<sd,degree,order> image P=<requests per item>", "... stream P=..." or
 * "fxk::serendipity_generic<sd> stream P=...".  Host only.  FX_ENOTIMPL where no instance covers the shape. */
int fx_serendipity_kernel(int sd, int degree, int order, int npts, char* buf, int n);

/* Serendipity.tabulate (FIAT/serendipity.py:134-174) for nreq point sets at once, on the box [lo, hi] (host, [sd]: the
 * first and last vertex of the flattened cell, :69-80): pts device [nreq][npts][sd] -> out device
 * [nreq][ntab][ndof][npts], tables in mis() order, ntab = C(sd + order, sd).  Compile-time instances cover degree
 * 1..6 and order 0..2, a generic one degree <= 12 and order <= 3; FX_ENOTIMPL beyond, and for a request of 2^31 entries
 * or more; FX_EINVAL for bad arguments.  Nothing is launched on an error. */
int fx_serendipity_tabulate_batch(fx_ctx* ctx, int sd, int degree, const double* lo, const double* hi, int order,
                                  int64_t nreq, int npts, const double* pts, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
