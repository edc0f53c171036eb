/* fiat_amd_dpc.h -- C ABI of libfiat_amd_dpc.so: DPC elements on quadrilaterals and hexahedra
 * (FIAT/discontinuous_pc.py), evaluated in closed form by HIP kernels for gfx950.
 *
 * A companion of libfiat_amd.so (fiat_amd.h): it links against it, so contexts (fx_ctx_create) and the error text
 * (fx_last_error) are shared, and the status codes are those of fiat_amd.h.  Plain C99.
 *
 * The element: DPC_k is P_k, dual to point evaluation at the equispaced degree-k lattice of a simplex that an affine map
 * places over the cube (DPCDualSet, FIAT/discontinuous_pc.py:59-73).  With lambda the barycentric coordinates of that
 * simplex, lambda_i(x) = lam0[i] + sum_d G[i][d] x_d, the basis function of the lattice point alpha / k is
 *   phi_alpha(x) = prod_{i = 0..sd} l_{alpha_i}(lambda_i(x)),   l_a(t) = prod_{j < a} (k t - j) / (j + 1),
 * and a dof is a row alpha (sd + 1 non-negative entries of sum k).  Rows come in the reference's node order: the
 * vertices, edges, faces and interior of the UFC simplex, each with the interior lattice of make_points. */
#ifndef FIAT_AMD_DPC_H
#define FIAT_AMD_DPC_H

#include <stdint.h>

#include "fiat_amd.h" /* fx_ctx, FX_OK / FX_E* */

#ifdef __cplusplus
extern "C" {
#endif

/* 1 */
int fx_dpc_abi_version(void);

/* The dof table: rows[ndof][sd + 1] = alpha, ndof = C(degree + sd, sd), the table the kernels are compiled from.
 * Host only, sd 2 or 3, 1 <= degree <= 64. */
int fx_dpc_descriptor(int sd, int degree, int* rows);

/* Name of the kernel instance, the output route and the requests per item fx_dpc_tabulate_batch takes for a shape:
 * "fxk::dpc_kernel<sd,degree,order> image P=<requests per item>" or "... stream P=...".  Host only.  FX_ENOTIMPL where
 * no instance covers the shape. */
int fx_dpc_kernel(int sd, int degree, int order, int npts, char* buf, int n);

/* DPC.tabulate for nreq point sets at once: lam0 (host, [sd + 1]) and G (host, [sd + 1][sd]) are the barycentric
 * coordinates of the mapped simplex, the inverse of its matrix of homogeneous vertex coordinates; pts device
 * [nreq][npts][sd] -> out device [nreq][ntab][ndof][npts], tables in mis() order, ntab = C(sd + order, sd).
 * Compile-time instances cover degree 1..6 and order 0..2; FX_ENOTIMPL beyond, and for a request of 2^31 entries or
 * more; FX_EINVAL for bad arguments.  Nothing is launched on an error. */
int fx_dpc_tabulate_batch(fx_ctx* ctx, int sd, int degree, const double* lam0, const double* G, int order, int64_t nreq,
                          int npts, const double* pts, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
