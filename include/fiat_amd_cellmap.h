/* fiat_amd_cellmap.h -- C ABI of libfiat_amd_cellmap.so: tabulation on physical quadrilaterals and hexahedra through the
 * multilinear (Q1) map, by HIP kernels for gfx950.
 *
 * A companion of libfiat_amd.so (fiat_amd.h): it links against it, so contexts (fx_ctx_create) and the error text
 * (fx_last_error) are shared, and the status codes and FX_MAP_* are those of fiat_amd.h.  Plain C99.
 *
 * The map.  [lo, hi] is the element's own axis-aligned box, xi_d = (X_d - lo_d) / (hi_d - lo_d), corners[i] the image of
 * the box's vertex i (bit sd-1-d of i belongs to coordinate d: the last coordinate runs fastest, (0,0), (0,1), (1,0), (1,1)
 * on the unit square),
 *   x(X) = sum_i N_i(xi) corners[i],  N_i = prod_d (bit_d(i) ? xi_d : 1 - xi_d),  J_ad = dx_a / dX_d,  G = J^-1.
 * Tables: table 0 holds values, table 1 + d the derivative with respect to the PHYSICAL coordinate x_d,
 *   FX_MAP_AFFINE               out_0 = Phi,  out_{1+d} = sum_e d_e Phi G_ed, component by component
 *   FX_MAP_COVARIANT_PIOLA      phi = M Phi, M = G^T;          d phi / dx_d = sum_e G_ed (d_e M Phi + M d_e Phi)
 *   FX_MAP_CONTRAVARIANT_PIOLA  phi = M Phi, M = J / det J (signed determinant); the same gradient
 * with d_e G = -G (d_e J) G and d_e det J = det J tr(G d_e J): the full gradient of the mapped field (d_e M does not vanish
 * on a cell that is no parallelogram / parallelepiped).  A cell whose map is singular at a point gives non-finite entries at
 * that point; nothing inspects the cells.  Derivative order 0 or 1 (FX_ENOTIMPL beyond: it needs more derivatives of the
 * map).  lo, hi and nodes are host pointers, everything else device pointers; nothing is launched on an error. */
#ifndef FIAT_AMD_CELLMAP_H
#define FIAT_AMD_CELLMAP_H

#include <stdint.h>

#include "fiat_amd.h" /* fx_ctx, FX_OK / FX_E*, FX_MAP_* */

#ifdef __cplusplus
extern "C" {
#endif

/* 1 */
int fx_cellmap_abi_version(void);

/* Name of the kernel instance and the route of a shape.  Host only.
 * nn == 0: the general pass, "fxk::cellmap_apply_kernel<sd,order,mapping> affine|covariant|contravariant P=<requests per
 * item>".  nn >= 1: the fused kernel of products of sd 1-D Lagrange factors of nn nodes (mapping FX_MAP_AFFINE, vdim 1;
 * nrows is not read), "fxk::cellmap_tensor_kernel<sd,nn,order,true|false> image|stream P=<requests per item>"; with grid != 0
 * npts is the number of 1-D coordinates per direction.  FX_ENOTIMPL where no instance covers the shape. */
int fx_cellmap_kernel(int sd, int nn, int mapping, int order, int nrows, int vdim, int npts, int grid, char* buf, int n);

/* pts [nreq][npts][sd], corners [nreq][2^sd][sd] -> x [nreq][npts][sd], J [nreq][npts][sd][sd], detJ [nreq][npts] (signed). */
int fx_cellmap_geometry(fx_ctx* ctx, int sd, const double* lo, const double* hi, int64_t nreq, int npts, const double* pts,
                        const double* corners, double* x, double* J, double* detJ, void* stream);

/* The general pass over reference tables in [nreq][ntab][nrows][vdim][npts] (ntab = 1 + sd * order, vdim 1 or sd; a Piola
 * map needs vdim == sd: FX_EINVAL otherwise) -> out, the same layout.  out may equal in: a lane reads every entry of a row
 * at its point before it writes one.  In place, order 0 and FX_MAP_AFFINE change nothing and launch nothing.  FX_EINVAL for
 * a request of 2^31 entries or more. */
int fx_cellmap_apply(fx_ctx* ctx, int sd, int mapping, int order, int64_t nreq, int npts, int nrows, int vdim, const double* lo,
                     const double* hi, const double* pts, const double* corners, const double* in, double* out, void* stream);

/* Products of sd 1-D Lagrange factors with nn nodes each (nodes host [sd][nn], any distinct nodes; 2 <= nn <= 5, FX_ENOTIMPL
 * beyond), fused: pts [nreq][npts][sd] in the element's coordinates -> out [nreq][ntab][nn^sd][npts], dofs row-major over
 * the factors, physical derivatives.  No reference table reaches device memory.  The node data of a set of factors is
 * uploaded at the first call that names it (hipMalloc and a synchronous copy: make that call outside a stream capture) and
 * kept; the library keeps at most 64 sets, and a further new set waits for the device, frees them all and starts again. */
int fx_cellmap_tensor_batch(fx_ctx* ctx, int sd, int nn, const double* nodes, const double* lo, const double* hi, int order,
                            int64_t nreq, int npts, const double* pts, const double* corners, double* out, void* stream);

/* The same from per-request 1-D coordinates grid [nreq][sd][q] of a tensor grid: npts = q^sd, points row-major (j0, j1[, j2]);
 * FX_EINVAL where q^sd is 2^31 or more. */
int fx_cellmap_tensor_grid_batch(fx_ctx* ctx, int sd, int nn, const double* nodes, const double* lo, const double* hi, int order,
                                 int64_t nreq, int q, const double* grid, const double* corners, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
