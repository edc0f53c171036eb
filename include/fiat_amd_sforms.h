/* fiat_amd_sforms.h -- C ABI of libfiat_amd_sforms.so: the vector-valued members of the serendipity complex on
 * quadrilaterals and hexahedra -- BDMCE / BDMCF (FIAT/brezzi_douglas_marini_cube.py) and the trimmed serendipity families
 * (FIAT/Sminus.py, SminusCurl.py, SminusDiv.py) -- evaluated from a term table by one HIP kernel for gfx950.
 *
 * A companion of libfiat_amd.so (fiat_amd.h): it links against it, so contexts (fx_ctx_create) and the error text
 * (fx_last_error) are shared, and the status codes are those of fiat_amd.h.  Plain C99.
 *
 * The element: every component of every basis function is zero or one term, a coefficient times one 1-D function per
 * direction of the flattened cell.  With v0, v1 the first and last vertex coordinate of a direction, h = v1 - v0,
 * t = 2 x - (v0 + v1) (the reference's x_mid, which is not divided by h) and L_j the Legendre polynomial, at degree k:
 *   code 0          lambda0 = (v1 - x) / h
 *   code 1          lambda1 = (x - v0) / h
 *   code 2 + j      L_j(t),                  0 <= j <= k
 *   code 3 + k + j  lambda0 lambda1 L_j(t),  0 <= j <= k
 * 2 k + 4 codes in all. */
#ifndef FIAT_AMD_SFORMS_H
#define FIAT_AMD_SFORMS_H

#include <stdint.h>

#include "fiat_amd.h" /* fx_ctx, FX_OK / FX_E* */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fx_sforms_element fx_sforms_element;

/* 1 */
int fx_sforms_abi_version(void);

/* The term table of an element of `degree` (1..6) with nrows basis functions on the quadrilateral (sd 2) or hexahedron
 * (sd 3), copied to the device of ctx: coef host [nrows][sd], 0 where the component is zero; codes host [nrows][sd][sd],
 * the code of direction d of component c of row i at [i][c][d] (ignored where the coefficient is zero).  FX_EINVAL for a
 * code outside the family or a coefficient that is not finite. */
int fx_sforms_element_create(fx_ctx* ctx, int sd, int degree, int nrows, const double* coef, const int* codes,
                             fx_sforms_element** out);
int fx_sforms_element_destroy(fx_sforms_element* el);

/* Name of the kernel instance, the output route, the requests per item and the image budget in bytes that
 * fx_sforms_tabulate_batch takes for a shape: "fxk::sforms_kernel<sd,order> image P=<p> budget=<bytes>" or
 * "... stream P=<p> budget=<bytes>".  An item of P requests goes through the per-wave LDS image where one request
 * (ntab * nrows * sd * npts doubles) fits the budget; P is then at most budget / request.  Host only. */
int fx_sforms_kernel(int sd, int degree, int nrows, int order, int npts, char* buf, int n);

/* tabulate() for nreq point sets at once, on the box [lo, hi] (host, [sd]: the first and last vertex of the flattened
 * cell): pts device [nreq][npts][sd] -> out device [nreq][ntab][nrows][sd][npts], tables in mis() order,
 * ntab = C(sd + order, sd), order 0..2.  Zero components are written as 0.0.  FX_ENOTIMPL beyond order 2 and for a
 * request of 2^31 entries or more; FX_EINVAL for bad arguments.  Nothing is launched on an error. */
int fx_sforms_tabulate_batch(fx_ctx* ctx, const fx_sforms_element* el, const double* lo, const double* hi, int order,
                             int64_t nreq, int npts, const double* pts, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
