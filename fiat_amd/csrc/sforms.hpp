// BDMCE / BDMCF and the trimmed serendipity H(curl) / H(div) families on quadrilaterals and hexahedra, evaluated from a
// term table (gfx950).
//
// Reference behaviour: the tabulate methods of FIAT/brezzi_douglas_marini_cube.py:93-137, FIAT/Sminus.py:124-151,
// FIAT/SminusCurl.py:102-130 and FIAT/SminusDiv.py:98-126 differentiate a sympy array of the basis functions and evaluate
// it point by point.  Every component of every one of those functions is zero or ONE term: a coefficient times one 1-D
// function per direction.  On direction d of the flattened cell, with v0, v1 the first and last vertex coordinate,
// h = v1 - v0, lambda0 = (v1 - x) / h, lambda1 = (x - v0) / h, b = lambda0 lambda1, t = 2 x - (v0 + v1) (the reference's
// x_mid: NOT divided by h), the function of
//   code 0 is lambda0,  code 1 lambda1,  code 2 + j  L_j(t),  code 3 + K + j  b L_j(t)   (Legendre, 0 <= j <= K),
// NF = 2 K + 4 functions.  The element is data: per (dof, component) a coefficient (0: the component is zero) and the packed
// codes.  The table of alpha is  coef * prod_d (d/dx)^alpha_d f_code_d (x_d).
//
// Lane <-> (request, point), as serendipity_kernel and hdivcurl_kernel.  The codes are run-time values (wave-uniform), so
// the lane keeps its 1-D tables F[d][m][c] lane-minor in LDS (a run-time-indexed private array would go to scratch), then
// walks tables, dofs and components: a nonzero entry is the coefficient times SD LDS reads, a zero entry is stored without
// reads.  An item is P whole requests (P * npts <= 64; one request in chunks of 64 points beyond).  Where it fits the image
// budget it goes through a per-wave LDS image behind the 1-D tables and leaves as whole-line non-temporal stores
// (store.hpp flush_item); larger requests stream: every lane stores its own entries with plain stores.
#pragma once
#include <hip/hip_runtime.h>

#include "line_basis.hpp"
#include "store.hpp"

namespace fxk {

constexpr int SF_MAXK = 6, SF_MAXORDER = 2;
constexpr int SF_CHUNK = 4;  // entries of the term table fetched together; the device table is padded to a multiple
// LDS of one (one-wave) workgroup: the 1-D tables, then the image.  While the tables leave room the workgroup stays at
// 40 KB (four per CU, one per SIMD); larger tables keep a 16 KB image, which bounds the workgroup by
// 64 KB (two per CU at the worst).
constexpr int SF_WG_BYTES = 40 * 1024, SF_MIN_IMAGE_BYTES = 16 * 1024;

__host__ __device__ constexpr int sf_ncodes(int k) { return 2 * k + 4; }
__host__ __device__ constexpr int sf_pack(int cx, int cy, int cz) { return cx | cy << 8 | cz << 16; }
__host__ __device__ constexpr int sf_code(int packed, int d) { return (packed >> (8 * d)) & 0xff; }
__host__ __device__ constexpr size_t sf_tables_bytes(int sd, int degree, int order) {
    return (size_t)sd * (order + 1) * sf_ncodes(degree) * 64 * 8;
}
__host__ __device__ constexpr int sf_image_budget(int sd, int degree, int order) {
    const long long room = (long long)SF_WG_BYTES - (long long)sf_tables_bytes(sd, degree, order);
    return room > SF_MIN_IMAGE_BYTES ? (int)room : SF_MIN_IMAGE_BYTES;
}

struct SfArgs {
    const double* pts;   // [nreq][npts][sd]
    double* out;         // [nreq][ntab][nrows][sd][npts]
    const double* coef;  // [nrows * sd] padded with zeros to a multiple of SF_CHUNK, 0: the entry is zero
    const int* codes;    // [nrows * sd] padded likewise, sf_pack
    double v0[3], v1[3];
    long long nreq, nitems;
    int npts, nrows, ntab;
    int P;               // whole requests per item
    int image;           // 1: per-wave LDS image of the item, 0: streaming stores
    int degree;
};

// this lane's 1-D tables of one direction: Td[(m nf + c) 64] = m-th derivative in x of the function of code c
template <int ORDER>
__device__ __forceinline__ void sf_line(double x, double v0, double v1, int K, double* Td) {
    const int nf = sf_ncodes(K);
    const double ih = 1.0 / (v1 - v0);
    const double l0 = (v1 - x) * ih, l1 = (x - v0) * ih;
    const double t = 2.0 * x - (v0 + v1);
    const double b = l0 * l1, b1 = -t * ih * ih, b2 = -2.0 * ih * ih;  // b, b', b''
#pragma unroll
    for (int m = 0; m <= ORDER; ++m) {
        Td[(m * nf + 0) * 64] = m == 0 ? l0 : (m == 1 ? -ih : 0.0);
        Td[(m * nf + 1) * 64] = m == 0 ? l1 : (m == 1 ? ih : 0.0);
    }
    // L_j and its derivatives in t, rolling (constant indices: registers)
    double Lp[ORDER + 1], Lc[ORDER + 1];  // L_{j-1}, L_j
#pragma unroll
    for (int m = 0; m <= ORDER; ++m) {
        Lp[m] = 0.0;
        Lc[m] = m == 0 ? 1.0 : 0.0;
    }
    for (int j = 0; j <= K; ++j) {
        // dt/dx = 2: (d/dx)^m L_j(t) = 2^m L_j^(m);  Leibniz for b L_j
        Td[(2 + j) * 64] = Lc[0];
        Td[(3 + K + j) * 64] = b * Lc[0];
        if constexpr (ORDER >= 1) {
            Td[(nf + 2 + j) * 64] = 2.0 * Lc[1];
            Td[(nf + 3 + K + j) * 64] = 2.0 * b * Lc[1] + b1 * Lc[0];
        }
        if constexpr (ORDER >= 2) {
            Td[(2 * nf + 2 + j) * 64] = 4.0 * Lc[2];
            Td[(2 * nf + 3 + K + j) * 64] = 4.0 * b * Lc[2] + 4.0 * b1 * Lc[1] + b2 * Lc[0];
        }
        // (j + 1) L_{j+1}^(m) = (2 j + 1) (t L_j^(m) + m L_j^(m-1)) - j L_{j-1}^(m)
        const double c1 = (double)(2 * j + 1), c2 = (double)j, inv = 1.0 / (double)(j + 1);
        double Ln[ORDER + 1];
#pragma unroll
        for (int m = 0; m <= ORDER; ++m) {
            double s = t * Lc[m];
            if (m > 0) s += (double)m * Lc[m > 0 ? m - 1 : 0];
            Ln[m] = (c1 * s - c2 * Lp[m]) * inv;
        }
#pragma unroll
        for (int m = 0; m <= ORDER; ++m) {
            Lp[m] = Lc[m];
            Lc[m] = Ln[m];
        }
    }
}

template <int SD, int ORDER>
__global__ __launch_bounds__(64) void sforms_kernel(const SfArgs a) {
    static_assert(SD == 2 || SD == 3, "quadrilaterals and hexahedra");
    static_assert(ORDER >= 0 && ORDER <= SF_MAXORDER, "derivative order");
    constexpr int NTAB = TensorAlpha<SD, ORDER>::NTAB;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int lane = threadIdx.x & 63;
    const int K = a.degree, npts = a.npts;
    const int nf = sf_ncodes(K);
    const int nent = a.nrows * SD;                   // entries (dof, component) of a table
    const int dstride = (ORDER + 1) * nf * 64;       // doubles of one direction's tables
    double* T = lds + lane;
    double* image = lds + SD * dstride;
    const long long reqsize = (long long)NTAB * nent * npts;
    for (long long item = blockIdx.x; item < a.nitems; item += gridDim.x) {
        const long long r0 = item * a.P;
        const long long left = a.nreq - r0;
        const int Pcur = left < a.P ? (int)left : a.P;
        const int nslots = Pcur * npts;
        double* gout = a.out + (size_t)r0 * reqsize;
        for (int s0 = 0; s0 < nslots; s0 += 64) {
            const int slot = s0 + lane;
            if (slot >= nslots) continue;
            const int rl = slot / npts;
            const int pl = slot - rl * npts;
            const double* p = a.pts + ((size_t)(r0 + rl) * npts + pl) * SD;
            sf_line<ORDER>(p[0], a.v0[0], a.v1[0], K, T);
            sf_line<ORDER>(p[1], a.v0[1], a.v1[1], K, T + dstride);
            if constexpr (SD == 3) sf_line<ORDER>(p[2], a.v0[2], a.v1[2], K, T + 2 * dstride);
            double* dst = (a.image ? image : gout) + (size_t)rl * reqsize + pl;
            // tables in mis() order: total order o, then (a0, a1[, a2]) with a0 descending.  Rolled loops: the walk over
            // the entries is the long one, and unrolled tables would keep a pointer triple per table live.
#pragma unroll 1
            for (int o = 0; o <= ORDER; ++o) {
#pragma unroll 1
                for (int i = 0; i <= o; ++i) {
#pragma unroll 1
                    for (int j = 0; j <= (SD == 3 ? i : 0); ++j) {
                        const int a0 = o - i, a1 = SD == 3 ? i - j : i, a2 = j;
                        const double* R0 = T + a0 * nf * 64;
                        const double* R1 = T + dstride + a1 * nf * 64;
                        const double* R2 = T + 2 * dstride + a2 * nf * 64;
                        // SF_CHUNK entries at a time: their coefficients and codes (wave-uniform: scalar loads; the table
                        // is padded to a whole chunk) are fetched together, ahead of the LDS reads they steer
                        for (int e0 = 0; e0 < nent; e0 += SF_CHUNK) {
                            double c[SF_CHUNK];
                            int k[SF_CHUNK];
#pragma unroll
                            for (int u = 0; u < SF_CHUNK; ++u) {
                                c[u] = a.coef[e0 + u];
                                k[u] = a.codes[e0 + u];
                            }
#pragma unroll
                            for (int u = 0; u < SF_CHUNK; ++u) {
                                if (e0 + u < nent) {
                                    double v = 0.0;
                                    if (c[u] != 0.0) {
                                        v = c[u] * R0[sf_code(k[u], 0) * 64] * R1[sf_code(k[u], 1) * 64];
                                        if constexpr (SD == 3) v *= R2[sf_code(k[u], 2) * 64];
                                    }
                                    *dst = v;
                                    dst += npts;
                                }
                            }
                        }
                    }
                }
            }
        }
        if (a.image) flush_item(gout, image, (long long)Pcur * reqsize, lane);
    }
}

}  // namespace fxk
