// Tabulation on physical quadrilaterals and hexahedra through the multilinear (Q1) map (gfx950).
//
// The map: with [lo, hi] the element's own box, xi_d = (X_d - lo_d) / (hi_d - lo_d) and v_i the images of the box's vertices
// (vertex i: bit SD-1-d of i belongs to coordinate d, so the last coordinate runs fastest),
//   x(X) = sum_i N_i(xi) v_i,   N_i = prod_d (bit_d(i) ? xi_d : 1 - xi_d),   J_ad = dx_a / dX_d,   G = J^-1.
// J is not constant on such a cell, so everything below is per point.  Tables of derivative order 1 come out with respect
// to the PHYSICAL coordinates: for a scalar (or component by component, "affine") d/dx_d = sum_e G_ed d/dX_e; for the Piola
// maps phi = M Phi with M = G^T (covariant) or J / det J (contravariant, signed determinant), and the gradient is that of
// the mapped field, d phi / dx_d = sum_e G_ed (d_e M . Phi + M . d_e Phi) with d_e G = -G (d_e J) G,
// d_e det J = det J tr(G d_e J), d_e J = sum_i v_i d_e grad N_i (no second derivative in one direction: N_i is multilinear).
//
// Three kernels, lane <-> (request, point) in all of them (an item is P whole requests, P * npts <= 64; one request in
// chunks of 64 points beyond):
//   cellmap_geometry_kernel<SD>                   x, J, det J of every point
//   cellmap_apply_kernel<SD, ORDER, MAP>          the general pass over any reference table [nreq][ntab][nrows][vdim][npts]:
//       the lane computes G, det J and d_e M once, then walks the rows; for a row it reads all ntab * vdim entries at its
//       point before it writes any of them, so the pass may run in place
//   cellmap_tensor_kernel<SD, NN, ORDER, GRID>    products of SD 1-D Lagrange factors of NN nodes each, fused: the lane
//       evaluates the factors and their derivatives in registers (line_basis.hpp) and G from the corners, and writes the
//       physical tables directly; output route as hdivcurl_kernel (per-wave LDS image and flush_item, or streamed rows)
#pragma once
#include <hip/hip_runtime.h>

#include "line_basis.hpp"
#include "store.hpp"

namespace fxk {

constexpr int CM_AFFINE = 0, CM_COVARIANT = 1, CM_CONTRAVARIANT = 2;  // FX_MAP_* of fiat_amd.h
constexpr int CM_IMAGE_BYTES = 40 * 1024;  // largest per-wave LDS image; larger items stream
constexpr int CM_MINNN = 2, CM_MAXNN = 5, CM_MAXORDER = 1;
constexpr int CM_LINE = CM_MAXNN * (2 + CM_MAXNN);  // doubles of one factor: nodes, weights, differentiation matrix

template <int SD> struct CmGeom {
    double x[SD];
    double J[SD][SD];  // J[a][d] = dx_a / dX_d
    double G[SD][SD];  // J^-1
    double det;        // signed
};

// x and J at xi from the corners V[2^SD][SD] of one request; ih[d] = 1 / (hi_d - lo_d).  SECOND: H[a][e][f] = d2 x_a / dX_e dX_f
// too (e != f; the diagonal is zero and is not touched).
template <int SD, bool SECOND>
__device__ __forceinline__ void cm_map(const double (&xi)[SD], const double* V, const double (&ih)[SD], CmGeom<SD>& g,
                                       double (&H)[SD][SD][SD]) {
    double f[SD][2];
#pragma unroll
    for (int d = 0; d < SD; ++d) {
        f[d][0] = 1.0 - xi[d];
        f[d][1] = xi[d];
    }
#pragma unroll
    for (int a = 0; a < SD; ++a) {
        g.x[a] = 0.0;
#pragma unroll
        for (int e = 0; e < SD; ++e) {
            g.J[a][e] = 0.0;
#pragma unroll
            for (int h = 0; h < SD; ++h) H[a][e][h] = 0.0;
        }
    }
#pragma unroll
    for (int i = 0; i < (1 << SD); ++i) {
        int b[SD];
#pragma unroll
        for (int d = 0; d < SD; ++d) b[d] = (i >> (SD - 1 - d)) & 1;
        double N = 1.0, dN[SD], d2N[SD][SD];
#pragma unroll
        for (int d = 0; d < SD; ++d) N *= f[d][b[d]];
#pragma unroll
        for (int e = 0; e < SD; ++e) {
            double p = b[e] ? ih[e] : -ih[e];
#pragma unroll
            for (int d = 0; d < SD; ++d)
                if (d != e) p *= f[d][b[d]];
            dN[e] = p;
#pragma unroll
            for (int h = 0; h < SD; ++h) {
                double q = (b[e] == b[h] ? 1.0 : -1.0) * ih[e] * ih[h];
#pragma unroll
                for (int d = 0; d < SD; ++d)
                    if (d != e && d != h) q *= f[d][b[d]];
                d2N[e][h] = e == h ? 0.0 : q;
            }
        }
#pragma unroll
        for (int a = 0; a < SD; ++a) {
            const double v = V[i * SD + a];
            g.x[a] += N * v;
#pragma unroll
            for (int e = 0; e < SD; ++e) {
                g.J[a][e] += dN[e] * v;
                if constexpr (SECOND) {
#pragma unroll
                    for (int h = 0; h < SD; ++h)
                        if (h != e) H[a][e][h] += d2N[e][h] * v;
                }
            }
        }
    }
}

// G = J^-1 and det J by cofactors; a singular J gives non-finite entries, nothing is inspected
template <int SD> __device__ __forceinline__ void cm_invert(CmGeom<SD>& g) {
    if constexpr (SD == 2) {
        g.det = g.J[0][0] * g.J[1][1] - g.J[0][1] * g.J[1][0];
        const double r = 1.0 / g.det;
        g.G[0][0] = g.J[1][1] * r;
        g.G[0][1] = -g.J[0][1] * r;
        g.G[1][0] = -g.J[1][0] * r;
        g.G[1][1] = g.J[0][0] * r;
    } else {
        double C[3][3];  // cofactors
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int r0 = (i + 1) % 3, r1 = (i + 2) % 3, c0 = (j + 1) % 3, c1 = (j + 2) % 3;
                C[i][j] = g.J[r0][c0] * g.J[r1][c1] - g.J[r0][c1] * g.J[r1][c0];
            }
        g.det = g.J[0][0] * C[0][0] + g.J[0][1] * C[0][1] + g.J[0][2] * C[0][2];
        const double r = 1.0 / g.det;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) g.G[i][j] = C[j][i] * r;
    }
}

// the Piola matrix M and, ORDER >= 1, its derivatives dM[e] = dM / dX_e
template <int SD, int ORDER, int MAP>
__device__ __forceinline__ void cm_piola(const CmGeom<SD>& g, const double (&H)[SD][SD][SD], double (&M)[SD][SD],
                                         double (&dM)[SD][SD][SD]) {
    const double rdet = 1.0 / g.det;
#pragma unroll
    for (int c = 0; c < SD; ++c)
#pragma unroll
        for (int k = 0; k < SD; ++k) M[c][k] = MAP == CM_COVARIANT ? g.G[k][c] : g.J[c][k] * rdet;
    if constexpr (ORDER >= 1) {
#pragma unroll
        for (int e = 0; e < SD; ++e) {
            // (d_e J)[a][d] = H[a][d][e]; GdJ = G d_e J
            double GdJ[SD][SD];
#pragma unroll
            for (int i = 0; i < SD; ++i)
#pragma unroll
                for (int d = 0; d < SD; ++d) {
                    double s = 0.0;
#pragma unroll
                    for (int a = 0; a < SD; ++a)
                        if (d != e) s += g.G[i][a] * H[a][d][e];
                    GdJ[i][d] = s;
                }
            if constexpr (MAP == CM_COVARIANT) {
                // d_e G = -(G d_e J) G;  M = G^T
#pragma unroll
                for (int c = 0; c < SD; ++c)
#pragma unroll
                    for (int k = 0; k < SD; ++k) {
                        double s = 0.0;
#pragma unroll
                        for (int d = 0; d < SD; ++d) s += GdJ[k][d] * g.G[d][c];
                        dM[e][c][k] = -s;
                    }
            } else {
                double tr = 0.0;
#pragma unroll
                for (int i = 0; i < SD; ++i) tr += GdJ[i][i];
#pragma unroll
                for (int c = 0; c < SD; ++c)
#pragma unroll
                    for (int k = 0; k < SD; ++k) dM[e][c][k] = ((k != e ? H[c][k][e] : 0.0) - g.J[c][k] * tr) * rdet;
            }
        }
    }
}

// ---- geometry -----------------------------------------------------------------------------------------------------------
struct CmGeomArgs {
    const double* pts;      // [nreq][npts][sd]
    const double* corners;  // [nreq][2^sd][sd]
    double *x, *J, *det;    // [nreq][npts][sd], [nreq][npts][sd][sd], [nreq][npts]
    double lo[3], h[3];     // the element's box: lower corner and edge lengths
    long long total;        // nreq * npts
    int npts;
};

template <int SD> __global__ __launch_bounds__(64) void cellmap_geometry_kernel(const CmGeomArgs a) {
    double ih[SD];
#pragma unroll
    for (int d = 0; d < SD; ++d) ih[d] = 1.0 / a.h[d];
    for (long long s = (long long)blockIdx.x * 64 + (threadIdx.x & 63); s < a.total; s += (long long)gridDim.x * 64) {
        const long long r = s / a.npts;
        double xi[SD];
#pragma unroll
        for (int d = 0; d < SD; ++d) xi[d] = (a.pts[(size_t)s * SD + d] - a.lo[d]) / a.h[d];
        CmGeom<SD> g;
        double H[SD][SD][SD];
        cm_map<SD, false>(xi, a.corners + (size_t)r * (SD << SD), ih, g, H);
        cm_invert<SD>(g);
#pragma unroll
        for (int i = 0; i < SD; ++i) {
            a.x[(size_t)s * SD + i] = g.x[i];
#pragma unroll
            for (int d = 0; d < SD; ++d) a.J[((size_t)s * SD + i) * SD + d] = g.J[i][d];
        }
        a.det[s] = g.det;
    }
}

// ---- the general pass ---------------------------------------------------------------------------------------------------
struct CmApplyArgs {
    const double* pts;      // [nreq][npts][sd]
    const double* corners;  // [nreq][2^sd][sd]
    const double* in;       // [nreq][ntab][nrows][vdim][npts]: reference tables
    double* out;            // the same layout; may be `in`
    double lo[3], h[3];
    long long nreq, nitems;
    int npts, nrows, vdim;
    int P;                  // whole requests per item
};

template <int SD, int ORDER, int MAP>
__global__ __launch_bounds__(64) void cellmap_apply_kernel(const CmApplyArgs a) {
    static_assert(SD == 2 || SD == 3, "quadrilaterals and hexahedra");
    static_assert(ORDER >= 0 && ORDER <= CM_MAXORDER && MAP >= CM_AFFINE && MAP <= CM_CONTRAVARIANT, "compile-time instances");
    constexpr int NTAB = 1 + SD * ORDER;
    const int lane = threadIdx.x & 63;
    const int npts = a.npts;
    const size_t rstride = (size_t)a.vdim * npts;      // doubles per row
    const size_t tstride = (size_t)a.nrows * rstride;  // per table (a request has fewer than 2^31 entries)
    double ih[SD];
#pragma unroll
    for (int d = 0; d < SD; ++d) ih[d] = 1.0 / a.h[d];
    for (long long item = blockIdx.x; item < a.nitems; item += gridDim.x) {
        const long long r0 = item * a.P;
        const long long left = a.nreq - r0;
        const int Pcur = left < a.P ? (int)left : a.P;
        const int nslots = Pcur * npts;
        for (int s0 = 0; s0 < nslots; s0 += 64) {
            const int slot = s0 + lane;
            if (slot >= nslots) continue;
            const int rl = slot / npts;
            const int pl = slot - rl * npts;
            const long long r = r0 + rl;
            double xi[SD];
#pragma unroll
            for (int d = 0; d < SD; ++d) xi[d] = (a.pts[((size_t)r * npts + pl) * SD + d] - a.lo[d]) / a.h[d];
            CmGeom<SD> g;
            double H[SD][SD][SD];
            cm_map<SD, (MAP != CM_AFFINE && ORDER >= 1)>(xi, a.corners + (size_t)r * (SD << SD), ih, g, H);
            cm_invert<SD>(g);
            const double* ip = a.in + (size_t)r * NTAB * tstride + pl;
            double* op = a.out + (size_t)r * NTAB * tstride + pl;
            if constexpr (MAP == CM_AFFINE) {
                // component by component: (row, component) pairs are rows of npts
                const int n = a.nrows * a.vdim;
                for (int row = 0; row < n; ++row) {
                    double v[NTAB];
#pragma unroll
                    for (int t = 0; t < NTAB; ++t) v[t] = ip[t * tstride];
                    op[0] = v[0];
                    if constexpr (ORDER >= 1) {
#pragma unroll
                        for (int d = 0; d < SD; ++d) {
                            double s = 0.0;
#pragma unroll
                            for (int e = 0; e < SD; ++e) s += v[1 + e] * g.G[e][d];
                            op[(1 + d) * tstride] = s;
                        }
                    }
                    ip += npts;
                    op += npts;
                }
            } else {
                double M[SD][SD], dM[SD][SD][SD];
                cm_piola<SD, ORDER, MAP>(g, H, M, dM);
                for (int row = 0; row < a.nrows; ++row) {
                    double v[NTAB][SD];
#pragma unroll
                    for (int t = 0; t < NTAB; ++t)
#pragma unroll
                        for (int k = 0; k < SD; ++k) v[t][k] = ip[t * tstride + (size_t)k * npts];
#pragma unroll
                    for (int c = 0; c < SD; ++c) {
                        double s = 0.0;
#pragma unroll
                        for (int k = 0; k < SD; ++k) s += M[c][k] * v[0][k];
                        op[(size_t)c * npts] = s;
                        if constexpr (ORDER >= 1) {
                            double de[SD];  // d phi_c / dX_e
#pragma unroll
                            for (int e = 0; e < SD; ++e) {
                                double t = 0.0;
#pragma unroll
                                for (int k = 0; k < SD; ++k) t += dM[e][c][k] * v[0][k] + M[c][k] * v[1 + e][k];
                                de[e] = t;
                            }
#pragma unroll
                            for (int d = 0; d < SD; ++d) {
                                double t = 0.0;
#pragma unroll
                                for (int e = 0; e < SD; ++e) t += de[e] * g.G[e][d];
                                op[(1 + d) * tstride + (size_t)c * npts] = t;
                            }
                        }
                    }
                    ip += rstride;
                    op += rstride;
                }
            }
        }
    }
}

// ---- the fused kernel ---------------------------------------------------------------------------------------------------
struct CmTensorArgs {
    const double* pts;      // [nreq][npts][sd], GRID: [nreq][sd][q] 1-D coordinates of a tensor grid
    const double* corners;  // [nreq][2^sd][sd]
    const double* lines;    // [sd][CM_LINE]: nodes [NN], barycentric weights [NN], differentiation matrix [NN][NN] per factor
    double* out;            // [nreq][ntab][NN^sd][npts]
    double lo[3], h[3];
    long long nreq, nitems;
    int npts, q;
    int P;                  // whole requests per item
    int image;              // 1: per-wave LDS image of the item, 0: streaming stores
};

// every dof of this lane's point: dst = the lane's (t = 0, dof 0) entry in the image or in HBM, rows rs apart, tables ts apart
// (runtime strides kept opaque by the caller: hdivcurl.hpp hdc_block)
template <int SD, int NN, int ORDER>
__device__ __forceinline__ void cm_tensor_rows(const double (&T)[SD][ORDER + 1][NN], const double (&G)[SD][SD], double* dst, int rs,
                                               int ts) {
    double* row = dst;
#pragma unroll
    for (int i0 = 0; i0 < NN; ++i0) {
#pragma unroll
        for (int i1 = 0; i1 < NN; ++i1) {
#pragma unroll
            for (int i2 = 0; i2 < (SD == 3 ? NN : 1); ++i2) {
                const int idx[3] = {i0, i1, i2};
                double v = T[0][0][i0] * T[1][0][i1];
                if constexpr (SD == 3) v *= T[2][0][i2];
                row[0] = v;
                if constexpr (ORDER >= 1) {
                    double ge[SD];  // d / dX_e
#pragma unroll
                    for (int e = 0; e < SD; ++e) {
                        double p = T[e][1][idx[e]];
#pragma unroll
                        for (int d = 0; d < SD; ++d)
                            if (d != e) p *= T[d][0][idx[d]];
                        ge[e] = p;
                    }
                    double* tp = row;
#pragma unroll
                    for (int d = 0; d < SD; ++d) {
                        double s = 0.0;
#pragma unroll
                        for (int e = 0; e < SD; ++e) s += ge[e] * G[e][d];
                        tp += ts;
                        *tp = s;
                    }
                }
                row += rs;
            }
        }
    }
}

template <int SD, int NN, int ORDER, bool GRID>
__global__ __launch_bounds__(64) void cellmap_tensor_kernel(const CmTensorArgs a) {
    static_assert(SD == 2 || SD == 3, "quadrilaterals and hexahedra");
    static_assert(NN >= CM_MINNN && NN <= CM_MAXNN && ORDER >= 0 && ORDER <= CM_MAXORDER, "compile-time instances");
    constexpr int NTAB = 1 + SD * ORDER;
    constexpr int NDOF = SD == 2 ? NN * NN : NN * NN * NN;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int lane = threadIdx.x & 63;
    const int npts = a.npts;
    const int tstride = NDOF * npts;  // (a request has fewer than 2^31 entries)
    const long long reqsize = (long long)NTAB * tstride;
    double ih[SD];
#pragma unroll
    for (int d = 0; d < SD; ++d) ih[d] = 1.0 / a.h[d];
    for (long long item = blockIdx.x; item < a.nitems; item += gridDim.x) {
        const long long r0 = item * a.P;
        const long long left = a.nreq - r0;
        const int Pcur = left < a.P ? (int)left : a.P;
        const int nslots = Pcur * npts;
        double* gout = a.out + (size_t)r0 * reqsize;
        for (int s0 = 0; s0 < nslots; s0 += 64) {
            const int slot = s0 + lane;
            const bool active = slot < nslots;
            const int rl = active ? slot / npts : 0;
            const int pl = active ? slot - rl * npts : 0;
            const long long r = r0 + rl;
            // the factors and their derivatives at this lane's point: T[d][k][i] = k-th derivative of basis function i at X_d
            double T[SD][ORDER + 1][NN], xi[SD];
#pragma unroll
            for (int d = 0; d < SD; ++d) {
                double X;
                if constexpr (GRID) {
                    const int q = a.q;
                    int j = pl;  // point = row-major (j0, j1[, j2])
                    if (d == 0) j = SD == 2 ? pl / q : pl / (q * q);
                    else if (d == 1) j = SD == 2 ? pl % q : (pl / q) % q;
                    else j = pl % q;
                    X = a.pts[((size_t)r * SD + d) * q + j];
                } else {
                    X = a.pts[((size_t)r * npts + pl) * SD + d];
                }
                const double* ln = a.lines + d * CM_LINE;
                const LineDesc L{ln, ln + NN, ln + 2 * NN, NN};
                lagrange_values_n<NN>(L, X, T[d][0]);
                if constexpr (ORDER >= 1) lagrange_diff_n<NN>(L, T[d][0], T[d][1]);
                xi[d] = (X - a.lo[d]) / a.h[d];
            }
            CmGeom<SD> g;
            if constexpr (ORDER >= 1) {
                double H[SD][SD][SD];
                cm_map<SD, false>(xi, a.corners + (size_t)r * (SD << SD), ih, g, H);
                cm_invert<SD>(g);
            }
            if (!active) continue;
            int rs = npts, ts = tstride;  // (opaque per item: the strides stay single registers, see cm_tensor_rows)
            asm volatile("" : "+v"(rs), "+v"(ts));
            const size_t off = (size_t)rl * reqsize + pl;  // the lane's (t = 0, dof 0) entry from the start of the item
            // ONE copy of the dof loops behind a generic pointer, as hdivcurl_kernel: with a copy per route the compiler lifts
            // the products the two copies share above the branch and keeps all of them live (order-0 Q4 hexahedra: 125 values,
            // 190 of them parked in AGPRs)
            cm_tensor_rows<SD, NN, ORDER>(T, g.G, (a.image ? lds : gout) + off, rs, ts);
        }
        if (a.image) flush_item(gout, lds, (long long)Pcur * reqsize, lane);
    }
}

}  // namespace fxk
