// Serendipity elements S_k on quadrilaterals and hexahedra, evaluated directly (gfx950).
//
// Reference behaviour: Serendipity.tabulate (FIAT/serendipity.py:134-174) differentiates a sympy array of the basis
// functions (v_lambda_0 / e_lambda_0 / f_lambda_0 / i_lambda_0, :180-225) and evaluates it per multi-index.  Every one of
// those functions is a signed product of one 1-D factor per direction.  On direction d of the flattened cell, with v0, v1
// the first and last vertex coordinate, h = v1 - v0:
//   lambda0 = (v1 - x) / h,  lambda1 = (x - v0) / h,  b = lambda0 lambda1,  t = 2 x - (v0 + v1)   (the reference's x_mid:
//   NOT divided by h), and the factor of code 0 is lambda0, of code 1 lambda1, of code 2 + j  b L_j(t)  (Legendre), j <= K - 2.
// The table of alpha is  sign * prod_d (d/dx)^alpha_d f_code_d (x_d):  O(ndof) products per point and table.
//
// Lane <-> (request, point), as hdivcurl_kernel: the lane evaluates the K + 1 functions of every direction and their
// derivatives in registers (three-term recurrence of L_j and its derivatives in t, Leibniz with b, b', b''; dt/dx = 2), then
// writes every table and dof.  The dof table is a constexpr function of (SD, K); tables and dofs are compile-time loops, so
// no private array is indexed at run time.  An item is P whole requests (P * npts <= 64; one request in chunks of 64 points
// beyond).  Where it fits SER_IMAGE_BYTES it goes through a per-wave LDS image and leaves as whole-line non-temporal stores
// (store.hpp flush_item); larger requests stream: every lane stores its own entries with plain stores.
#pragma once
#include <hip/hip_runtime.h>

#include <utility>

#include "line_basis.hpp"
#include "store.hpp"

namespace fxk {

// 40 KB per wave: four one-wave workgroups share the 160 KB of a CU, one per SIMD
constexpr int SER_IMAGE_BYTES = 40 * 1024;
constexpr int SER_SPEC_MAXK = 6, SER_SPEC_MAXORDER = 2;  // compile-time instances
constexpr int SER_GEN_MAXK = 12, SER_GEN_MAXORDER = 3;   // generic instance

struct SerArgs {
    const double* pts;  // [nreq][npts][sd]
    double* out;        // [nreq][ntab][ndof][npts]
    double v0[3], v1[3];
    long long nreq, nitems;
    int npts, ndof, ntab;
    int P;              // whole requests per item
    int image;          // 1: per-wave LDS image of the item, 0: streaming stores
    int degree, order;  // generic instance only
};

// ---- the dof table ------------------------------------------------------------------------------------------------------
// One packed row per dof, in FIAT's order: bit 0 = the sign is minus, bits 8.., 16.., 24.. = the codes of x, y, z.
__host__ __device__ constexpr int ser_pack(int minus, int cx, int cy, int cz) { return minus | cx << 8 | cy << 16 | cz << 24; }
__host__ __device__ constexpr int ser_code(int row, int d) { return (row >> (8 + 8 * d)) & 0xff; }
__host__ __device__ constexpr int ser_minus(int row) { return row & 1; }

// rows of S_k on the quadrilateral (sd 2) or hexahedron (sd 3) into rows[] (nullptr: count only); returns their number
__host__ __device__ constexpr int ser_fill(int sd, int k, int* rows) {
    int n = 0;
    const int ne = k - 1;  // functions b L_j per direction
    if (sd == 2) {
        for (int a = 0; a < 2; ++a)
            for (int b = 0; b < 2; ++b) {
                if (rows) rows[n] = ser_pack(0, a, b, 0);
                ++n;
            }
        for (int a = 0; a < 2; ++a)
            for (int j = 0; j < ne; ++j) {
                if (rows) rows[n] = ser_pack(1, a, 2 + j, 0);
                ++n;
            }
        for (int b = 0; b < 2; ++b)
            for (int j = 0; j < ne; ++j) {
                if (rows) rows[n] = ser_pack(1, 2 + j, b, 0);
                ++n;
            }
        for (int m = 4; m <= k; ++m)
            for (int j = 0; j < m - 3; ++j) {
                if (rows) rows[n] = ser_pack(0, 2 + j, 2 + m - 4 - j, 0);
                ++n;
            }
        return n;
    }
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b)
            for (int c = 0; c < 2; ++c) {
                if (rows) rows[n] = ser_pack(0, a, b, c);
                ++n;
            }
    for (int b = 0; b < 2; ++b)
        for (int a = 0; a < 2; ++a)
            for (int j = 0; j < ne; ++j) {
                if (rows) rows[n] = ser_pack(1, b, a, 2 + j);
                ++n;
            }
    for (int a = 0; a < 2; ++a)
        for (int c = 0; c < 2; ++c)
            for (int j = 0; j < ne; ++j) {
                if (rows) rows[n] = ser_pack(1, a, 2 + j, c);
                ++n;
            }
    for (int c = 0; c < 2; ++c)
        for (int b = 0; b < 2; ++b)
            for (int j = 0; j < ne; ++j) {
                if (rows) rows[n] = ser_pack(1, 2 + j, c, b);
                ++n;
            }
    for (int a = 0; a < 2; ++a)
        for (int m = 4; m <= k; ++m)
            for (int j = 0; j < m - 3; ++j) {
                if (rows) rows[n] = ser_pack(0, a, 2 + j, 2 + m - 4 - j);
                ++n;
            }
    for (int b = 0; b < 2; ++b)
        for (int m = 4; m <= k; ++m)
            for (int j = 0; j < m - 3; ++j) {
                if (rows) rows[n] = ser_pack(0, 2 + m - 4 - j, b, 2 + j);
                ++n;
            }
    for (int c = 0; c < 2; ++c)
        for (int m = 4; m <= k; ++m)
            for (int j = 0; j < m - 3; ++j) {
                if (rows) rows[n] = ser_pack(0, 2 + j, 2 + m - 4 - j, c);
                ++n;
            }
    for (int l = 6; l <= k; ++l)
        for (int j = 0; j < l - 5; ++j)
            for (int i = 0; i <= j; ++i) {
                if (rows) rows[n] = ser_pack(1, 2 + l - 6 - j, 2 + j - i, 2 + i);
                ++n;
            }
    return n;
}

template <int SD, int K> struct SerDofs {
    static constexpr int NDOF = ser_fill(SD, K, nullptr);
    int row[NDOF];
    constexpr SerDofs() : row{} { ser_fill(SD, K, row); }
};

// ---- compile-time instances -------------------------------------------------------------------------------------------
// F[m][c] = m-th derivative in x of the function of code c on [v0, v1]
template <int K, int ORDER>
__device__ __forceinline__ void ser_line(double x, double v0, double v1, double (&F)[ORDER + 1][K + 1]) {
    const double ih = 1.0 / (v1 - v0);
    F[0][0] = (v1 - x) * ih;
    F[0][1] = (x - v0) * ih;
    if constexpr (ORDER >= 1) {
        F[1][0] = -ih;
        F[1][1] = ih;
    }
    if constexpr (ORDER >= 2) {
        F[2][0] = 0.0;
        F[2][1] = 0.0;
    }
    if constexpr (K >= 2) {
        constexpr int NE = K - 1;
        const double t = 2.0 * x - (v0 + v1);
        const double b = F[0][0] * F[0][1];
        const double b1 = -t * ih * ih;      // b'
        const double b2 = -2.0 * ih * ih;    // b''
        double L[ORDER + 1][NE];             // d^m L_j / dt^m
#pragma unroll
        for (int m = 0; m <= ORDER; ++m) {
            L[m][0] = m == 0 ? 1.0 : 0.0;
            if constexpr (NE > 1) L[m][1] = m == 0 ? t : (m == 1 ? 1.0 : 0.0);
        }
#pragma unroll
        for (int j = 2; j < NE; ++j) {
#pragma unroll
            for (int m = 0; m <= ORDER; ++m) {
                double s = t * L[m][j - 1];
                if (m > 0) s += (double)m * L[m - 1][j - 1];
                L[m][j] = ((double)(2 * j - 1) * s - (double)(j - 1) * L[m][j - 2]) * (1.0 / (double)j);
            }
        }
#pragma unroll
        for (int j = 0; j < NE; ++j) {
            F[0][2 + j] = b * L[0][j];
            if constexpr (ORDER >= 1) F[1][2 + j] = 2.0 * b * L[1][j] + b1 * L[0][j];
            if constexpr (ORDER >= 2) F[2][2 + j] = 4.0 * b * L[2][j] + 4.0 * b1 * L[1][j] + b2 * L[0][j];
        }
    }
}

// one entry: table T, dof DOF.  The row pointer advances by the opaque runtime stride `rs` (hdc_block: a compile-time
// multiple per store would be hoisted out of the item loop as hundreds of live registers).
template <int SD, int K, int ORDER, int T, int DOF>
__device__ __forceinline__ void ser_entry(const double (&F)[SD][ORDER + 1][K + 1], double*& row, int rs) {
    constexpr SerDofs<SD, K> TBL{};
    constexpr TensorAlpha<SD, ORDER> AL{};
    constexpr int r = TBL.row[DOF];
    double v = F[0][AL.a[T][0]][ser_code(r, 0)] * F[1][AL.a[T][1]][ser_code(r, 1)];
    if constexpr (SD == 3) v *= F[2][AL.a[T][2]][ser_code(r, 2)];
    *row = ser_minus(r) ? -v : v;
    row += rs;
}

template <int SD, int K, int ORDER, int T, int... DOFS>
__device__ __forceinline__ void ser_table(std::integer_sequence<int, DOFS...>, const double (&F)[SD][ORDER + 1][K + 1], double*& row, int rs) {
    (ser_entry<SD, K, ORDER, T, DOFS>(F, row, rs), ...);
}

template <int SD, int K, int ORDER, int... TS>
__device__ __forceinline__ void ser_tables(std::integer_sequence<int, TS...>, const double (&F)[SD][ORDER + 1][K + 1], double* row, int rs) {
    (ser_table<SD, K, ORDER, TS>(std::make_integer_sequence<int, SerDofs<SD, K>::NDOF>{}, F, row, rs), ...);
}

template <int SD, int K, int ORDER>
__global__ __launch_bounds__(64) void serendipity_kernel(const SerArgs a) {
    static_assert(SD == 2 || SD == 3, "quadrilaterals and hexahedra");
    constexpr int NTAB = TensorAlpha<SD, ORDER>::NTAB;
    constexpr int NDOF = SerDofs<SD, K>::NDOF;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int lane = threadIdx.x & 63;
    const int npts = a.npts;
    const long long reqsize = (long long)NTAB * NDOF * npts;
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
            double F[SD][ORDER + 1][K + 1];
#pragma unroll
            for (int d = 0; d < SD; ++d) ser_line<K, ORDER>(a.pts[((size_t)r * npts + pl) * SD + d], a.v0[d], a.v1[d], F[d]);
            if (!active) continue;
            int rs = npts;  // (opaque per item: the stride stays one register)
            asm volatile("" : "+v"(rs));
            double* base = (a.image ? lds : gout) + (size_t)rl * reqsize + pl;
            ser_tables<SD, K, ORDER>(std::make_integer_sequence<int, NTAB>{}, F, base, rs);
        }
        if (a.image) flush_item(gout, lds, (long long)Pcur * reqsize, lane);
    }
}

// ---- generic instance ---------------------------------------------------------------------------------------------------
// Runtime degree <= SER_GEN_MAXK and order <= SER_GEN_MAXORDER.  The dof table is built in LDS once per workgroup (ser_fill);
// every lane keeps its 1-D tables T[d][m][c] in LDS (lane-minor: no bank conflicts), then walks tables and dofs and streams
// its entries with plain stores.  LDS: ndof ints (rounded to doubles) + sd (order + 1) (degree + 1) 64 doubles.
__host__ __device__ constexpr size_t ser_generic_lds(int sd, int degree, int order, int ndof) {
    return (size_t)((ndof + 1) / 2) * 8 + (size_t)sd * (order + 1) * (degree + 1) * 64 * 8;
}

template <int SD>
__global__ __launch_bounds__(64) void serendipity_generic(const SerArgs a) {
    constexpr int MO = SER_GEN_MAXORDER;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int lane = threadIdx.x & 63;
    const int K = a.degree, order = a.order, npts = a.npts, ndof = a.ndof;
    const int nf = K + 1;
    int* rows = reinterpret_cast<int*>(lds);
    double* T = lds + (ndof + 1) / 2;
    if (lane == 0) ser_fill(SD, K, rows);
    wave_lds_fence();
    const size_t tstride = (size_t)ndof * npts;
    const long long reqsize = (long long)a.ntab * tstride;
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
            // this lane's 1-D tables: T[((d (order + 1) + m) nf + c) 64 + lane]
            for (int d = 0; d < SD; ++d) {
                const double x = a.pts[((size_t)r * npts + pl) * SD + d];
                double v0 = a.v0[0], v1 = a.v1[0];
                if (d == 1) v0 = a.v0[1], v1 = a.v1[1];
                if (d == 2) v0 = a.v0[2], v1 = a.v1[2];
                const double ih = 1.0 / (v1 - v0);
                const double l0 = (v1 - x) * ih, l1 = (x - v0) * ih;
                const double t = 2.0 * x - (v0 + v1);
                const double b = l0 * l1, b1 = -t * ih * ih, b2 = -2.0 * ih * ih;
                double* Td = T + (size_t)d * (order + 1) * nf * 64 + lane;
                for (int m = 0; m <= order; ++m) {
                    Td[(m * nf + 0) * 64] = m == 0 ? l0 : (m == 1 ? -ih : 0.0);
                    Td[(m * nf + 1) * 64] = m == 0 ? l1 : (m == 1 ? ih : 0.0);
                }
                // L_j and its first MO derivatives in t, rolling (constant indices: registers)
                double Lp[MO + 1], Lc[MO + 1];  // L_{j-1}, L_j
#pragma unroll
                for (int m = 0; m <= MO; ++m) {
                    Lp[m] = 0.0;
                    Lc[m] = m == 0 ? 1.0 : 0.0;
                }
                for (int j = 0; j + 2 < nf; ++j) {
                    double pw = 1.0;  // 2^m
#pragma unroll
                    for (int m = 0; m <= MO; ++m) {
                        if (m <= order) {
                            double f = pw * b * Lc[m];
                            if (m >= 1) f += (double)m * (0.5 * pw) * b1 * Lc[m >= 1 ? m - 1 : 0];
                            if (m >= 2) f += (double)(m * (m - 1) / 2) * (0.25 * pw) * b2 * Lc[m >= 2 ? m - 2 : 0];
                            Td[(m * nf + 2 + j) * 64] = f;
                        }
                        pw *= 2.0;
                    }
                    // (j + 1) L_{j+1} = (2 j + 1) (t L_j)^(m) - j L_{j-1}^(m)
                    double Ln[MO + 1];
                    const double c1 = (double)(2 * j + 1), c2 = (double)j, inv = 1.0 / (double)(j + 1);
#pragma unroll
                    for (int m = 0; m <= MO; ++m) {
                        double s = t * Lc[m];
                        if (m > 0) s += (double)m * Lc[m > 0 ? m - 1 : 0];
                        Ln[m] = (c1 * s - c2 * Lp[m]) * inv;
                    }
#pragma unroll
                    for (int m = 0; m <= MO; ++m) {
                        Lp[m] = Lc[m];
                        Lc[m] = Ln[m];
                    }
                }
            }
            double* dst = a.out + (size_t)r * reqsize + pl;
            const double* T0 = T + lane;
            const double* T1 = T0 + (size_t)(order + 1) * nf * 64;
            const double* T2 = T1 + (size_t)(order + 1) * nf * 64;
            // tables in mis() order: total order o, then (a0, a1[, a2]) with a0 descending
            for (int o = 0; o <= order; ++o) {
                for (int i = 0; i <= o; ++i) {
                    for (int j = 0; j <= (SD == 3 ? i : 0); ++j) {
                        const int a0 = o - i, a1 = SD == 3 ? i - j : i, a2 = j;
                        const double* R0 = T0 + (size_t)a0 * nf * 64;
                        const double* R1 = T1 + (size_t)a1 * nf * 64;
                        const double* R2 = T2 + (size_t)a2 * nf * 64;
                        double* e = dst;
                        for (int dof = 0; dof < ndof; ++dof) {
                            const int row = rows[dof];
                            double v = R0[ser_code(row, 0) * 64] * R1[ser_code(row, 1) * 64];
                            if (SD == 3) v *= R2[ser_code(row, 2) * 64];
                            *e = ser_minus(row) ? -v : v;
                            e += npts;
                        }
                        dst += tstride;
                    }
                }
            }
        }
    }
}

}  // namespace fxk
