// DPC elements on quadrilaterals and hexahedra, evaluated in closed form (gfx950).
//
// Reference behaviour: DPC_k (FIAT/discontinuous_pc.py) is a Ciarlet element: P_k over the expansion set of the simplex of
// the cell's dimension, dual to point evaluation at the equispaced degree-k lattice of that simplex, which an affine map
// places over the cube (DPCDualSet :59-73).  The nodal basis of an equispaced lattice on an affine simplex is
//   phi_alpha(x) = prod_{i = 0..SD} l_{alpha_i}(lambda_i(x)),   l_a(t) = prod_{j < a} (K t - j) / (j + 1),   |alpha| = K,
// lambda the barycentric coordinates of the mapped simplex: no Vandermonde matrix, no coefficient contraction.  The
// structure is that of bernstein.hpp with l_a in place of the powers lambda^a / a!: 1-D tables per barycentric coordinate,
// a product per dof, and the barycentric derivatives contracted with G = d lambda / dx for the Cartesian tables.
//
// Lane <-> (request, point), as serendipity_kernel: the lane evaluates l_a, l_a', l_a'' (a <= K) of every barycentric
// coordinate in registers by the recurrence l_a = l_{a-1} (K t - a + 1) / a, then writes every dof and table.  The dof table
// is a constexpr function of (SD, K); dofs are a fold over an integer sequence, so no private array is indexed at run time.
// An item is P whole requests (P * npts <= 64; one request in chunks of 64 points beyond).  Where it fits DPC_IMAGE_BYTES it
// goes through a per-wave LDS image and leaves as whole-line non-temporal stores (store.hpp flush_item); larger requests stream:
// every lane stores its own entries with plain stores.
#pragma once
#include <hip/hip_runtime.h>

#include <utility>

#include "store.hpp"

namespace fxk {

// 40 KB per wave: four one-wave workgroups share the 160 KB of a CU, one per SIMD
constexpr int DPC_IMAGE_BYTES = 40 * 1024;
constexpr int DPC_MAXK = 6, DPC_MAXORDER = 2;  // compile-time instances

struct DpcArgs {
    const double* pts;  // [nreq][npts][sd]
    double* out;        // [nreq][ntab][ndof][npts]
    double lam0[4];     // lambda_i = lam0[i] + sum_d G[i][d] x_d on the mapped simplex
    double G[12];       // [sd + 1][sd]
    long long nreq, nitems;
    int npts;
    int P;              // whole requests per item
    int image;          // 1: per-wave LDS image of the item, 0: streaming stores
};

__host__ __device__ constexpr int dpc_binom(int a, int b) {
    if (b < 0 || a < b) return 0;
    long long r = 1;
    for (int j = 0; j < b; ++j) r = r * (a - j) / (j + 1);
    return (int)r;
}

// ---- the dof table ------------------------------------------------------------------------------------------------------
// One packed row per dof: alpha_i in bits 8 i ...  Rows come in the order of the reference's nodes: the entities of the UFC
// simplex by dimension and number (vertices, edges, faces, interior), each with the interior lattice points of make_points
// (multiindex_equal(dim + 1, K, 1): positive entries on the entity's vertices, the last vertex slowest).
__host__ __device__ constexpr int dpc_pack(int a0, int a1, int a2, int a3) { return a0 | a1 << 8 | a2 << 16 | a3 << 24; }
__host__ __device__ constexpr int dpc_alpha(int row, int i) { return (row >> (8 * i)) & 0xff; }

// rows of DPC_k on the quadrilateral (sd 2) or hexahedron (sd 3) into rows[] (nullptr: count only); returns their number
__host__ __device__ constexpr int dpc_fill(int sd, int k, int* rows) {
    // the entities of the UFC triangle / tetrahedron as vertex bit masks (vertex tuples are ascending), in entity order
    const int tri[7] = {1, 2, 4, 6, 5, 3, 7};
    const int tet[15] = {1, 2, 4, 8, 12, 10, 6, 9, 5, 3, 14, 13, 11, 7, 15};
    const int nent = sd == 2 ? 7 : 15;
    int n = 0;
    for (int e = 0; e < nent; ++e) {
        const int mask = sd == 2 ? tri[e] : tet[e];
        int d = -1;
        for (int v = 0; v < 4; ++v) d += (mask >> v) & 1;
        for (int l3 = d >= 3 ? 1 : 0; l3 <= (d >= 3 ? k - 3 : 0); ++l3)
            for (int l2 = d >= 2 ? 1 : 0; l2 <= (d >= 2 ? k - l3 - 2 : 0); ++l2)
                for (int l1 = d >= 1 ? 1 : 0; l1 <= (d >= 1 ? k - l3 - l2 - 1 : 0); ++l1) {
                    const int local[4] = {k - l3 - l2 - l1, l1, l2, l3};
                    if (rows) {
                        int a[4] = {0, 0, 0, 0};
                        int j = 0;
                        for (int v = 0; v < 4; ++v)
                            if ((mask >> v) & 1) a[v] = local[j++];
                        rows[n] = dpc_pack(a[0], a[1], a[2], a[3]);
                    }
                    ++n;
                }
    }
    return n;
}

template <int SD, int K> struct DpcDofs {
    static constexpr int NDOF = dpc_binom(K + SD, SD);
    static_assert(dpc_fill(SD, K, nullptr) == NDOF, "the lattice of a simplex");
    int row[NDOF];
    constexpr DpcDofs() : row{} { dpc_fill(SD, K, row); }
};

// L[m][a] = m-th derivative in t of l_a at t = lam
template <int K, int ORDER> __device__ __forceinline__ void dpc_line(double lam, double (&L)[ORDER + 1][K + 1]) {
    L[0][0] = 1.0;
    if constexpr (ORDER >= 1) L[1][0] = 0.0;
    if constexpr (ORDER >= 2) L[2][0] = 0.0;
#pragma unroll
    for (int a = 1; a <= K; ++a) {
        const double f = (double)K * lam - (double)(a - 1);
        const double inv = 1.0 / (double)a;
        L[0][a] = L[0][a - 1] * f * inv;
        if constexpr (ORDER >= 1) L[1][a] = (L[1][a - 1] * f + (double)K * L[0][a - 1]) * inv;
        if constexpr (ORDER >= 2) L[2][a] = (L[2][a - 1] * f + (double)(2 * K) * L[1][a - 1]) * inv;
    }
}

// The tables of one dof (compile-time DOF: alpha is constant, so l_0 = 1 and the vanishing derivatives l_0', l_0'', l_1'' drop
// out at compile time).
template <int SD, int K, int ORDER, int DOF>
__device__ __forceinline__ void dpc_dof(const double (&L)[SD + 1][ORDER + 1][K + 1], const double (&G)[SD + 1][SD],
                                        double (&tab)[dpc_binom(SD + ORDER, SD)]) {
    constexpr DpcDofs<SD, K> TBL{};
    constexpr int r = TBL.row[DOF];
    double v = 1.0;
#pragma unroll
    for (int i = 0; i <= SD; ++i)
        if (dpc_alpha(r, i) >= 1) v *= L[i][0][dpc_alpha(r, i)];
    tab[0] = v;
    if constexpr (ORDER >= 1) {
        // first barycentric derivatives D1[i] = l'_{alpha_i}(lambda_i) prod_{j != i} l_{alpha_j}(lambda_j)
        double g[SD];
#pragma unroll
        for (int d = 0; d < SD; ++d) g[d] = 0.0;
#pragma unroll
        for (int i = 0; i <= SD; ++i) {
            if (dpc_alpha(r, i) >= 1) {
                double t = L[i][1][dpc_alpha(r, i)];
#pragma unroll
                for (int j = 0; j <= SD; ++j)
                    if (j != i && dpc_alpha(r, j) >= 1) t *= L[j][0][dpc_alpha(r, j)];
#pragma unroll
                for (int d = 0; d < SD; ++d) g[d] += G[i][d] * t;
            }
        }
#pragma unroll
        for (int d = 0; d < SD; ++d) tab[1 + d] = g[d];
    }
    if constexpr (ORDER >= 2) {
        // D2[i][j] = l'_i l'_j prod_{m != i, j} l_m (i != j),  l''_i prod_{m != i} l_m (i == j);  H[i][d] = sum_j G[j][d] D2[i][j]
        double H[SD + 1][SD];
#pragma unroll
        for (int i = 0; i <= SD; ++i)
#pragma unroll
            for (int d = 0; d < SD; ++d) H[i][d] = 0.0;
#pragma unroll
        for (int i = 0; i <= SD; ++i) {
#pragma unroll
            for (int j = i; j <= SD; ++j) {
                const int ai = dpc_alpha(r, i), aj = dpc_alpha(r, j);
                if (i == j ? ai >= 2 : (ai >= 1 && aj >= 1)) {
                    double t = i == j ? L[i][2][ai] : L[i][1][ai] * L[j][1][aj];
#pragma unroll
                    for (int m = 0; m <= SD; ++m)
                        if (m != i && m != j && dpc_alpha(r, m) >= 1) t *= L[m][0][dpc_alpha(r, m)];
#pragma unroll
                    for (int d = 0; d < SD; ++d) {
                        H[i][d] += G[j][d] * t;
                        if (j != i) H[j][d] += G[i][d] * t;
                    }
                }
            }
        }
        int h = 1 + SD;  // mis(SD, 2) order: (d1, d2), d1 <= d2, lexicographic
#pragma unroll
        for (int d1 = 0; d1 < SD; ++d1)
#pragma unroll
            for (int d2 = d1; d2 < SD; ++d2) {
                double s = 0.0;
#pragma unroll
                for (int i = 0; i <= SD; ++i)
                    if (dpc_alpha(r, i) >= 1) s += G[i][d1] * H[i][d2];
                tab[h++] = s;
            }
    }
}

// one dof: its tables into the image (li: index of the lane's (t = 0, dof) entry) or to HBM (gp: pointer to it).  Both
// advance by the opaque runtime stride `rs` (serendipity.hpp ser_entry: a compile-time multiple per dof would be hoisted out
// of the item loop as hundreds of live registers).
template <int SD, int K, int ORDER, int DOF>
__device__ __forceinline__ void dpc_dof_store(const double (&L)[SD + 1][ORDER + 1][K + 1], const double (&G)[SD + 1][SD], bool image,
                                              double* lds, int& li, double*& gp, int rs, int tstride) {
    constexpr int NTAB = dpc_binom(SD + ORDER, SD);
    double tab[NTAB];
    dpc_dof<SD, K, ORDER, DOF>(L, G, tab);
    if (image) {  // (uniform) LDS image
#pragma unroll
        for (int t = 0; t < NTAB; ++t) lds[li + t * tstride] = tab[t];
    } else {      // streaming: plain stores, the L2 joins the partial lines of neighbouring lanes and rows
#pragma unroll
        for (int t = 0; t < NTAB; ++t) gp[(size_t)t * (size_t)tstride] = tab[t];
    }
    li += rs;
    gp += rs;
}

template <int SD, int K, int ORDER, int... DOFS>
__device__ __forceinline__ void dpc_all_dofs(std::integer_sequence<int, DOFS...>, const double (&L)[SD + 1][ORDER + 1][K + 1],
                                             const double (&G)[SD + 1][SD], bool image, double* lds, int li, double* gp, int rs,
                                             int tstride) {
    (dpc_dof_store<SD, K, ORDER, DOFS>(L, G, image, lds, li, gp, rs, tstride), ...);
}

template <int SD, int K, int ORDER>
__global__ __launch_bounds__(64) void dpc_kernel(const DpcArgs a) {
    static_assert(SD == 2 || SD == 3, "quadrilaterals and hexahedra");
    static_assert(K >= 1 && K <= DPC_MAXK && ORDER >= 0 && ORDER <= DPC_MAXORDER, "compile-time instances");
    constexpr int NTAB = dpc_binom(SD + ORDER, SD);
    constexpr int NDOF = DpcDofs<SD, K>::NDOF;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int lane = threadIdx.x & 63;
    const int npts = a.npts;
    const int tstride = NDOF * npts;                         // (a request has fewer than 2^31 entries)
    const long long reqsize = (long long)NTAB * tstride;
    double G[SD + 1][SD];
#pragma unroll
    for (int i = 0; i <= SD; ++i)
#pragma unroll
        for (int d = 0; d < SD; ++d) G[i][d] = a.G[i * SD + d];
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
            const double* pp = a.pts + ((size_t)(r0 + rl) * npts + pl) * SD;
            double L[SD + 1][ORDER + 1][K + 1];
#pragma unroll
            for (int i = 0; i <= SD; ++i) {
                double lam = a.lam0[i];
#pragma unroll
                for (int d = 0; d < SD; ++d) lam += G[i][d] * pp[d];
                dpc_line<K, ORDER>(lam, L[i]);
            }
            int rs = npts;  // (opaque per item: the stride stays one register)
            asm volatile("" : "+v"(rs));
            const size_t off = (size_t)rl * reqsize + pl;   // the lane's (t = 0, dof = 0) entry from the start of the item
            dpc_all_dofs<SD, K, ORDER>(std::make_integer_sequence<int, NDOF>{}, L, G, a.image != 0, lds, (int)off, gout + off, rs,
                                       tstride);
        }
        if (a.image) flush_item(gout, lds, (long long)Pcur * reqsize, lane);
    }
}

}  // namespace fxk
