// Bernstein-Bezier basis on simplices, evaluated directly in barycentric coordinates (gfx950).
//
// Bernstein.tabulate of the reference (FIAT/bernstein.py) never goes through the expansion set: a table entry is
//   B_k = n!/prod k_i! prod lambda_i^k_i,      d^beta_lambda B_k = n!/prod (k-beta)_i! prod lambda_i^(k-beta)_i
// (zero where k - beta has a negative entry), and the Cartesian table of alpha contracts the barycentric derivatives of
// order |alpha| with the columns G = R2B[:, :sd] = d lambda / dx:  d/dx_d = sum_i G[i][d] d/dlambda_i.
// That is O(ndof) flops per point and table, no coefficient contraction.
//
// Lane <-> (request, point); an item is P whole requests (P * npts <= 64, or one request in chunks of 64 points).  Where
// the item's tables fit (BERN_IMAGE_BYTES) they go through a per-wave LDS image and leave as whole-line non-temporal
// stores (store.hpp flush_item); larger requests stream: every lane stores its own entries, row by row, with plain
// stores.  Powers are repeated products, so an exponent 0 is exactly 1 at lambda = 0.
//
// Three sources of (lambda, G), set by the arguments:
//   verts == nullptr              the element's own cell: lambda from (E, v0), G by value;
//   verts != nullptr, !shared     the request's cell verts[r]: lambda and G from that cell (physical basis functions);
//   verts != nullptr,  shared     ONE point set on the element's cell: lambda from (E, v0), G from verts[r].
#pragma once
#include <hip/hip_runtime.h>

#include <utility>

#include "store.hpp"

namespace fxk {

constexpr int BERN_MAXN = 16;             // degree limit of the C ABI
constexpr int BERN_SPEC_MAXN = 6;         // compile-time instances: degree <= 6, order <= 2
constexpr int BERN_IMAGE_BYTES = 48 * 1024;  // largest per-wave LDS image; larger items stream

struct BernArgs {
    const double* pts;    // [nreq][npts][SD], or [npts][SD] when shared
    const double* verts;  // [nreq][SD+1][SD] or nullptr
    double* out;          // [nreq][ntab][ndof][npts]
    double E[9];          // element cell: lambda_{1..SD} = E (x - v0), lambda_0 = 1 - sum
    double v0[3];
    double G[12];         // element cell: G[i][d] = d lambda_i / d x_d, [SD+1][SD]
    long long nreq, nitems;
    int npts, P;
    int n, order;         // generic instance only
    int ntab, ndof;
    int image;            // 1: per-wave LDS image of the item, 0: streaming stores
    int stage_doubles;    // per-wave LDS doubles of the image (generic: of the chain-rule coefficients)
    int shared;
};

constexpr int bern_binom(int a, int b) {
    if (b < 0 || a < b) return 0;
    long long r = 1;
    for (int j = 0; j < b; ++j) r = r * (a - j) / (j + 1);
    return (int)r;
}

// dofs in mis(SD+1, N) order (first entry descending), with the weights N!/prod k_i!
template <int SD, int N> struct BernDofs {
    static constexpr int NDOF = bern_binom(N + SD, SD);
    int k[NDOF][SD + 1];
    double w[NDOF];
    constexpr BernDofs() : k{}, w{} {
        int a[SD + 1] = {};
        a[0] = N;
        for (int dof = 0; dof < NDOF; ++dof) {
            double f = 1.0;
            for (int j = 2; j <= N; ++j) f *= j;
            for (int i = 0; i <= SD; ++i) {
                k[dof][i] = a[i];
                for (int j = 2; j <= a[i]; ++j) f /= j;
            }
            w[dof] = f;
            // next multi-index: the rightmost p < SD with a[p] > 0 gives one to position p+1, which takes all of the tail
            int p = -1;
            for (int q = 0; q < SD; ++q)
                if (a[q] > 0) p = q;
            if (p < 0) break;
            int tail = 1;
            for (int q = p + 1; q <= SD; ++q) tail += a[q];
            a[p] -= 1;
            for (int q = p + 1; q <= SD; ++q) a[q] = 0;
            a[p + 1] = tail;
        }
    }
};

// Barycentric coordinates of an affine simplex: E = inverse of [v1-v0 | ... | vSD-v0]; G[0] = -(sum of E's rows).
template <int SD> __device__ __forceinline__ void bern_cell(const double* v, double (&E)[SD][SD], double (&v0)[SD]) {
    double e[SD][SD];
#pragma unroll
    for (int r = 0; r < SD; ++r) {
        v0[r] = v[r];
#pragma unroll
        for (int c = 0; c < SD; ++c) e[r][c] = v[(c + 1) * SD + r] - v[r];
    }
    if constexpr (SD == 1) {
        E[0][0] = 1.0 / e[0][0];
    } else if constexpr (SD == 2) {
        const double inv = 1.0 / (e[0][0] * e[1][1] - e[0][1] * e[1][0]);
        E[0][0] = e[1][1] * inv;
        E[0][1] = -e[0][1] * inv;
        E[1][0] = -e[1][0] * inv;
        E[1][1] = e[0][0] * inv;
    } else {
        const double c00 = e[1][1] * e[2][2] - e[1][2] * e[2][1];
        const double c01 = e[1][2] * e[2][0] - e[1][0] * e[2][2];
        const double c02 = e[1][0] * e[2][1] - e[1][1] * e[2][0];
        const double inv = 1.0 / (e[0][0] * c00 + e[0][1] * c01 + e[0][2] * c02);
        E[0][0] = c00 * inv;
        E[0][1] = (e[0][2] * e[2][1] - e[0][1] * e[2][2]) * inv;
        E[0][2] = (e[0][1] * e[1][2] - e[0][2] * e[1][1]) * inv;
        E[1][0] = c01 * inv;
        E[1][1] = (e[0][0] * e[2][2] - e[0][2] * e[2][0]) * inv;
        E[1][2] = (e[0][2] * e[1][0] - e[0][0] * e[1][2]) * inv;
        E[2][0] = c02 * inv;
        E[2][1] = (e[0][1] * e[2][0] - e[0][0] * e[2][1]) * inv;
        E[2][2] = (e[0][0] * e[1][1] - e[0][1] * e[1][0]) * inv;
    }
}

template <int SD> __device__ __forceinline__ void bern_grad(const double (&E)[SD][SD], double (&G)[SD + 1][SD]) {
#pragma unroll
    for (int d = 0; d < SD; ++d) {
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < SD; ++i) {
            G[i + 1][d] = E[i][d];
            s += E[i][d];
        }
        G[0][d] = -s;
    }
}

template <int SD>
__device__ __forceinline__ void bern_lambda(const double (&E)[SD][SD], const double (&v0)[SD], const double (&x)[SD],
                                            double (&lam)[SD + 1]) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < SD; ++i) {
        double t = 0.0;
#pragma unroll
        for (int d = 0; d < SD; ++d) t += E[i][d] * (x[d] - v0[d]);
        lam[i + 1] = t;
        s += t;
    }
    lam[0] = 1.0 - s;
}

// lambda and G of one lane (uniform branches on the mode)
template <int SD>
__device__ __forceinline__ void bern_setup(const BernArgs& a, long long req, int pl, double (&lam)[SD + 1], double (&G)[SD + 1][SD]) {
    double x[SD];
    const double* pp = a.pts + ((size_t)(a.shared ? 0 : req) * a.npts + pl) * SD;
#pragma unroll
    for (int d = 0; d < SD; ++d) x[d] = pp[d];
    double E[SD][SD], v0[SD];
#pragma unroll
    for (int i = 0; i < SD; ++i) {
        v0[i] = a.v0[i];
#pragma unroll
        for (int d = 0; d < SD; ++d) E[i][d] = a.E[i * SD + d];
    }
    if (a.verts != nullptr) {
        double Ec[SD][SD], vc[SD];
        bern_cell<SD>(a.verts + (size_t)req * (SD + 1) * SD, Ec, vc);
        bern_grad<SD>(Ec, G);
        if (!a.shared) bern_lambda<SD>(Ec, vc, x, lam);
        else bern_lambda<SD>(E, v0, x, lam);
    } else {
#pragma unroll
        for (int i = 0; i <= SD; ++i)
#pragma unroll
            for (int d = 0; d < SD; ++d) G[i][d] = a.G[i * SD + d];
        bern_lambda<SD>(E, v0, x, lam);
    }
}

// item loop of the compile-time instances: body(req, off, active, gout) with off = the lane's (t = 0, dof = 0) entry from the
// start of the item, in the image (a.image) or in HBM at gout: the image of P whole requests is laid out as they are in HBM
template <class Body>
__device__ __forceinline__ void bern_items(const BernArgs& a, double* stage, Body&& body) {
    const int lane = threadIdx.x & 63;
    const int npts = a.npts;
    const long long reqsize = (long long)a.ntab * a.ndof * npts;
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
            body(r0 + rl, (size_t)rl * reqsize + pl, active, gout);
        }
        if (a.image) flush_item(gout, stage, (long long)Pcur * reqsize, lane);
    }
}

// The tables of one dof (compile-time DOF: every exponent and weight is a constant, the powers stay in registers).
template <int SD, int N, int ORDER, int DOF>
__device__ __forceinline__ void bern_dof(const double (&pw)[SD + 1][N + 1], const double (&G)[SD + 1][SD],
                                         double (&tab)[bern_binom(SD + ORDER, SD)]) {
    constexpr BernDofs<SD, N> TBL{};
    constexpr double W = TBL.w[DOF];
    double v = W;
#pragma unroll
    for (int i = 0; i <= SD; ++i) v *= pw[i][TBL.k[DOF][i]];
    tab[0] = v;
    if constexpr (ORDER >= 1) {
        // first barycentric derivatives D1[i] = w k_i lambda^(k - e_i)
        double D1[SD + 1];
#pragma unroll
        for (int i = 0; i <= SD; ++i) {
            D1[i] = 0.0;
            if (TBL.k[DOF][i] >= 1) {
                double t = W * TBL.k[DOF][i];
#pragma unroll
                for (int j = 0; j <= SD; ++j) t *= pw[j][TBL.k[DOF][j] - (j == i ? 1 : 0)];
                D1[i] = t;
            }
        }
#pragma unroll
        for (int d = 0; d < SD; ++d) {
            double s = 0.0;
#pragma unroll
            for (int i = 0; i <= SD; ++i) s += G[i][d] * D1[i];
            tab[1 + d] = s;
        }
    }
    if constexpr (ORDER >= 2) {
        // D2[i][j] = w k_i (k_j - [i == j]) lambda^(k - e_i - e_j);  H[i][d] = sum_j G[j][d] D2[i][j]
        double H[SD + 1][SD];
#pragma unroll
        for (int i = 0; i <= SD; ++i)
#pragma unroll
            for (int d = 0; d < SD; ++d) H[i][d] = 0.0;
#pragma unroll
        for (int i = 0; i <= SD; ++i) {
#pragma unroll
            for (int j = i; j <= SD; ++j) {
                const int ki = TBL.k[DOF][i], kj = TBL.k[DOF][j] - (i == j ? 1 : 0);
                if (ki >= 1 && kj >= 1) {
                    double t = W * ki * kj;
#pragma unroll
                    for (int m = 0; m <= SD; ++m) t *= pw[m][TBL.k[DOF][m] - (m == i ? 1 : 0) - (m == j ? 1 : 0)];
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
                for (int i = 0; i <= SD; ++i) s += G[i][d1] * H[i][d2];
                tab[h++] = s;
            }
    }
}

template <int SD, int N, int ORDER, int DOF>
__device__ __forceinline__ void bern_dof_store(const double (&pw)[SD + 1][N + 1], const double (&G)[SD + 1][SD], bool image,
                                               double* lds, double* gout, size_t off, int npts, size_t tstride) {
    constexpr int NTAB = bern_binom(SD + ORDER, SD);
    double tab[NTAB];
    bern_dof<SD, N, ORDER, DOF>(pw, G, tab);
    const size_t e = off + (size_t)DOF * npts;
    if (image) {  // (uniform) LDS image
#pragma unroll
        for (int t = 0; t < NTAB; ++t) lds[e + t * tstride] = tab[t];
    } else {      // streaming: plain stores, the L2 joins the partial lines of neighbouring lanes and rows
#pragma unroll
        for (int t = 0; t < NTAB; ++t) gout[e + t * tstride] = tab[t];
    }
}

template <int SD, int N, int ORDER, int... DOFS>
__device__ __forceinline__ void bern_all_dofs(std::integer_sequence<int, DOFS...>, const double (&pw)[SD + 1][N + 1],
                                              const double (&G)[SD + 1][SD], bool image, double* lds, double* gout, size_t off,
                                              int npts, size_t tstride) {
    (bern_dof_store<SD, N, ORDER, DOFS>(pw, G, image, lds, gout, off, npts, tstride), ...);
}

// Compile-time instance: SD, degree N <= 6, ORDER <= 2.
template <int SD, int N, int ORDER>
__global__ __launch_bounds__(64) void tabulate_bernstein(const BernArgs a) {
    constexpr int NDOF = BernDofs<SD, N>::NDOF;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const size_t tstride = (size_t)NDOF * a.npts;
    bern_items(a, lds, [&](long long req, size_t off, bool active, double* gout) {
        const int pl = (int)(off % a.npts);
        double lam[SD + 1], G[SD + 1][SD];
        bern_setup<SD>(a, req, pl, lam, G);
        double pw[SD + 1][N + 1];
#pragma unroll
        for (int i = 0; i <= SD; ++i) {
            pw[i][0] = 1.0;
#pragma unroll
            for (int j = 1; j <= N; ++j) pw[i][j] = pw[i][j - 1] * lam[i];
        }
        if (!active) return;
        bern_all_dofs<SD, N, ORDER>(std::make_integer_sequence<int, NDOF>{}, pw, G, a.image != 0, lds, gout, off, a.npts, tstride);
    });
}

// ---------------------------------------------------------------------------------------------------------------------
// Generic instance: runtime degree n <= 16 and order.  The chain-rule coefficients c_o[alpha][beta] (Cartesian table alpha
// in mis(SD, o) order, barycentric multi-index beta in mis(SD+1, o) order) are built in LDS by the recursion
//   c_o[alpha][beta] = sum_{i: beta_i > 0} G[i][d] c_{o-1}[alpha - e_d][beta - e_i],   d = first direction of alpha,
// once per workgroup on the element's cell, per request with cells.  Each lane then walks its dofs and tables.

template <int M> __device__ __forceinline__ int bern_rank(int o, const int (&a)[M]) {
    int r = 0, rem = o;
#pragma unroll
    for (int p = 0; p < M - 1; ++p) {
        const int i = rem - a[p];
        r += bern_binom(i + M - p - 2, M - p - 1);
        rem = i;
    }
    return r;
}

template <int M> __device__ __forceinline__ void bern_unrank(int o, int t, int (&a)[M]) {
    int rem = o;
#pragma unroll
    for (int p = 0; p < M - 1; ++p) {
        int i = 0;
        while (i < rem && bern_binom(i + 1 + M - p - 2, M - p - 1) <= t) ++i;
        t -= bern_binom(i + M - p - 2, M - p - 1);
        a[p] = rem - i;
        rem = i;
    }
    a[M - 1] = rem;
}

template <int M> __device__ __forceinline__ bool bern_next(int (&a)[M]) {
    int p = -1;
#pragma unroll
    for (int q = 0; q < M - 1; ++q)
        if (a[q] > 0) p = q;
    if (p < 0) return false;
    int tail = 1;
#pragma unroll
    for (int q = 0; q < M; ++q)
        if (q > p) tail += a[q];
#pragma unroll
    for (int q = 0; q < M; ++q) {
        if (q == p) a[q] -= 1;
        if (q > p) a[q] = (q == p + 1) ? tail : 0;
    }
    return true;
}

__host__ __device__ constexpr int bern_coef_size(int sd, int order) {
    int s = 0;
    for (int o = 0; o <= order; ++o) s += bern_binom(o + sd - 1, sd - 1) * bern_binom(o + sd, sd);
    return s;
}

// c for one cell into `c` (csize doubles); lanes lane0, lane0 + nl, ... of the wave share the work
template <int SD>
__device__ __forceinline__ void bern_chain_coefs(double* c, const double (&G)[SD + 1][SD], int order, int lane0, int nl) {
    if (lane0 == 0) c[0] = 1.0;
    int off_prev = 0, off = 1;
    for (int o = 1; o <= order; ++o) {
        wave_lds_fence();
        const int nt = bern_binom(o + SD - 1, SD - 1), nb = bern_binom(o + SD, SD);
        const int nbp = bern_binom(o - 1 + SD, SD);
        for (int e = lane0; e < nt * nb; e += nl) {
            const int t = e / nb, b = e - t * nb;
            int al[SD], be[SD + 1];
            bern_unrank<SD>(o, t, al);
            bern_unrank<SD + 1>(o, b, be);
            int d = 0;
#pragma unroll
            for (int q = SD - 1; q >= 0; --q)
                if (al[q] > 0) d = q;
            double g[SD + 1];
#pragma unroll
            for (int i = 0; i <= SD; ++i) {
                g[i] = G[i][0];
#pragma unroll
                for (int q = 1; q < SD; ++q)
                    if (d == q) g[i] = G[i][q];
            }
#pragma unroll
            for (int q = 0; q < SD; ++q)
                if (q == d) al[q] -= 1;
            const int tp = bern_rank<SD>(o - 1, al);
            double s = 0.0;
#pragma unroll
            for (int i = 0; i <= SD; ++i) {
                if (be[i] > 0) {
                    int bm[SD + 1];
#pragma unroll
                    for (int q = 0; q <= SD; ++q) bm[q] = be[q] - (q == i ? 1 : 0);
                    s += g[i] * c[off_prev + tp * nbp + bern_rank<SD + 1>(o - 1, bm)];
                }
            }
            c[off + e] = s;
        }
        off_prev = off;
        off += nt * nb;
    }
    wave_lds_fence();
}

template <int SD>
__global__ __launch_bounds__(64) void tabulate_bernstein_generic(const BernArgs a) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int lane = threadIdx.x & 63;
    const int n = a.n, order = a.order, npts = a.npts;
    const int csize = bern_coef_size(SD, order);
    const bool per_request = a.verts != nullptr;
    if (!per_request) {  // the element's cell: one set of coefficients for the whole launch
        double G[SD + 1][SD];
#pragma unroll
        for (int i = 0; i <= SD; ++i)
#pragma unroll
            for (int d = 0; d < SD; ++d) G[i][d] = a.G[i * SD + d];
        bern_chain_coefs<SD>(lds, G, order, lane, 64);
    }
    double nfact = 1.0;
    for (int j = 2; j <= n; ++j) nfact *= j;
    const size_t tstride = (size_t)a.ndof * npts;
    const long long reqsize = (long long)a.ntab * tstride;

    for (long long item = blockIdx.x; item < a.nitems; item += gridDim.x) {
        const long long r0 = item * a.P;
        const long long left = a.nreq - r0;
        const int Pcur = left < a.P ? (int)left : a.P;
        const int nslots = Pcur * npts;
        for (int s0 = 0; s0 < nslots; s0 += 64) {
            const int slot = s0 + lane;
            const bool active = slot < nslots;
            const int rl = active ? slot / npts : 0;
            const int pl = active ? slot - rl * npts : 0;
            const long long req = r0 + rl;
            double lam[SD + 1], G[SD + 1][SD];
            bern_setup<SD>(a, req, pl, lam, G);
            const double* c = lds;
            if (per_request) {
                // the coefficients of request rl: built by its lane of point 0 (npts <= 64 here, all requests of the
                // item are in this pass)
                double* cr = lds + (size_t)rl * csize;
                wave_lds_fence();  // the previous item is done reading
                if (active && pl == 0) bern_chain_coefs<SD>(cr, G, order, 0, 1);
                wave_lds_fence();
                c = cr;
            }
            if (!active) continue;
            double* dst = a.out + (size_t)req * reqsize + pl;
            int k[SD + 1] = {};
            k[0] = n;
            for (int dof = 0; dof < a.ndof; ++dof, bern_next<SD + 1>(k)) {
                int t0 = 0, off = 0;
                for (int o = 0; o <= order; ++o) {
                    const int nt = bern_binom(o + SD - 1, SD - 1), nb = bern_binom(o + SD, SD);
                    for (int t = 0; t < nt; ++t) {
                        double s = 0.0;
                        int be[SD + 1] = {};
                        be[0] = o;
                        for (int b = 0; b < nb; ++b, bern_next<SD + 1>(be)) {
                            const double cf = c[off + t * nb + b];
                            bool ok = true;
                            double den = 1.0, val = 1.0;
#pragma unroll
                            for (int i = 0; i <= SD; ++i) {
                                const int e = k[i] - be[i];
                                if (e < 0) ok = false;
                                for (int j = 2; j <= e; ++j) den *= j;
                                for (int j = 0; j < e; ++j) val *= lam[i];
                            }
                            if (ok) s += cf * (nfact / den) * val;
                        }
                        dst[(size_t)(t0 + t) * tstride + (size_t)dof * npts] = s;
                    }
                    t0 += nt;
                    off += nt * nb;
                }
            }
        }
    }
}

}  // namespace fxk
