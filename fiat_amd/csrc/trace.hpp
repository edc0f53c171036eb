// The H(div) trace element: one dense facet block per point, zeros elsewhere (gfx950).
//
// Reference behaviour: HDivTrace (FIAT/hdiv_trace.py) carries one discontinuous element per facet of the cell.  Its table
// [ndof][npts], ndof = nfac * nf, holds at point j the values of the facet element of the facet f(j) the point lies on, in
// rows f nf .. (f + 1) nf, and zeros in all other rows.  Without an entity the element decides f(j) itself: with lambda the
// barycentric coordinates of the point on the (simplex) cell, f is the one index with |lambda_f| < 1e-10; a call in which a
// point has no such index, or more than one, is NaN throughout.  The facet coordinates of a point are its barycentric
// coordinates with lambda_f dropped, read on the UFC facet simplex: x_j = the (j + 1)-th of those that are left.
//
// Lane <-> (request, point), the tiling of dpc_kernel and serendipity_kernel: an item is P whole requests (P * npts <= 64;
// one request in chunks of 64 points beyond).  The lane
//   1. (identify mode) forms lambda = lam0 + G x, counts the coordinates inside the tolerance and votes: the verdict of a
//      request is the OR of its lanes' failures (a wave ballot masked to the request's lanes; a chunked request takes a first
//      pass over all of its chunks), so a failed request is NaN throughout and its neighbours in the wave are untouched;
//   2. forms the facet coordinates;
//   3. evaluates the expansion of the facet simplex by recurrence in registers: on the interval the Legendre polynomials
//      P_p(X), X = 2 x - 1; on the triangle a_p(x, y) b_{p,q}(y) of Dubiner's basis without its normalisation,
//        a_0 = 1,  a_{p+1} = (2p+1)/(p+1) (2x + y - 1) a_p - p/(p+1) (y - 1)^2 a_{p-1},
//        b_{p,0} = a_p,  b_{p,q+1} = (A Y + B) b_{p,q} - C b_{p,q-1},  Y = 2 y - 1,  (A, B, C) the Jacobi(2p+1, 0) coefficients,
//      member (p, q) at (p + q)(p + q + 1) / 2 + q; on a point the constant 1;
//   4. contracts it with the facet element's nf x nf matrix, which the host has prepared against exactly this expansion
//      (the normalisation sqrt(2p+1) resp. sqrt((2p+1)(p+q+1)) and the element's scale folded into its columns).
// Compile-time instances (K >= 0) hold the expansion in registers and the matrix in LDS; the run-time-degree instance
// (K = -1, degree <= TRACE_MAXGEN) keeps neither: per dof it walks the recurrence again, two live values per level, against
// coefficients read from a kernel argument of its own (TraceRec) and matrix rows read through the scalar cache from L2.
//
// Output: where an item fits the image it is zeroed in LDS, the lanes write their facet blocks (or NaN columns) into it and
// it leaves as whole-line non-temporal stores (store.hpp flush_item); larger requests stream: every lane stores its own column, zeros
// included, with plain stores.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "store.hpp"

namespace fxk {

// LDS of one (one-wave) workgroup, matrix and image together: four workgroups share the 160 KB of a CU
constexpr int TRACE_LDS_BYTES = 40 * 1024;
constexpr int TRACE_MAXK = 6;      // compile-time instances: degree 0..6
constexpr int TRACE_MAXGEN = 12;   // the run-time-degree instance
constexpr int TRACE_MAXNF = 91;    // members of degree 12 on the triangle
constexpr double TRACE_TOL = 1e-10;

__host__ __device__ constexpr int trace_nf(int fd, int k) { return fd == 0 ? 1 : fd == 1 ? k + 1 : (k + 1) * (k + 2) / 2; }

// the three-term coefficients: a-steps (Legendre: (2p+1)/(p+1), p/(p+1)) and b-steps (Jacobi(2p+1, 0) from q - 1 to q)
__host__ __device__ constexpr double trace_a1(int p) { return (double)(2 * p + 1) / (double)(p + 1); }
__host__ __device__ constexpr double trace_a2(int p) { return (double)p / (double)(p + 1); }
__host__ __device__ constexpr double trace_b(int p, int q, int which) {
    const double s = 2 * p + 1, i = q - 1;
    if (which == 0) return (2 * i + 1 + s) * (2 * i + 2 + s) / (2 * (i + 1) * (i + 1 + s));
    if (which == 1) return s * s * (2 * i + 1 + s) / (2 * (i + 1) * (i + 1 + s) * (2 * i + s));
    return (i + s) * i * (2 * i + 2 + s) / ((i + 1) * (i + 1 + s) * (2 * i + s));
}

struct TraceRec {  // the coefficients of the run-time-degree instance: its second kernel argument, 2.4 KB by value
    double a1[TRACE_MAXGEN + 1], a2[TRACE_MAXGEN + 1];
    double b[TRACE_MAXNF][3];  // by member
};
struct TraceNoRec {};  // the compile-time instances take no coefficients
template <int K> using TraceRecOf = std::conditional_t<(K < 0), TraceRec, TraceNoRec>;

struct TraceArgs {
    const double* pts;   // [nreq][npts][pd]: pd = fd + 1 (cell coordinates) in identify mode, fd (facet coordinates) otherwise
    const int* facets;   // [nreq] flat facet numbers (mode 2)
    const double* C;     // [nf][nf], row = dof of the facet element, column = member of the expansion above
    double* out;         // [nreq][nfac * nf][npts]
    double lam0[4];      // identify mode: lambda_i = lam0[i] + sum_d G[i][d] x_d on the element's cell
    double G[12];        // [fd + 2][fd + 1]
    long long nreq, nitems;
    int npts;
    int P;               // whole requests per item
    int image;           // 1: per-wave LDS image of the item, 0: streaming stores
    int mode;            // 0 identify, 1 one facet (facet), 2 facet per request (facets)
    int facet, nfac, degree;
    int swap;            // the interval: the point where lambda_i vanishes is facet 1 - i
};

// steps 1 and 2: the facet the point is on (false: none, or more than one) and its facet coordinates
template <int FD> __device__ __forceinline__ bool trace_locate(const TraceArgs& a, const double* pp, int& f, double (&x)[FD + 1]) {
    constexpr int SD = FD + 1;
    double lam[SD + 2];
    int cnt = 0;
    f = 0;
#pragma unroll
    for (int i = 0; i <= SD; ++i) {
        double l = a.lam0[i];
#pragma unroll
        for (int d = 0; d < SD; ++d) l += a.G[i * SD + d] * pp[d];
        lam[i] = l;
        if (fabs(l) < TRACE_TOL) {
            ++cnt;
            f = i;
        }
    }
    lam[SD + 1] = 0.0;
#pragma unroll
    for (int j = 0; j < FD; ++j) x[j] = (j + 1 < f) ? lam[j + 1] : lam[j + 2];
    if (a.swap) f = 1 - f;
    return cnt == 1;
}

// step 3, compile-time degree: every member into registers
template <int FD, int K> __device__ __forceinline__ void trace_expand(const double (&x)[FD + 1], double (&phi)[trace_nf(FD, K)]) {
    if constexpr (FD == 0) {
        phi[0] = 1.0;
    } else if constexpr (FD == 1) {
        const double X = 2.0 * x[0] - 1.0;
        phi[0] = 1.0;
        if constexpr (K >= 1) phi[1] = X;
#pragma unroll
        for (int p = 1; p < K; ++p) phi[p + 1] = trace_a1(p) * X * phi[p] - trace_a2(p) * phi[p - 1];
    } else {
        const double u = 2.0 * x[0] + x[1] - 1.0, v = (x[1] - 1.0) * (x[1] - 1.0), Y = 2.0 * x[1] - 1.0;
        phi[0] = 1.0;
#pragma unroll
        for (int p = 0; p <= K; ++p) {
            const int k0 = p * (p + 1) / 2;
            if (p < K) {  // a_{p+1}
                const int k1 = (p + 1) * (p + 2) / 2;
                phi[k1] = trace_a1(p) * u * phi[k0];
                if (p >= 1) phi[k1] -= trace_a2(p) * v * phi[(p - 1) * p / 2];
            }
#pragma unroll
            for (int q = 1; q <= K - p; ++q) {
                const int k = (p + q) * (p + q + 1) / 2 + q, km = (p + q - 1) * (p + q) / 2 + q - 1;
                phi[k] = (trace_b(p, q, 0) * Y + trace_b(p, q, 1)) * phi[km];
                if (q >= 2) phi[k] -= trace_b(p, q, 2) * phi[(p + q - 2) * (p + q - 1) / 2 + q - 2];
            }
        }
    }
}

// steps 3 and 4, run-time degree: one dof, the recurrence walked with two live values per level
template <int FD> __device__ __forceinline__ double trace_walk(const TraceRec& rec, const double* Ci, int n, const double (&x)[FD + 1]) {
    if constexpr (FD == 1) {
        const double X = 2.0 * x[0] - 1.0;
        double pm = 0.0, pc = 1.0, acc = 0.0;
        for (int p = 0; p <= n; ++p) {
            acc += Ci[p] * pc;
            const double pn = rec.a1[p] * X * pc - rec.a2[p] * pm;
            pm = pc;
            pc = pn;
        }
        return acc;
    } else {
        const double u = 2.0 * x[0] + x[1] - 1.0, v = (x[1] - 1.0) * (x[1] - 1.0), Y = 2.0 * x[1] - 1.0;
        double am = 0.0, ac = 1.0, acc = 0.0;
        for (int p = 0; p <= n; ++p) {
            acc += Ci[p * (p + 1) / 2] * ac;
            double bm = 0.0, bc = ac;
            for (int q = 1; q <= n - p; ++q) {
                const int k = (p + q) * (p + q + 1) / 2 + q;
                const double bn = (rec.b[k][0] * Y + rec.b[k][1]) * bc - rec.b[k][2] * bm;
                bm = bc;
                bc = bn;
                acc += Ci[k] * bn;
            }
            const double an = rec.a1[p] * u * ac - rec.a2[p] * v * am;
            am = ac;
            ac = an;
        }
        return acc;
    }
}

template <int FD, int K>
__global__ __launch_bounds__(64) void trace_kernel(const TraceArgs a, const TraceRecOf<K> rec) {
    static_assert(FD >= 0 && FD <= 2 && K >= -1 && K <= TRACE_MAXK, "facets of dimension 0..2, degree 0..6 or run-time");
    static_assert(FD > 0 || K == 0, "a point carries the constant");
    constexpr bool GEN = K < 0;
    constexpr int NF = GEN ? 1 : trace_nf(FD, GEN ? 0 : K);
    constexpr int COFF = GEN ? 0 : (NF * NF + 1) & ~1;  // the image starts 16-byte aligned behind the matrix
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* img = lds + COFF;
    const int lane = threadIdx.x & 63;
    const int npts = a.npts;
    const int nf = GEN ? trace_nf(FD, a.degree) : NF;
    const int ndof = a.nfac * nf;
    const int reqsize = ndof * npts;  // (a request has fewer than 2^31 entries)
    const bool ident = a.mode == 0;
    const int pd = ident ? FD + 1 : FD;
    const double nan = __builtin_nan("");
    if constexpr (!GEN) {
        for (int i = lane; i < NF * NF; i += 64) lds[i] = a.C[i];
        wave_lds_fence();
    }
    for (long long item = blockIdx.x; item < a.nitems; item += gridDim.x) {
        const long long r0 = item * a.P;
        const long long left = a.nreq - r0;
        const int Pcur = left < a.P ? (int)left : a.P;
        const int nslots = Pcur * npts;
        double* gout = a.out + (size_t)r0 * (size_t)reqsize;
        const long long total = (long long)Pcur * reqsize;
        // a chunked request: its verdict over all of its points before any of them is written
        bool chunk_bad = false;
        if (ident && npts > 64) {
            unsigned long long any = 0;
            for (int s0 = 0; s0 < nslots; s0 += 64) {
                bool bad = false;
                if (s0 + lane < nslots) {
                    int f;
                    double x[FD + 1];
                    bad = !trace_locate<FD>(a, a.pts + ((size_t)r0 * npts + s0 + lane) * pd, f, x);
                }
                any |= __ballot(bad);
            }
            chunk_bad = any != 0;
        }
        if (a.image) {
            for (long long i = lane; i < total; i += 64) img[i] = 0.0;
            wave_lds_fence();
        }
        for (int s0 = 0; s0 < nslots; s0 += 64) {
            const int slot = s0 + lane;
            const bool active = slot < nslots;
            const int rl = active ? slot / npts : 0;
            const int pl = slot - rl * npts;
            int f = 0;
            double x[FD + 1];
#pragma unroll
            for (int j = 0; j <= FD; ++j) x[j] = 0.0;
            bool ok = true;
            if (active) {
                const double* pp = a.pts + ((size_t)(r0 + rl) * npts + pl) * pd;
                if (ident) {
                    ok = trace_locate<FD>(a, pp, f, x);
                } else {
                    f = a.mode == 1 ? a.facet : a.facets[r0 + rl];
#pragma unroll
                    for (int j = 0; j < FD; ++j) x[j] = pp[j];
                    ok = (unsigned)f < (unsigned)a.nfac;  // (the host has checked: nothing is ever written outside the request)
                }
            }
            bool bad = chunk_bad || !ok;
            if (npts <= 64) {  // the verdict of the lane's request: the failures among its npts lanes
                const unsigned long long fails = __ballot(active && !ok);
                const unsigned long long ones = npts == 64 ? ~0ull : (1ull << npts) - 1ull;
                bad = (fails & (ones << (rl * npts))) != 0;
            }
            if (!active) continue;
            int rs = npts;  // (opaque per item: the stride stays one register, see dpc.hpp)
            asm volatile("" : "+v"(rs));
            const size_t off = (size_t)rl * (size_t)reqsize + pl;  // the lane's row-0 entry from the start of the item
            if (bad) {
                if (a.image) {
                    int li = (int)off;
                    for (int j = 0; j < ndof; ++j, li += rs) img[li] = nan;
                } else {
                    double* gp = gout + off;
                    for (int j = 0; j < ndof; ++j, gp += rs) *gp = nan;
                }
                continue;
            }
            const int row0 = f * nf;
            if (!a.image) {  // streaming: the zeros of the other facets' blocks
                double* gp = gout + off;
                for (int j = 0; j < ndof; ++j, gp += rs)
                    if (j < row0 || j >= row0 + nf) *gp = 0.0;
            }
            int li = (int)off + row0 * npts;
            double* gp = gout + off + (size_t)row0 * npts;
            if constexpr (GEN) {
                for (int i = 0; i < nf; ++i) {
                    double val = 1.0;
                    if constexpr (FD > 0) val = trace_walk<FD>(rec, a.C + (size_t)i * nf, a.degree, x);
                    if (a.image) img[li] = val; else *gp = val;
                    li += rs;
                    gp += rs;
                }
            } else {
                double phi[NF];
                trace_expand<FD, GEN ? 0 : K>(x, phi);
#pragma unroll
                for (int i = 0; i < NF; ++i) {
                    double val = 0.0;
#pragma unroll
                    for (int k = 0; k < NF; ++k) val += lds[i * NF + k] * phi[k];
                    if (a.image) img[li] = val; else *gp = val;
                    li += rs;
                    gp += rs;
                }
            }
        }
        if (a.image) flush_item(gout, img, total, lane);
    }
}

}  // namespace fxk
