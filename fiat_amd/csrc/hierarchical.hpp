// IntegratedLegendre on simplices, tabulated directly from the C0 hierarchy (gfx950).
//
// Reference behaviour: IntegratedLegendre(k) (FIAT/hierarchical.py:103-114) is a Ciarlet element over the bubble-variant
// expansion set.  Its nodal coefficient matrix is diagonal: dof i is the i-th member of the C0 hierarchy
// (FIAT/expansions.py:270-322) times a scale that depends on the dimension of the dof's entity only.  So the table needs no
// coefficient contraction: it is the integrated-Jacobi Dubiner recurrence (expansions.py:140-267, variant "bubble"), the
// corrections that turn members into vertex, edge and face functions, and one multiplication per entry.
//
// Lane <-> (request, point) and the image / streaming routes are those of dpc.hpp; the item plan is host_common.hpp
// plan_items, the flush store.hpp flush_item.  The recurrence is a
// depth-first walk unrolled at compile time: the p-chain, per p the q-chain, per (p, q) the r-chain, two live members per
// level.  Members are kept in their final normalisation (the ratios of the level norms are folded into the step
// coefficients, as plan.hpp does on the host), coefficients and output rows are compile-time constants.
//
// The corrections couple chains:  (0,0,0) <- -(0,0,0) - sum of the degree-1 members;  (0,i[,j]) <- (0,i[,j]) - (1,i-1[,j]);
// on the tetrahedron (0,0,i) <- (0,0,i) - (0,1,i-1) - (1,0,i-1).  Two chains of the last codimension whose prefixes have the
// same sum run the SAME linear recurrence (its coefficients depend on that sum only), so a difference of their members is
// the chain of the difference of their seeds.  Hence, on both output routes and with no second pass over any row:
//   * the q-chains of p = 0 and p = 1 advance in lockstep; (0,q,0) - (1,q-1,0) seeds the r-chain of the corrected (0,q,.);
//   * (0,0,i) - [(0,1,.) + (1,0,.)](i-1): the r-chain of (0,0,.) advances in lockstep with ONE chain seeded by
//     (0,1,0) + (1,0,0);
//   * the vertex function of vertex 0 is accumulated in registers while the degree-1 members pass and written after them.
// Every row is written exactly once, by the lane that owns the point.
#pragma once
#include <hip/hip_runtime.h>

#include "store.hpp"

namespace fxk {

constexpr int HIER_IMAGE_BYTES = 40 * 1024;      // per wave: four one-wave workgroups per CU
constexpr int HIER_MAXK = 6, HIER_MAXORDER = 2;  // compile-time instances

struct HierArgs {
    const double* pts;  // [nreq][npts][sd]
    double* out;        // [nreq][ntab][ndof][npts]
    double A0[9], b0[3];  // X = A0 x + b0: the element's cell onto the (-1, 1)^sd simplex
    double dfa[9], dfb[9];  // [codim][d]: gradients of the collapsed-coordinate factors fa, fb (uniform: the map is affine)
    double ddfc[18];        // [codim][h]: Hessian of fc = fb^2, h over d1 <= d2
    double scales[4];       // per entity dimension
    long long nreq, nitems;
    int npts;
    int P;      // whole requests per item
    int image;  // 1: per-wave LDS image of the item, 0: streaming stores
};

__host__ __device__ constexpr int hier_binom(int a, int b) {
    if (b < 0 || a < b) return 0;
    long long r = 1;
    for (int j = 0; j < b; ++j) r = r * (a - j) / (j + 1);
    return (int)r;
}

// ---- the dof table ------------------------------------------------------------------------------------------------------
// One packed row per dof: the member's lattice index (p, q, r) in bits 0-7, 8-15, 16-23 and the dimension of the dof's entity
// in bits 24-31, in the order in which the reference leaves the C0 members (expansions.py:297-322): vertices, edges, faces,
// interior.
__host__ __device__ constexpr int hier_pack(int p, int q, int r, int dim) { return p | q << 8 | r << 16 | dim << 24; }
__host__ __device__ constexpr int hier_field(int row, int i) { return (row >> (8 * i)) & 0xff; }

// rows of IntegratedLegendre(k) on the simplex of dimension sd into rows[] (nullptr: count only); returns their number
__host__ __device__ constexpr int hier_fill(int sd, int k, int* rows) {
    int n = 0;
    auto put = [&](int p, int q, int r, int dim) {
        if (rows) rows[n] = hier_pack(p, q, r, dim);
        ++n;
    };
    if (sd == 1) {
        put(0, 0, 0, 0);
        put(1, 0, 0, 0);
        for (int i = 2; i <= k; ++i) put(i, 0, 0, 1);
    } else if (sd == 2) {
        put(0, 0, 0, 0);
        put(1, 0, 0, 0);
        put(0, 1, 0, 0);
        for (int i = 2; i <= k; ++i) put(1, i - 1, 0, 1);
        for (int i = 2; i <= k; ++i) put(0, i, 0, 1);
        for (int i = 2; i <= k; ++i) put(i, 0, 0, 1);
        for (int j = 1; j <= k; ++j)
            for (int i = 2; i <= k - j; ++i) put(i, j, 0, 2);
    } else {
        put(0, 0, 0, 0);
        put(1, 0, 0, 0);
        put(0, 1, 0, 0);
        put(0, 0, 1, 0);
        for (int i = 2; i <= k; ++i) put(0, 1, i - 1, 1);
        for (int i = 2; i <= k; ++i) put(1, 0, i - 1, 1);
        for (int i = 2; i <= k; ++i) put(1, i - 1, 0, 1);
        for (int i = 2; i <= k; ++i) put(0, 0, i, 1);
        for (int i = 2; i <= k; ++i) put(0, i, 0, 1);
        for (int i = 2; i <= k; ++i) put(i, 0, 0, 1);
        for (int j = 1; j <= k; ++j)
            for (int i = 2; i <= k - j; ++i) put(1, i - 1, j, 2);
        for (int j = 1; j <= k; ++j)
            for (int i = 2; i <= k - j; ++i) put(0, i, j, 2);
        for (int j = 1; j <= k; ++j)
            for (int i = 2; i <= k - j; ++i) put(i, 0, j, 2);
        for (int j = 1; j <= k; ++j)
            for (int i = 2; i <= k - j; ++i) put(i, j, 0, 2);
        for (int l = 1; l <= k; ++l)
            for (int j = 1; j <= k - l; ++j)
                for (int i = 2; i <= k - j - l; ++i) put(i, j, l, 3);
    }
    return n;
}

template <int SD, int K> struct HierDofs {
    static constexpr int NDOF = hier_binom(K + SD, SD);
    static_assert(hier_fill(SD, K, nullptr) == NDOF, "one dof per member");
    int row[NDOF];
    constexpr HierDofs() : row{} { hier_fill(SD, K, row); }
    // the row of member (p, q, r)
    constexpr int find(int p, int q, int r) const {
        for (int i = 0; i < NDOF; ++i)
            if ((row[i] & 0xffffff) == hier_pack(p, q, r, 0)) return i;
        return -1;
    }
};

// ---- the step coefficients ----------------------------------------------------------------------------------------------
__host__ __device__ constexpr double hier_csqrt(double x) {
    if (!(x > 0.0)) return 0.0;
    double r = x > 1.0 ? x : 1.0;  // Newton from above: monotone
    for (int it = 0; it < 128; ++it) {
        const double n = 0.5 * (r + x / r);
        if (!(n < r)) break;
        r = n;
    }
    return r;
}

// the part of the level norm (expansions.py:251-266, variant "bubble") that varies along a chain: prefix sum s, member i
__host__ __device__ constexpr double hier_norm2(int s, int i) {
    const int al = 2 * s - 1;
    return (i > 0 && i + al > 0) ? double(i + al) * double(2 * i + al) / double(i) : 1.0;
}

struct HierCoef {
    double A, B, C;
};

// step i -> i + 1 of a chain whose prefix sums to s, members in final normalisation:
//   m_{i+1} = (A fa - B fb) m_i - C fc m_{i-1}      (integrated_jrc(2 s, 0, i); a = b = -1/2 at i = 0)
__host__ __device__ constexpr HierCoef hier_coef(int s, int i) {
    double a = -0.5, b = -0.5, c = 0.0;
    if (i == 1) {
        a = (2.0 * s + 2.0) / 2.0;
        b = (2.0 * s - 2.0) / 2.0;
    } else if (i > 1) {  // jrc(2 s - 1, 1, i - 1)
        const double ja = 2.0 * s - 1.0, jb = 1.0, t = ja + jb;
        const int n = i - 1;
        a = (2 * n + 1 + t) * (2 * n + 2 + t) / (2 * (n + 1) * (n + 1 + t));
        b = t * (ja - jb) * (2 * n + 1 + t) / (2 * (n + 1) * (n + 1 + t) * (2 * n + t));
        c = (n + ja) * (n + jb) * (2 * n + 2 + t) / ((n + 1) * (n + 1 + t) * (2 * n + t));
    }
    const double up = hier_csqrt(hier_norm2(s, i + 1) / hier_norm2(s, i));
    const double up2 = i > 0 ? hier_csqrt(hier_norm2(s, i + 1) / hier_norm2(s, i - 1)) : 0.0;
    return HierCoef{a * up, b * up, c * up2};
}

// the normalised first member: -sqrt(1 / |K|) prod_d sqrt((d + 1/2) / d), |K| the volume of the (-1, 1)^sd simplex
__host__ __device__ constexpr double hier_phi0(int sd) {
    return -hier_csqrt(sd == 1 ? 3.0 / 4.0 : sd == 2 ? 15.0 / 16.0 : 105.0 / 64.0);
}

template <int SD, int ORDER> struct HierJet {
    static constexpr int NH = SD * (SD + 1) / 2;
    double v;
    double g[ORDER >= 1 ? SD : 1];
    double h[ORDER >= 2 ? NH : 1];
};

template <int SD, int ORDER> __device__ __forceinline__ void hier_axpy(HierJet<SD, ORDER>& y, double w, const HierJet<SD, ORDER>& x) {
    y.v += w * x.v;
    if constexpr (ORDER >= 1) {
#pragma unroll
        for (int d = 0; d < SD; ++d) y.g[d] += w * x.g[d];
    }
    if constexpr (ORDER >= 2) {
#pragma unroll
        for (int h = 0; h < HierJet<SD, ORDER>::NH; ++h) y.h[h] += w * x.h[h];
    }
}

// y = w x
template <int SD, int ORDER> __device__ __forceinline__ void hier_scaled(HierJet<SD, ORDER>& y, double w, const HierJet<SD, ORDER>& x) {
    y.v = w * x.v;
    if constexpr (ORDER >= 1) {
#pragma unroll
        for (int d = 0; d < SD; ++d) y.g[d] = w * x.g[d];
    }
    if constexpr (ORDER >= 2) {
#pragma unroll
        for (int h = 0; h < HierJet<SD, ORDER>::NH; ++h) y.h[h] = w * x.h[h];
    }
}

// The walk of one lane.  Everything the steps read besides the jets: the lane's factors fa, fb per codimension, the uniform
// derivative tables of the kernel arguments, and where the lane's entries go.
template <int SD, int K, int ORDER> struct HierWalk {
    typedef HierJet<SD, ORDER> Jet;
    static constexpr int NH = Jet::NH;
    static constexpr int NTAB = hier_binom(SD + ORDER, SD);

    const HierArgs& a;
    double fa[SD], fb[SD];  // (the last codimension: fb = -1, fc = 1, no derivatives)
    bool image;
    double* lds;
    int li;        // image: index of the lane's (t = 0, row 0) entry
    double* gp;    // stream: pointer to it
    int rs;        // row stride (npts), opaque
    int tstride;   // table stride
    Jet v0;        // the function of vertex 0, accumulated

    __device__ __forceinline__ HierWalk(const HierArgs& a_) : a(a_) {}

    // one step of codimension CODIM with compile-time coefficients; FIRST: two-term step (prv is not read).  Derivatives by
    // the product rule in closed form; every uniform factor stays a scalar operand (no uniform product is formed: it would
    // be loop-invariant and hoisted out of the item loop into live registers).
    template <int CODIM, bool FIRST, bool FLAT = false>
    __device__ __forceinline__ void step(Jet& nw, const Jet& cur, const Jet& prv, const double A, const double B, const double C) const {
        constexpr bool LAST = CODIM == SD - 1;
        const double* dfa = a.dfa + 3 * CODIM;
        const double* dfb = a.dfb + 3 * CODIM;
        const double* ddfc = a.ddfc + 6 * CODIM;
        double f, g = 0.0;
        if constexpr (LAST) {
            f = A * fa[CODIM] + B;
            if constexpr (!FIRST) g = -C;
        } else {
            f = A * fa[CODIM] - B * fb[CODIM];
            if constexpr (!FIRST) g = -C * (fb[CODIM] * fb[CODIM]);
        }
        nw.v = cur.v * f;
        if constexpr (!FIRST) nw.v += prv.v * g;
        if constexpr (ORDER >= 1) {
            const double tA = A * cur.v;
            double tB = 0.0, u = 0.0;
            if constexpr (!LAST) tB = B * cur.v;
            if constexpr (!LAST && !FIRST) u = (-2.0 * C) * fb[CODIM] * prv.v;
#pragma unroll
            for (int d = 0; d < SD; ++d) {
                double t = tA * dfa[d];
                if constexpr (!FLAT) t += cur.g[d] * f;
                if constexpr (!LAST) t -= tB * dfb[d];
                if constexpr (!FIRST) t += prv.g[d] * g;
                if constexpr (!LAST && !FIRST) t += u * dfb[d];
                nw.g[d] = t;
            }
        }
        if constexpr (ORDER >= 2) {
            double Ag[SD], Bg[SD], w[SD];
#pragma unroll
            for (int d = 0; d < SD; ++d) {
                if constexpr (!FLAT) Ag[d] = A * cur.g[d];
                if constexpr (!LAST && !FLAT) Bg[d] = B * cur.g[d];
                if constexpr (!LAST && !FIRST) w[d] = (-2.0 * C) * fb[CODIM] * prv.g[d];
            }
            const double tC = -C * prv.v;
            int h = 0;
#pragma unroll
            for (int d1 = 0; d1 < SD; ++d1)
#pragma unroll
                for (int d2 = d1; d2 < SD; ++d2) {
                    double t = 0.0;
                    if constexpr (!FLAT) t = cur.h[h] * f + Ag[d2] * dfa[d1] + Ag[d1] * dfa[d2];
                    if constexpr (!LAST && !FLAT) t -= Bg[d2] * dfb[d1] + Bg[d1] * dfb[d2];
                    if constexpr (!FIRST) t += prv.h[h] * g;
                    if constexpr (!LAST && !FIRST) t += w[d2] * dfb[d1] + w[d1] * dfb[d2] + tC * ddfc[h];
                    nw.h[h] = t;
                    ++h;
                }
        }
    }

    // FLAT: cur is the constant member (its derivatives are zero and are not read)
    template <int CODIM, int S, int I, bool FLAT = false> __device__ __forceinline__ void advance(Jet& nw, const Jet& cur, const Jet& prv) const {
        constexpr HierCoef c = hier_coef(S, I);
        static_assert(!FLAT || I == 0, "the constant member starts chains only");
        step<CODIM, I == 0, FLAT>(nw, cur, prv, c.A, c.B, c.C);
    }

    // the tables of one row, scaled, into the image or to HBM.  ROW is a compile-time constant; the offset is ROW times the
    // opaque run-time stride, one integer multiply-add per row.
    template <int ROW> __device__ __forceinline__ void store_row(const Jet& m) const {
        constexpr HierDofs<SD, K> TBL{};
        constexpr int DIM = hier_field(TBL.row[ROW], 3);
        const double s = a.scales[DIM];
        double tab[NTAB];
        tab[0] = s * m.v;
        if constexpr (ORDER >= 1) {
#pragma unroll
            for (int d = 0; d < SD; ++d) tab[1 + d] = s * m.g[d];
        }
        if constexpr (ORDER >= 2) {
#pragma unroll
            for (int h = 0; h < NH; ++h) tab[1 + SD + h] = s * m.h[h];
        }
        const int off = ROW * rs;
        if (image) {  // (uniform)
#pragma unroll
            for (int t = 0; t < NTAB; ++t) lds[li + off + t * tstride] = tab[t];
        } else {
            double* p = gp + off;
#pragma unroll
            for (int t = 0; t < NTAB; ++t) p[(size_t)t * (size_t)tstride] = tab[t];
        }
        // the walk is one straight line: the fence keeps a row's stores where the row is finished, ahead of the next steps
        __builtin_amdgcn_sched_barrier(0);
    }

    // a finished member: the constant starts the function of vertex 0, the degree-1 members are vertex functions and are
    // subtracted from it, everything else is its own row
    template <int P, int Q, int R> __device__ __forceinline__ void finish(const Jet& m) {
        constexpr HierDofs<SD, K> TBL{};
        constexpr int ROW = TBL.find(P, Q, R);
        static_assert(ROW >= 0, "a member of the lattice");
        if constexpr (P + Q + R == 0) {
            hier_scaled<SD, ORDER>(v0, -1.0, m);
        } else {
            if constexpr (P + Q + R == 1) hier_axpy<SD, ORDER>(v0, -1.0, m);
            store_row<ROW>(m);
        }
    }

    // ---- chains ---------------------------------------------------------------------------------------------------------
    // cur = (P, Q, R), prv = (P, Q, R - 1)
    template <int P, int Q, int R> __device__ __forceinline__ void rchain(const Jet& cur, const Jet& prv) {
        finish<P, Q, R>(cur);
        if constexpr (P + Q + R < K) {
            Jet nw;
            advance<2, P + Q, R>(nw, cur, prv);
            rchain<P, Q, R + 1>(nw, cur);
        }
    }

    // member (P, Q, 0) [corrected where the hierarchy corrects it] is known: a row on the triangle, a seed on the tetrahedron
    template <int P, int Q> __device__ __forceinline__ void level1(const Jet& m) {
        if constexpr (SD == 2) finish<P, Q, 0>(m);
        else rchain<P, Q, 0>(m, m);
    }

    template <int P, int Q> __device__ __forceinline__ void qchain(const Jet& cur, const Jet& prv) {
        level1<P, Q>(cur);
        if constexpr (P + Q < K) {
            Jet nw;
            advance<1, P, Q>(nw, cur, prv);
            qchain<P, Q + 1>(nw, cur);
        }
    }

    template <int P> __device__ __forceinline__ void pchain(const Jet& cur, const Jet& prv) {
        if constexpr (SD == 1) finish<P, 0, 0>(cur);
        else qchain<P, 0>(cur, cur);
        if constexpr (P < K) {
            Jet nw;
            advance<0, 0, P>(nw, cur, prv);
            pchain<P + 1>(nw, cur);
        }
    }

    // tetrahedron: the edge chain (0, 0, R) in lockstep with T(R - 1) = (0, 1, R - 1) + (1, 0, R - 1), the chain of the seed
    // t0 = (0, 1, 0) + (1, 0, 0).  e = (0, 0, R), ep = (0, 0, R - 1), t = T(R - 1), tp = T(R - 2).
    template <int R> __device__ __forceinline__ void edge00(const Jet& e, const Jet& ep, const Jet& t, const Jet& tp, const Jet& t0) {
        if constexpr (R < 2) {
            finish<0, 0, R>(e);
        } else {
            Jet c = e;
            hier_axpy<SD, ORDER>(c, -1.0, t);
            finish<0, 0, R>(c);
        }
        if constexpr (R < K) {
            Jet en, tn;
            advance<2, 0, R, R == 0>(en, e, ep);
            if constexpr (R == 0) tn = t0;
            else advance<2, 1, R - 1>(tn, t, tp);
            edge00<R + 1>(en, e, tn, t, t0);
        }
    }

    // triangle and tetrahedron: the q-chains of p = 0 and p = 1 in lockstep.  c0 = (0, Q, 0), p0 = (0, Q - 1, 0),
    // c1 = (1, Q - 1, 0), p1 = (1, Q - 2, 0); m1 = (1, 0, 0).
    template <int Q> __device__ __forceinline__ void lock01(const Jet& c0, const Jet& p0, const Jet& c1, const Jet& p1, const Jet& m1) {
        Jet n0;
        if constexpr (Q < K) advance<1, 0, Q, Q == 0>(n0, c0, p0);
        if constexpr (Q == 0 && SD == 3) {
            Jet t0 = n0;  // (K >= 1)
            hier_axpy<SD, ORDER>(t0, 1.0, m1);
            edge00<0>(c0, c0, t0, t0, t0);
        } else if constexpr (Q < 2) {
            level1<0, Q>(c0);
        } else {
            Jet c = c0;
            hier_axpy<SD, ORDER>(c, -1.0, c1);
            level1<0, Q>(c);
        }
        if constexpr (Q >= 1) level1<1, Q - 1>(c1);
        if constexpr (Q < K) {
            Jet n1;
            if constexpr (Q == 0) n1 = m1;
            else advance<1, 1, Q - 1>(n1, c1, p1);
            lock01<Q + 1>(n0, c0, n1, c1, m1);
        }
    }

    __device__ __forceinline__ void run() {
        constexpr HierDofs<SD, K> TBL{};
        constexpr double PHI0 = hier_phi0(SD);
        Jet m0;
        m0.v = PHI0;
        if constexpr (ORDER >= 1) {
#pragma unroll
            for (int d = 0; d < SD; ++d) m0.g[d] = 0.0;
        }
        if constexpr (ORDER >= 2) {
#pragma unroll
            for (int h = 0; h < NH; ++h) m0.h[h] = 0.0;
        }
        if constexpr (SD == 1) {
            pchain<0>(m0, m0);
            store_row<TBL.find(0, 0, 0)>(v0);
        } else {
            Jet m1;
            advance<0, 0, 0, true>(m1, m0, m0);
            lock01<0>(m0, m0, m1, m1, m1);
            store_row<TBL.find(0, 0, 0)>(v0);
            if constexpr (K >= 2) {
                Jet m2;
                advance<0, 0, 1>(m2, m1, m0);
                pchain<2>(m2, m1);
            }
        }
    }
};

template <int SD, int K, int ORDER>
__global__ __launch_bounds__(64) void hier_kernel(const HierArgs a) {
    static_assert(SD >= 1 && SD <= 3, "interval, triangle, tetrahedron");
    static_assert(K >= 1 && K <= HIER_MAXK && ORDER >= 0 && ORDER <= HIER_MAXORDER, "compile-time instances");
    constexpr int NTAB = hier_binom(SD + ORDER, SD);
    constexpr int NDOF = HierDofs<SD, K>::NDOF;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int lane = threadIdx.x & 63;
    const int npts = a.npts;
    const int tstride = NDOF * npts;                         // (a request has fewer than 2^31 entries)
    const long long reqsize = (long long)NTAB * tstride;
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
            double X[SD];
#pragma unroll
            for (int i = 0; i < SD; ++i) {
                double t = a.b0[i];
#pragma unroll
                for (int d = 0; d < SD; ++d) t += a.A0[i * 3 + d] * pp[d];
                X[i] = t;
            }
            HierWalk<SD, K, ORDER> w(a);
#pragma unroll
            for (int c = 0; c < SD; ++c) {
                if (c == SD - 1) {
                    w.fb[c] = -1.0;
                    w.fa[c] = X[c];
                } else {
                    const double z = c + 2 < SD ? X[c + 2 < SD ? c + 2 : 0] : -1.0;
                    w.fb[c] = 0.5 * (X[c + 1] + z);
                    w.fa[c] = X[c] + (w.fb[c] + 1.0);
                }
            }
            int rs = npts;  // (opaque per item: the row offsets are formed here, one multiply-add each, never hoisted)
            asm volatile("" : "+v"(rs));
            const size_t off = (size_t)rl * reqsize + pl;   // the lane's (t = 0, row 0) entry from the start of the item
            w.image = a.image != 0;
            w.lds = lds;
            w.li = (int)off;
            w.gp = gout + off;
            w.rs = rs;
            w.tstride = tstride;
            w.run();
        }
        if (a.image) flush_item(gout, lds, (long long)Pcur * reqsize, lane);
    }
}

}  // namespace fxk
