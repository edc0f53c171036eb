// Evaluation of finite element functions at points, fused (gfx950): out = sum_i dofs[i] D^alpha phi_i(x), no table in HBM.
//
// Reference behaviour: the contraction of FiniteElement.tabulate (FIAT/finite_element.py:181-197) with a dof vector.  With A the
// nodal coefficients over the expansion set, u = c^T (A Phi) = (A^T c)^T Phi: one small transform w = A^T c per request
// (nexp * vdim numbers), then one depth-first walk of the Dubiner recurrence (FIAT/expansions.py:140-267) per point in which
// every member is multiplied into ntab * vdim accumulators as it appears and then forgotten.
//
// What is compiled in and what is data.  Template parameters: the spatial dimension, the derivative order and the number of
// components (1 or sd).  Run-time tables: the degree (1..6), the step coefficients of the recurrence in the order of the walk
// (three doubles per member, the level norms folded in as plan.hpp does, read with uniform indices: scalar loads) and the
// coefficients A'[ndof][vdim][nexp], columns in the order of the walk.  The bubble variant's C0 transform is folded into A' on
// the host (eval_fold), so the kernel only ever walks the raw recurrence.  15 instances.
//
// Lane <-> (request, point), items of whole requests and a per-wave LDS image as in dpc.hpp / hierarchical.hpp; the image is
// per right-hand side, so the kernel flushes it itself (store.hpp flush_block) instead of through flush_item.  A
// request of more than 64 points is chunked by points: an item is then one chunk of one request, every chunk RECOMPUTES w
// (ndof * vdim * nexp / 64 FMAs per lane against nexp * ntab * vdim and the steps of the walk: a few per cent, and no wave
// waits for another), and its rows, 64 consecutive doubles each, leave as full-width stores straight from the registers.
// Right-hand sides: the walk is repeated per right-hand side inside the one launch (accumulators for 8 right-hand sides of a
// vector-valued order-2 instance would be 480 VGPRs); points, cell maps and the factors of the collapsed coordinates are set
// up once per item.  Cost: nrhs walks instead of one; each right-hand side runs the single-rhs instruction sequence, so
// its result is the single-rhs result bit for bit.
//
// The per-lane walk and the geometry are __host__ __device__ and compile as plain C++ (tools/evaluate_walk_host.cpp runs them
// on the CPU, under the sanitizers).
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "store.hpp"
#define FXE_HD __host__ __device__ __forceinline__
#else
#define FXE_HD inline
#endif

#include <cmath>
#include <vector>

#include "plan.hpp"

namespace fxk {

constexpr int EVAL_MAXK = 6, EVAL_MAXORDER = 2, EVAL_MAXRHS = 8;  // degrees, orders, right-hand sides of one call
constexpr int EVAL_LDS_BYTES = 16 * 1024;  // per wave: dofs, w and the image of an item; the item shrinks to what fits
constexpr int EVAL_RB = 4;                 // requests whose transforms share one read of A'
constexpr int EVAL_GRID_PER_CU = 32;       // workgroups (of one wave) per compute unit at most

constexpr int eval_binom(int a, int b) {
    if (b < 0 || a < b) return 0;
    long long r = 1;
    for (int j = 0; j < b; ++j) r = r * (a - j) / (j + 1);
    return (int)r;
}

// ---- geometry of one lane -----------------------------------------------------------------------------------------------
// X = A x + b maps the request's cell onto the (-1, 1)^SD simplex (rows of A: gradients of X_i); the factors of the collapsed
// coordinates per codimension and their gradients (FIAT/expansions.py:43-63); the last codimension has fb = -1, fc = 1.
template <int SD> struct EvalGeom {
    double fa[SD], fb[SD];
    double dfa[SD][SD], dfb[SD][SD];  // [codim][d]
};

// the map of the simplex with vertices v[SD + 1][SD] onto the (-1, 1)^SD simplex: A row-major [SD][SD]
template <int SD> FXE_HD void eval_cell_map(const double* v, double* A, double* b) {
    if constexpr (SD == 1) {
        A[0] = 2.0 / (v[1] - v[0]);
    } else if constexpr (SD == 2) {
        const double e00 = v[2] - v[0], e10 = v[3] - v[1], e01 = v[4] - v[0], e11 = v[5] - v[1];
        const double inv = 2.0 / (e00 * e11 - e01 * e10);
        A[0] = e11 * inv;
        A[1] = -e01 * inv;
        A[2] = -e10 * inv;
        A[3] = e00 * inv;
    } else {
        double e[3][3];
        for (int c = 0; c < 3; ++c)
            for (int r = 0; r < 3; ++r) e[r][c] = v[3 * (c + 1) + r] - v[r];
        const double c00 = e[1][1] * e[2][2] - e[1][2] * e[2][1];
        const double c01 = e[1][2] * e[2][0] - e[1][0] * e[2][2];
        const double c02 = e[1][0] * e[2][1] - e[1][1] * e[2][0];
        const double inv = 2.0 / (e[0][0] * c00 + e[0][1] * c01 + e[0][2] * c02);
        A[0] = c00 * inv;
        A[1] = (e[0][2] * e[2][1] - e[0][1] * e[2][2]) * inv;
        A[2] = (e[0][1] * e[1][2] - e[0][2] * e[1][1]) * inv;
        A[3] = c01 * inv;
        A[4] = (e[0][0] * e[2][2] - e[0][2] * e[2][0]) * inv;
        A[5] = (e[0][2] * e[1][0] - e[0][0] * e[1][2]) * inv;
        A[6] = c02 * inv;
        A[7] = (e[0][1] * e[2][0] - e[0][0] * e[2][1]) * inv;
        A[8] = (e[0][0] * e[1][1] - e[0][1] * e[1][0]) * inv;
    }
    for (int i = 0; i < SD; ++i) {
        double t = -1.0;
        for (int d = 0; d < SD; ++d) t -= A[i * SD + d] * v[d];
        b[i] = t;
    }
}

template <int SD> FXE_HD void eval_geom(const double* A, const double* b, const double* x, EvalGeom<SD>& g) {
    double X[SD + 2], J[SD + 2][SD];
    for (int i = 0; i < SD + 2; ++i) {
        double t = i < SD ? b[i] : -1.0;
        for (int d = 0; d < SD; ++d) {
            J[i][d] = i < SD ? A[i * SD + d] : 0.0;
            t += J[i][d] * x[d];
        }
        X[i] = t;
    }
    for (int c = 0; c < SD; ++c) {
        if (c == SD - 1) {
            g.fb[c] = -1.0;
            g.fa[c] = X[c];
        } else {
            g.fb[c] = 0.5 * (X[c + 1] + X[c + 2]);
            g.fa[c] = X[c] + (g.fb[c] + 1.0);
        }
        for (int d = 0; d < SD; ++d) {
            g.dfb[c][d] = c == SD - 1 ? 0.0 : 0.5 * (J[c + 1][d] + J[c + 2][d]);
            g.dfa[c][d] = J[c][d] + g.dfb[c][d];
        }
    }
}

// The matrix of the Piola maps of one cell, as aux_kernels.hpp: J = E G with E the edge matrix of the physical cell (columns
// v_i - v_0) and G = A0 / 2 of the element's own cell; kind 1 (covariant): J^-T, kind 2 (contravariant): J / det J.
template <int SD> FXE_HD void eval_piola_matrix(const double* v, const double* G, int kind, double (&M)[SD][SD]) {
    double J[SD][SD];
    for (int r = 0; r < SD; ++r)
        for (int c = 0; c < SD; ++c) {
            double t = 0.0;
            for (int k = 0; k < SD; ++k) t += (v[(k + 1) * SD + r] - v[r]) * G[k * SD + c];
            J[r][c] = t;
        }
    double det, inv[SD][SD];
    if constexpr (SD == 1) {
        det = J[0][0];
        inv[0][0] = 1.0 / det;
    } else if constexpr (SD == 2) {
        det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
        inv[0][0] = J[1][1] / det;
        inv[0][1] = -J[0][1] / det;
        inv[1][0] = -J[1][0] / det;
        inv[1][1] = J[0][0] / det;
    } else {
        const double c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1];
        const double c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2];
        const double c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
        det = J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02;
        inv[0][0] = c00 / det;
        inv[0][1] = (J[0][2] * J[2][1] - J[0][1] * J[2][2]) / det;
        inv[0][2] = (J[0][1] * J[1][2] - J[0][2] * J[1][1]) / det;
        inv[1][0] = c01 / det;
        inv[1][1] = (J[0][0] * J[2][2] - J[0][2] * J[2][0]) / det;
        inv[1][2] = (J[0][2] * J[1][0] - J[0][0] * J[1][2]) / det;
        inv[2][0] = c02 / det;
        inv[2][1] = (J[0][1] * J[2][0] - J[0][0] * J[2][1]) / det;
        inv[2][2] = (J[0][0] * J[1][1] - J[0][1] * J[1][0]) / det;
    }
    for (int r = 0; r < SD; ++r)
        for (int c = 0; c < SD; ++c) M[r][c] = kind == 1 ? inv[c][r] : J[r][c] / det;
}

// ---- the walk of one lane -----------------------------------------------------------------------------------------------
template <int SD, int ORDER> struct EvalJet {
    static constexpr int NH = SD * (SD + 1) / 2;
    double v;
    double g[ORDER >= 1 ? SD : 1];
    double h[ORDER >= 2 ? NH : 1];  // d1 <= d2, the order of mis(SD, 2)
};

template <int SD, int ORDER> FXE_HD void eval_jet_const(EvalJet<SD, ORDER>& j, double v) {
    j.v = v;
    for (int d = 0; d < (ORDER >= 1 ? SD : 1); ++d) j.g[d] = 0.0;
    for (int h = 0; h < (ORDER >= 2 ? EvalJet<SD, ORDER>::NH : 1); ++h) j.h[h] = 0.0;
}

// nw = (A fa - B fb) cur - C fb^2 prv of codimension CODIM, derivatives by the product rule (the factors are at most
// quadratic).  The first step of a chain has C = 0 and is given prv = cur.
template <int SD, int ORDER, int CODIM>
FXE_HD void eval_step(EvalJet<SD, ORDER>& nw, const EvalJet<SD, ORDER>& cur, const EvalJet<SD, ORDER>& prv, const EvalGeom<SD>& G,
                      const double* abc) {
    constexpr bool LAST = CODIM == SD - 1;
    const double A = abc[0], B = abc[1], C = abc[2];
    const double fa = G.fa[CODIM], fb = G.fb[CODIM];
    const double f = LAST ? A * fa + B : A * fa - B * fb;
    const double g = LAST ? -C : -C * (fb * fb);
    nw.v = cur.v * f + prv.v * g;
    if constexpr (ORDER >= 1) {
        double df[SD], dg[SD];
        for (int d = 0; d < SD; ++d) {
            df[d] = LAST ? A * G.dfa[CODIM][d] : A * G.dfa[CODIM][d] - B * G.dfb[CODIM][d];
            dg[d] = LAST ? 0.0 : (-2.0 * C) * fb * G.dfb[CODIM][d];
        }
        for (int d = 0; d < SD; ++d) {
            double t = cur.g[d] * f + cur.v * df[d] + prv.g[d] * g;
            if constexpr (!LAST) t += prv.v * dg[d];
            nw.g[d] = t;
        }
        if constexpr (ORDER >= 2) {
            int h = 0;
            for (int d1 = 0; d1 < SD; ++d1)
                for (int d2 = d1; d2 < SD; ++d2) {
                    double t = cur.h[h] * f + cur.g[d1] * df[d2] + cur.g[d2] * df[d1] + prv.h[h] * g;
                    if constexpr (!LAST)
                        t += prv.g[d1] * dg[d2] + prv.g[d2] * dg[d1] + prv.v * ((-2.0 * C) * G.dfb[CODIM][d1] * G.dfb[CODIM][d2]);
                    nw.h[h] = t;
                    ++h;
                }
        }
    }
}

template <int SD, int ORDER, int VDIM>
FXE_HD void eval_accumulate(double (&acc)[eval_binom(SD + ORDER, SD)][VDIM], const EvalJet<SD, ORDER>& m, const double* w, int wstride,
                            int k) {
    for (int v = 0; v < VDIM; ++v) {
        const double wv = w[v * wstride + k];
        acc[0][v] += wv * m.v;
        if constexpr (ORDER >= 1)
            for (int d = 0; d < SD; ++d) acc[1 + d][v] += wv * m.g[d];
        if constexpr (ORDER >= 2)
            for (int h = 0; h < EvalJet<SD, ORDER>::NH; ++h) acc[1 + SD + h][v] += wv * m.h[h];
    }
}

// acc[t][v] += sum_k w[v][k] D^t member_k(x): members k in the order of the walk (p slowest, then q, then r), two live members
// per level; coef[k] = (A, B, C) of the step that produces member k (coef[0] is not read), phi0 the constant member.
template <int SD, int ORDER, int VDIM>
FXE_HD void eval_walk(int n, double phi0, const double* coef, const double* w, int wstride, const EvalGeom<SD>& G,
                      double (&acc)[eval_binom(SD + ORDER, SD)][VDIM]) {
    typedef EvalJet<SD, ORDER> Jet;
    Jet pc, pp;
    eval_jet_const<SD, ORDER>(pc, phi0);
    pp = pc;
    int k = 0;
    for (int p = 0; p <= n; ++p) {
        if (p > 0) {
            Jet nw{};
            eval_step<SD, ORDER, 0>(nw, pc, pp, G, coef + 3 * k);
            pp = pc;
            pc = nw;
        }
        if constexpr (SD == 1) {
            eval_accumulate<SD, ORDER, VDIM>(acc, pc, w, wstride, k);
            ++k;
        } else {
            Jet qc = pc, qp = pc;
            for (int q = 0; q <= n - p; ++q) {
                if (q > 0) {
                    Jet nw{};
                    eval_step<SD, ORDER, 1>(nw, qc, qp, G, coef + 3 * k);
                    qp = qc;
                    qc = nw;
                }
                if constexpr (SD == 2) {
                    eval_accumulate<SD, ORDER, VDIM>(acc, qc, w, wstride, k);
                    ++k;
                } else {
                    Jet rc = qc, rp = qc;
                    for (int r = 0; r <= n - p - q; ++r) {
                        if (r > 0) {
                            Jet nw{};
                            eval_step<SD, ORDER, 2>(nw, rc, rp, G, coef + 3 * k);
                            rp = rc;
                            rc = nw;
                        }
                        eval_accumulate<SD, ORDER, VDIM>(acc, rc, w, wstride, k);
                        ++k;
                    }
                }
            }
        }
    }
}

// the Piola matrix applied to the components of every accumulator (VDIM == SD)
template <int SD, int NTAB> FXE_HD void eval_apply_piola(double (&acc)[NTAB][SD], const double (&M)[SD][SD]) {
    for (int t = 0; t < NTAB; ++t) {
        double y[SD];
        for (int r = 0; r < SD; ++r) {
            double s = 0.0;
            for (int c = 0; c < SD; ++c) s += M[r][c] * acc[t][c];
            y[r] = s;
        }
        for (int r = 0; r < SD; ++r) acc[t][r] = y[r];
    }
}

}  // namespace fxk

// ---- host tables ----------------------------------------------------------------------------------------------------------
namespace fx {

struct EvalTables {
    int nexp = 0;
    double phi0 = 0.0;
    std::vector<int> member;   // walk position -> member index of the expansion set
    std::vector<double> coef;  // [nexp][3]: (A, B, C) of the step that produces the member at that position
};

inline EvalTables eval_tables(int sd, int n, int variant, double scale) {
    EvalTables t;
    const Program prog = build_program(sd, n, variant, scale);
    t.nexp = prog.nexp;
    t.phi0 = prog.phi0;
    for (int p = 0; p <= n; ++p)
        for (int q = 0; q <= (sd >= 2 ? n - p : 0); ++q)
            for (int r = 0; r <= (sd >= 3 ? n - p - q : 0); ++r) {
                const int idx[3] = {p, q, r};
                t.member.push_back(member_index(sd, idx));
            }
    std::vector<int> pos((size_t)t.nexp, -1);
    for (int k = 0; k < t.nexp; ++k) pos[(size_t)t.member[(size_t)k]] = k;
    t.coef.assign((size_t)t.nexp * 3, 0.0);
    for (const Step& s : prog.steps) {
        double* c = &t.coef[(size_t)pos[(size_t)s.dst] * 3];
        c[0] = s.A;
        c[1] = s.B;
        c[2] = s.prv >= 0 ? s.C : 0.0;
    }
    return t;
}

// A'[ndof][vdim][nexp]: the coefficients over the RAW recurrence (bubble: coeffs . T, the C0 transform folded in), columns in
// the order of the walk
inline std::vector<double> eval_fold(int sd, int n, int variant, int ndof, int vdim, const double* coeffs, const std::vector<int>& member) {
    const int nexp = binom(n + sd, sd), rows = ndof * vdim;
    std::vector<double> C(coeffs, coeffs + (size_t)rows * nexp);
    if (variant == 1) {
        const std::vector<double> T = c0_transform(sd, n);
        std::vector<double> F((size_t)rows * nexp, 0.0);
        for (int i = 0; i < rows; ++i)
            for (int m = 0; m < nexp; ++m) {
                const double c = C[(size_t)i * nexp + m];
                if (c == 0.0) continue;
                for (int k = 0; k < nexp; ++k) F[(size_t)i * nexp + k] += c * T[(size_t)m * nexp + k];
            }
        C.swap(F);
    }
    std::vector<double> out((size_t)rows * nexp);
    for (int i = 0; i < rows; ++i)
        for (int k = 0; k < nexp; ++k) out[(size_t)i * nexp + k] = C[(size_t)i * nexp + member[(size_t)k]];
    return out;
}

}  // namespace fx

#if defined(__HIPCC__)
namespace fxk {

struct EvalArgs {
    double A0[9], b0[3];  // the element's own cell onto the (-1, 1)^sd simplex, A0 row-major [sd][sd]
    double G[9];          // A0 / 2 (Piola maps)
    double phi0;
    long long nreq, nitems;
    int npts, nrhs, ndof, nexp, n;
    int P;        // whole requests per item (npts <= 64), 1 with chunks
    int chunks;   // point chunks per request (1: whole requests)
    int mapping;  // 0 affine, 1 covariant, 2 contravariant Piola
};

// LDS of one wave, in doubles: dofs of the item's requests (rounded up to EVAL_RB requests), w, the image
__host__ __device__ constexpr int eval_lds_c(int P, int ndof) { return ((P + EVAL_RB - 1) / EVAL_RB * EVAL_RB * ndof + 1) & ~1; }
__host__ __device__ constexpr int eval_lds_w(int P, int vn) { return (P * vn + 1) & ~1; }

template <int SD, int ORDER, int VDIM>
__global__ __launch_bounds__(64) void eval_kernel(const EvalArgs a, const double* __restrict__ pts, const double* __restrict__ verts,
                                                  const double* __restrict__ dofs, const double* __restrict__ Ap,
                                                  const double* __restrict__ coef, double* __restrict__ out) {
    static_assert(SD >= 1 && SD <= 3 && ORDER >= 0 && ORDER <= EVAL_MAXORDER && (VDIM == 1 || VDIM == SD), "compile-time instances");
    constexpr int NTAB = eval_binom(SD + ORDER, SD);
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int lane = threadIdx.x & 63;
    const int npts = a.npts, nrhs = a.nrhs, ndof = a.ndof, nexp = a.nexp;
    const int VN = VDIM * nexp;
    const bool whole = a.chunks == 1;
    double* cs = lds;
    double* ws = cs + eval_lds_c(a.P, ndof);
    double* img = ws + eval_lds_w(a.P, VN);
    const int seg = VDIM * npts;                             // one table of one right-hand side of one request
    const size_t reqsize = (size_t)NTAB * nrhs * seg;        // (fewer than 2^31 entries: host)
    for (long long item = blockIdx.x; item < a.nitems; item += gridDim.x) {
        long long r0;
        int Pcur, q0, cnt;
        if (whole) {
            r0 = item * a.P;
            const long long left = a.nreq - r0;
            Pcur = left < a.P ? (int)left : a.P;
            q0 = 0;
            cnt = npts;
        } else {
            r0 = item / a.chunks;
            Pcur = 1;
            q0 = (int)(item - r0 * a.chunks) * 64;
            cnt = npts - q0 < 64 ? npts - q0 : 64;
        }
        const int nslots = Pcur * cnt;  // (at most 64)
        const bool active = lane < nslots;
        const int rl = active ? lane / cnt : 0;
        const int pl = active ? lane - rl * cnt : 0;
        // the lane's point and cell: once per item, for every right-hand side
        EvalGeom<SD> geo;
        {
            const double* pp = pts + ((size_t)(r0 + rl) * npts + q0 + pl) * SD;
            double x[SD], A[SD * SD], b[SD];
#pragma unroll
            for (int d = 0; d < SD; ++d) x[d] = pp[d];
            if (verts) {  // (uniform)
                eval_cell_map<SD>(verts + (size_t)(r0 + rl) * (SD + 1) * SD, A, b);
            } else {
#pragma unroll
                for (int i = 0; i < SD * SD; ++i) A[i] = a.A0[i];
#pragma unroll
                for (int i = 0; i < SD; ++i) b[i] = a.b0[i];
            }
            eval_geom<SD>(A, b, x, geo);
        }
        for (int j = 0; j < nrhs; ++j) {
            // the dof vectors of the item's requests for this right-hand side
            for (int idx = lane; idx < Pcur * ndof; idx += 64) {
                const int rr = idx / ndof;
                cs[idx] = dofs[((size_t)(r0 + rr) * nrhs + j) * ndof + (idx - rr * ndof)];
            }
            wave_lds_fence();
            // w[r][v][k] = sum_i c[r][i] A'[i][v][k]: lanes over (v, k), EVAL_RB requests per read of A'
            for (int x = lane; x < VN; x += 64) {
                for (int rb = 0; rb < Pcur; rb += EVAL_RB) {
                    double s[EVAL_RB];
#pragma unroll
                    for (int u = 0; u < EVAL_RB; ++u) s[u] = 0.0;
                    const double* c = cs + rb * ndof;
                    for (int i = 0; i < ndof; ++i) {
                        const double av = Ap[(size_t)i * VN + x];
#pragma unroll
                        for (int u = 0; u < EVAL_RB; ++u) s[u] += c[u * ndof + i] * av;  // (rows past Pcur: read, never stored)
                    }
#pragma unroll
                    for (int u = 0; u < EVAL_RB; ++u)
                        if (rb + u < Pcur) ws[(rb + u) * VN + x] = s[u];
                }
            }
            wave_lds_fence();
            if (active) {
                double acc[NTAB][VDIM];
#pragma unroll
                for (int t = 0; t < NTAB; ++t)
#pragma unroll
                    for (int v = 0; v < VDIM; ++v) acc[t][v] = 0.0;
                eval_walk<SD, ORDER, VDIM>(a.n, a.phi0, coef, ws + rl * VN, nexp, geo, acc);
                if constexpr (VDIM == SD && SD >= 2) {
                    if (a.mapping != 0) {  // (uniform)
                        double M[SD][SD];
                        eval_piola_matrix<SD>(verts + (size_t)(r0 + rl) * (SD + 1) * SD, a.G, a.mapping, M);
                        eval_apply_piola<SD, NTAB>(acc, M);
                    }
                }
                if (whole) {
#pragma unroll
                    for (int t = 0; t < NTAB; ++t)
#pragma unroll
                        for (int v = 0; v < VDIM; ++v) img[((rl * NTAB + t) * VDIM + v) * npts + pl] = acc[t][v];
                } else {  // rows of up to 64 consecutive doubles, one per lane
                    double* g = out + (size_t)r0 * reqsize + (size_t)j * seg + q0 + pl;
#pragma unroll
                    for (int t = 0; t < NTAB; ++t)
#pragma unroll
                        for (int v = 0; v < VDIM; ++v) stream_store(g + (size_t)t * nrhs * seg + (size_t)v * npts, acc[t][v]);
                }
            }
            if (whole) {
                wave_lds_fence();
                const int total = Pcur * NTAB * seg;
                if (nrhs == 1) {  // the item is one contiguous block
                    double* g = out + (size_t)r0 * reqsize;
                    if ((total & 1) == 0 && (reinterpret_cast<unsigned long long>(g) & 15ull) == 0) {
                        typedef double dv2d __attribute__((ext_vector_type(2)));
                        flush_block(reinterpret_cast<dv2d*>(g), reinterpret_cast<const dv2d*>(img), total >> 1, lane);
                    } else {
                        for (int i = lane; i < total; i += 64) g[i] = img[i];
                    }
                } else {  // segments of one table of this right-hand side, nrhs segments apart
                    double* g = out + ((size_t)r0 * NTAB * nrhs + j) * seg;
                    for (int i = lane; i < total; i += 64) {
                        const int s = i / seg;
                        g[(size_t)s * nrhs * seg + (i - s * seg)] = img[i];
                    }
                }
            }
            wave_lds_fence();  // the next right-hand side, or item, overwrites dofs, w and the image
        }
    }
}

}  // namespace fxk
#endif
