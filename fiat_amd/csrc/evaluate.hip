// Host side of the fused evaluation kernels (evaluate.hpp): libfiat_amd_eval.so, a companion of libfiat_amd.so
// (include/fiat_amd_eval.h).  It links against the main library and uses its error slot and contexts.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/fiat_amd_eval.h"
#include "evaluate.hpp"
#include "host_common.hpp"
#include <memory>

struct fx_eval_element {
    fx_ctx* ctx = nullptr;
    int sd = 0, n = 0, variant = 0, ndof = 0, vdim = 1, nexp = 0;
    double phi0 = 0.0;
    double A0[9] = {0}, b0[3] = {0};
    DeviceBuffer<double> d_Ap;    // A'[ndof][vdim][nexp], columns in the order of the walk
    DeviceBuffer<double> d_coef;  // [nexp][3]
};

namespace {

const double UFC_VERTS[3][12] = {{0, 1}, {0, 0, 1, 0, 0, 1}, {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1}};

// the instance set: what is outside it is FX_ENOTIMPL, what is malformed FX_EINVAL
int check_set(const char* who, int sd, int degree, int variant, int vdim) {
    if (sd < 1 || sd > 3) return fail(FX_EINVAL, "%s: spatial dimension %d (intervals, triangles and tetrahedra)", who, sd);
    if (degree < 0) return fail(FX_EINVAL, "%s: negative degree", who);
    if (variant < 0 || variant > 2) return fail(FX_EINVAL, "%s: invalid variant %d", who, variant);
    if (vdim < 1) return fail(FX_EINVAL, "%s: %d components", who, vdim);
    if (degree < 1 || degree > fxk::EVAL_MAXK) return fail(FX_ENOTIMPL, "%s: degree %d (1..%d)", who, degree, fxk::EVAL_MAXK);
    if (variant == 2) return fail(FX_ENOTIMPL, "%s: the dual variant of the expansion set", who);
    if (vdim != 1 && vdim != sd) return fail(FX_ENOTIMPL, "%s: %d components (value shape () or (%d,))", who, vdim, sd);
    return FX_OK;
}

// which item scheme a shape takes
struct EvalPlan {
    int P, chunks, ntab, nexp;
    long long reqsize;
    size_t lds;
};

size_t lds_bytes(int P, int ndof, int vn, int image) {
    return (size_t)(fxk::eval_lds_c(P, ndof) + fxk::eval_lds_w(P, vn) + ((image + 1) & ~1)) * 8;
}

int make_plan(const char* who, int sd, int degree, int order, int vdim, int ndof, int npts, int nrhs, EvalPlan* p) {
    if (order < 0 || npts < 0) return fail(FX_EINVAL, "%s: negative order or count", who);
    if (ndof < 1) return fail(FX_EINVAL, "%s: %d dofs", who, ndof);
    if (nrhs < 1 || nrhs > fxk::EVAL_MAXRHS) return fail(FX_EINVAL, "%s: %d right-hand sides (1..%d)", who, nrhs, fxk::EVAL_MAXRHS);
    if (order > fxk::EVAL_MAXORDER) return fail(FX_ENOTIMPL, "%s: derivative order %d > %d", who, order, fxk::EVAL_MAXORDER);
    p->ntab = fxk::eval_binom(sd + order, sd);
    p->nexp = fxk::eval_binom(degree + sd, sd);
    p->reqsize = (long long)p->ntab * nrhs * vdim * npts;
    if (p->reqsize >= (1LL << 31)) return fail(FX_ENOTIMPL, "%s: request of %lld entries", who, p->reqsize);
    if ((long long)ndof * vdim * p->nexp >= (1LL << 31)) return fail(FX_ENOTIMPL, "%s: %d dofs", who, ndof);
    const int vn = vdim * p->nexp;
    if (npts > 64) {
        p->P = 1;
        p->chunks = (npts + 63) / 64;
        p->lds = lds_bytes(1, ndof, vn, 0);
    } else {
        // whole requests per 64 lanes, shrunk to those whose dofs, w and image fit the budget
        const int per = p->ntab * vdim * npts;
        int P = npts > 0 ? 64 / npts : 1;
        while (P > 1 && lds_bytes(P, ndof, vn, P * per) > (size_t)fxk::EVAL_LDS_BYTES) --P;
        p->P = P;
        p->chunks = 1;
        p->lds = lds_bytes(P, ndof, vn, P * per);
    }
    if (p->lds > 64 * 1024) return fail(FX_ENOTIMPL, "%s: %zu bytes of LDS for one request", who, p->lds);
    return FX_OK;
}

// (sd, vdim): value shape () or (sd,)
template <int SD, int VDIM, class... Args> hipError_t launch_order(int order, unsigned grid, size_t lds, hipStream_t s, const Args&... args) {
    return dispatch_int<0, fxk::EVAL_MAXORDER>(order, [&](auto ORDER) {
        return launch_wave64(fxk::eval_kernel<SD, ORDER(), VDIM>, grid, lds, s, args...);
    });
}

template <int SD> void cell_map(const double* v, double* A, double* b) { fxk::eval_cell_map<SD>(v, A, b); }

}  // namespace

extern "C" {

int fx_eval_abi_version(void) { return 1; }

int fx_eval_walk_order(int sd, int degree, int* members) {
    if (!members) return fail(FX_EINVAL, "fx_eval_walk_order: null result");
    const int rc = check_set("fx_eval_walk_order", sd, degree, 0, 1);
    if (rc != FX_OK) return rc;
    const fx::EvalTables t = fx::eval_tables(sd, degree, 0, 1.0);
    for (int k = 0; k < t.nexp; ++k) members[k] = t.member[(size_t)k];
    return FX_OK;
}

int fx_eval_fold(int sd, int degree, int variant, int ndof, int vdim, const double* coeffs, double* folded) {
    if (!coeffs || !folded) return fail(FX_EINVAL, "fx_eval_fold: null argument");
    if (ndof < 1) return fail(FX_EINVAL, "fx_eval_fold: %d dofs", ndof);
    const int rc = check_set("fx_eval_fold", sd, degree, variant, vdim);
    if (rc != FX_OK) return rc;
    const fx::EvalTables t = fx::eval_tables(sd, degree, variant, 1.0);
    const std::vector<double> F = fx::eval_fold(sd, degree, variant, ndof, vdim, coeffs, t.member);
    memcpy(folded, F.data(), F.size() * sizeof(double));
    return FX_OK;
}

int fx_eval_element_create(fx_ctx* ctx, int sd, int degree, int variant, double scale, const double* cell, int ndof, int vdim,
                           const double* coeffs, fx_eval_element** elem) {
    const char* who = "fx_eval_element_create";
    if (!ctx || !coeffs || !elem) return fail(FX_EINVAL, "%s: null argument", who);
    if (ndof < 1) return fail(FX_EINVAL, "%s: %d dofs", who, ndof);
    const int rc = check_set(who, sd, degree, variant, vdim);
    if (rc != FX_OK) return rc;
    const int nexp = fxk::eval_binom(degree + sd, sd);
    if ((long long)ndof * vdim * nexp >= (1LL << 31)) return fail(FX_ENOTIMPL, "%s: %d dofs", who, ndof);
    for (size_t i = 0; i < (size_t)ndof * vdim * nexp; ++i)
        if (!std::isfinite(coeffs[i])) return fail(FX_EINVAL, "%s: the coefficients are not finite", who);
    if (!(scale > 0.0)) {  // the default: sqrt(1 / |(-1, 1)^sd simplex|)
        double vol = 1.0;
        for (int i = 1; i <= sd; ++i) vol *= 2.0 / i;
        scale = std::sqrt(1.0 / vol);
    }
    std::unique_ptr<fx_eval_element> e(new fx_eval_element);
    e->ctx = ctx;
    e->sd = sd;
    e->n = degree;
    e->variant = variant;
    e->ndof = ndof;
    e->vdim = vdim;
    e->nexp = nexp;
    const double* v = cell ? cell : UFC_VERTS[sd - 1];
    double A[9], b[3];
    sd == 1 ? cell_map<1>(v, A, b) : sd == 2 ? cell_map<2>(v, A, b) : cell_map<3>(v, A, b);
    for (int i = 0; i < sd * sd; ++i) {
        if (!std::isfinite(A[i])) return fail(FX_EINVAL, "%s: degenerate cell", who);
        e->A0[i] = A[i];
    }
    for (int i = 0; i < sd; ++i) e->b0[i] = b[i];
    const fx::EvalTables t = fx::eval_tables(sd, degree, variant, scale);
    e->phi0 = t.phi0;
    const std::vector<double> F = fx::eval_fold(sd, degree, variant, ndof, vdim, coeffs, t.member);
    int device = 0, num_cu = 0, lds_per_cu = 0;
    fx::ctx_facts(ctx, &device, &num_cu, &lds_per_cu);
    hipError_t he = hipSetDevice(device);
    if (he == hipSuccess) he = e->d_Ap.upload(F.data(), F.size());
    if (he == hipSuccess) he = e->d_coef.upload(t.coef.data(), t.coef.size());
    if (he != hipSuccess) {
        (void)hipGetLastError();  // (a failed hipSetDevice)
        return fail(FX_EHIP, "%s: %s", who, hipGetErrorString(he));
    }
    *elem = e.release();
    return FX_OK;
}

int fx_eval_element_destroy(fx_eval_element* e) {
    delete e;
    return FX_OK;
}

int fx_eval_kernel(int sd, int degree, int order, int vdim, int ndof, int npts, int nrhs, char* buf, int n) {
    const char* who = "fx_eval_kernel";
    if (!buf || n <= 0) return fail(FX_EINVAL, "%s: no buffer", who);
    int rc = check_set(who, sd, degree, 0, vdim);
    if (rc != FX_OK) return rc;
    EvalPlan p;
    rc = make_plan(who, sd, degree, order, vdim, ndof, npts, nrhs, &p);
    if (rc != FX_OK) return rc;
    snprintf(buf, (size_t)n, "fxk::eval_kernel<%d,%d,%d> degree=%d P=%d chunks=%d", sd, order, vdim, degree, p.P, p.chunks);
    return FX_OK;
}

int fx_eval_batch(fx_ctx* ctx, const fx_eval_element* e, int mapping, int order, int64_t nreq, int npts, int nrhs, const double* pts,
                  const double* verts, const double* dofs, double* out, void* stream) {
    const char* who = "fx_eval_batch";
    if (!ctx || !e) return fail(FX_EINVAL, "%s: null context or element", who);
    if (e->ctx != ctx) return fail(FX_EINVAL, "%s: the element belongs to another context", who);
    if (nreq < 0) return fail(FX_EINVAL, "%s: negative order or count", who);
    if (mapping < 0 || mapping > 5) return fail(FX_EINVAL, "%s: unknown mapping %d", who, mapping);
    if (mapping > FX_MAP_CONTRAVARIANT_PIOLA) return fail(FX_ENOTIMPL, "%s: the double Piola maps", who);
    if (mapping != FX_MAP_AFFINE && (e->vdim != e->sd || e->sd < 2))
        return fail(FX_EINVAL, "%s: Piola maps need vector-valued functions with value shape (%d,), got %d components", who, e->sd, e->vdim);
    EvalPlan p;
    const int rc = make_plan(who, e->sd, e->n, order, e->vdim, e->ndof, npts, nrhs, &p);
    if (rc != FX_OK) return rc;
    if (mapping != FX_MAP_AFFINE && !verts && nreq > 0 && npts > 0)
        return fail(FX_EINVAL, "%s: a Piola push-forward needs the physical cells (verts)", who);
    if (nreq == 0 || npts == 0) return FX_OK;
    if (!pts || !dofs || !out) return fail(FX_EINVAL, "%s: null device pointer", who);

    int device = 0, num_cu = 0, lds_per_cu = 0;
    fx::ctx_facts(ctx, &device, &num_cu, &lds_per_cu);
    if ((long long)p.lds > (long long)lds_per_cu) return fail(FX_ENOTIMPL, "%s: %zu bytes of LDS", who, p.lds);
    fxk::EvalArgs a;
    memset(&a, 0, sizeof a);
    for (int i = 0; i < e->sd * e->sd; ++i) {
        a.A0[i] = e->A0[i];
        a.G[i] = 0.5 * e->A0[i];
    }
    for (int i = 0; i < e->sd; ++i) a.b0[i] = e->b0[i];
    a.phi0 = e->phi0;
    a.nreq = nreq;
    a.npts = npts;
    a.nrhs = nrhs;
    a.ndof = e->ndof;
    a.nexp = e->nexp;
    a.n = e->n;
    a.P = p.P;
    a.chunks = p.chunks;
    a.mapping = mapping;
    a.nitems = p.chunks > 1 ? nreq * p.chunks : (nreq + p.P - 1) / p.P;
    const unsigned grid = item_grid(a.nitems, num_cu, fxk::EVAL_GRID_PER_CU);
    hipStream_t s = (hipStream_t)stream;
    FX_HIP_TRY(hipSetDevice(device));
    const bool vec = e->vdim > 1;
    const double *Ap = e->d_Ap.get(), *coef = e->d_coef.get();
    hipError_t he;
    if (e->sd == 1) he = launch_order<1, 1>(order, grid, p.lds, s, a, pts, verts, dofs, Ap, coef, out);
    else if (e->sd == 2) he = vec ? launch_order<2, 2>(order, grid, p.lds, s, a, pts, verts, dofs, Ap, coef, out)
                                  : launch_order<2, 1>(order, grid, p.lds, s, a, pts, verts, dofs, Ap, coef, out);
    else he = vec ? launch_order<3, 3>(order, grid, p.lds, s, a, pts, verts, dofs, Ap, coef, out)
                  : launch_order<3, 1>(order, grid, p.lds, s, a, pts, verts, dofs, Ap, coef, out);
    FX_HIP_TRY(he);
    return FX_OK;
}

}  // extern "C"
