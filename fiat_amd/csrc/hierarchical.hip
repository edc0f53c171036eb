// Host side of the IntegratedLegendre kernels (hierarchical.hpp): libfiat_amd_hier.so, a companion of libfiat_amd.so
// (include/fiat_amd_hier.h).  It links against the main library and uses its error slot and contexts.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/fiat_amd_hier.h"
#include "hierarchical.hpp"
#include "host_common.hpp"

namespace {

// which route a shape takes
struct HierPlan {
    int P, image, ndof, ntab;
    long long reqsize;
    size_t lds;
};

int make_plan(const char* who, int sd, int degree, int order, int npts, HierPlan* p) {
    if (sd < 1 || sd > 3) return fail(FX_EINVAL, "%s: spatial dimension %d (intervals, triangles and tetrahedra)", who, sd);
    if (degree < 0 || order < 0 || npts < 0) return fail(FX_EINVAL, "%s: negative degree, order or count", who);
    if (degree < 1 || degree > fxk::HIER_MAXK) return fail(FX_ENOTIMPL, "%s: degree %d (1..%d)", who, degree, fxk::HIER_MAXK);
    if (order > fxk::HIER_MAXORDER) return fail(FX_ENOTIMPL, "%s: derivative order %d > %d", who, order, fxk::HIER_MAXORDER);
    p->ndof = fxk::hier_binom(degree + sd, sd);
    p->ntab = fxk::hier_binom(sd + order, sd);
    p->reqsize = (long long)p->ntab * p->ndof * npts;
    if (p->reqsize >= (1LL << 31)) return fail(FX_ENOTIMPL, "%s: request of %lld entries", who, p->reqsize);
    const ItemPlan ip = plan_items(npts, p->reqsize, fxk::HIER_IMAGE_BYTES, true);
    p->P = ip.P;
    p->image = ip.image;
    p->lds = ip.image_bytes;
    return FX_OK;
}

hipError_t launch(int sd, int degree, int order, unsigned grid, size_t lds, hipStream_t s, const fxk::HierArgs& a) {
    return dispatch_int<1, 3>(sd, [&](auto SD) {
        return dispatch_int<1, fxk::HIER_MAXK>(degree, [&](auto K) {
            return dispatch_int<0, fxk::HIER_MAXORDER>(order, [&](auto ORDER) {
                return launch_wave64(fxk::hier_kernel<SD(), K(), ORDER()>, grid, lds, s, a);
            });
        });
    });
}

}  // namespace

extern "C" {

int fx_hier_abi_version(void) { return 1; }

int fx_hier_descriptor(int sd, int degree, int* rows) {
    if (!rows) return fail(FX_EINVAL, "fx_hier_descriptor: null result");
    if (sd < 1 || sd > 3) return fail(FX_EINVAL, "fx_hier_descriptor: spatial dimension %d (intervals, triangles and tetrahedra)", sd);
    if (degree < 1 || degree > 64) return fail(FX_EINVAL, "fx_hier_descriptor: degree %d (1..64)", degree);
    const int ndof = fxk::hier_fill(sd, degree, nullptr);
    std::vector<int> packed((size_t)ndof);
    fxk::hier_fill(sd, degree, packed.data());
    for (int i = 0; i < ndof; ++i)
        for (int j = 0; j < 4; ++j) rows[(size_t)i * 4 + j] = fxk::hier_field(packed[i], j);
    return FX_OK;
}

int fx_hier_kernel(int sd, int degree, int order, int npts, char* buf, int n) {
    if (!buf || n <= 0) return fail(FX_EINVAL, "fx_hier_kernel: no buffer");
    HierPlan p;
    const int rc = make_plan("fx_hier_kernel", sd, degree, order, npts, &p);
    if (rc != FX_OK) return rc;
    snprintf(buf, (size_t)n, "fxk::hier_kernel<%d,%d,%d> %s P=%d", sd, degree, order, p.image ? "image" : "stream", p.P);
    return FX_OK;
}

int fx_hier_tabulate_batch(fx_ctx* ctx, int sd, int degree, int order, const double* scales, const double* pts, int64_t nreq,
                           int npts, double* out, void* stream, const double* A, const double* b) {
    const char* who = "fx_hier_tabulate_batch";
    if (!ctx || !scales || !A || !b) return fail(FX_EINVAL, "%s: null context, scales or cell map", who);
    if (nreq < 0) return fail(FX_EINVAL, "%s: negative degree, order or count", who);
    HierPlan p;
    const int rc = make_plan(who, sd, degree, order, npts, &p);
    if (rc != FX_OK) return rc;
    for (int i = 0; i < sd * sd; ++i)
        if (!std::isfinite(A[i])) return fail(FX_EINVAL, "%s: the cell map is not finite", who);
    for (int i = 0; i < sd; ++i)
        if (!std::isfinite(b[i])) return fail(FX_EINVAL, "%s: the cell map is not finite", who);
    for (int i = 0; i <= sd; ++i)
        if (!std::isfinite(scales[i])) return fail(FX_EINVAL, "%s: the scales are not finite", who);
    if (nreq == 0 || npts == 0) return FX_OK;
    if (!pts || !out) return fail(FX_EINVAL, "%s: null device pointer", who);

    int device = 0, num_cu = 0, lds_per_cu = 0;
    fx::ctx_facts(ctx, &device, &num_cu, &lds_per_cu);
    if ((long long)p.lds > (long long)lds_per_cu) return fail(FX_ENOTIMPL, "%s: %zu bytes of LDS", who, p.lds);
    fxk::HierArgs a;
    memset(&a, 0, sizeof a);
    a.pts = pts;
    a.out = out;
    // rows of the map, padded with zero rows (FIAT/expansions.py:43-51), and the gradients of the factors of every
    // codimension (:54-63): fb = (y + z) / 2, fa = x + fb + 1, fc = fb^2 with (x, y, z) = X[codim .. codim + 2]
    double J[5][3] = {};
    for (int i = 0; i < sd; ++i) {
        a.b0[i] = b[i];
        for (int d = 0; d < sd; ++d) J[i][d] = a.A0[i * 3 + d] = A[i * sd + d];
    }
    for (int c = 0; c < sd; ++c) {
        for (int d = 0; d < 3; ++d) {
            a.dfb[c * 3 + d] = 0.5 * (J[c + 1][d] + J[c + 2][d]);
            a.dfa[c * 3 + d] = J[c][d] + a.dfb[c * 3 + d];
        }
        int h = 0;
        for (int d1 = 0; d1 < sd; ++d1)
            for (int d2 = d1; d2 < sd; ++d2) a.ddfc[c * 6 + h++] = 2.0 * a.dfb[c * 3 + d1] * a.dfb[c * 3 + d2];
    }
    for (int i = 0; i <= sd; ++i) a.scales[i] = scales[i];
    a.nreq = nreq;
    a.npts = npts;
    a.P = p.P;
    a.image = p.image;
    a.nitems = (nreq + p.P - 1) / p.P;
    FX_HIP_TRY(hipSetDevice(device));
    FX_HIP_TRY(launch(sd, degree, order, item_grid(a.nitems, num_cu, 64), p.lds, (hipStream_t)stream, a));
    return FX_OK;
}

}  // extern "C"
