// Host side of the DPC kernels (dpc.hpp): libfiat_amd_dpc.so, a companion of libfiat_amd.so (include/fiat_amd_dpc.h).
// It links against the main library and uses its error slot and contexts.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/fiat_amd_dpc.h"
#include "dpc.hpp"
#include "host_common.hpp"

namespace {

// which route a shape takes
struct DpcPlan {
    int P, image, ndof, ntab;
    long long reqsize;
    size_t lds;
};

int make_plan(const char* who, int sd, int degree, int order, int npts, DpcPlan* p) {
    if (sd != 2 && sd != 3) return fail(FX_EINVAL, "%s: spatial dimension %d (quadrilaterals and hexahedra)", who, sd);
    if (degree < 0 || order < 0 || npts < 0) return fail(FX_EINVAL, "%s: negative degree, order or count", who);
    if (degree < 1 || degree > fxk::DPC_MAXK) return fail(FX_ENOTIMPL, "%s: degree %d (1..%d)", who, degree, fxk::DPC_MAXK);
    if (order > fxk::DPC_MAXORDER) return fail(FX_ENOTIMPL, "%s: derivative order %d > %d", who, order, fxk::DPC_MAXORDER);
    p->ndof = fxk::dpc_binom(degree + sd, sd);
    p->ntab = fxk::dpc_binom(sd + order, sd);
    p->reqsize = (long long)p->ntab * p->ndof * npts;
    if (p->reqsize >= (1LL << 31)) return fail(FX_ENOTIMPL, "%s: request of %lld entries", who, p->reqsize);
    const ItemPlan ip = plan_items(npts, p->reqsize, fxk::DPC_IMAGE_BYTES, true);
    p->P = ip.P;
    p->image = ip.image;
    p->lds = ip.image_bytes;
    return FX_OK;
}

hipError_t launch(int sd, int degree, int order, unsigned grid, size_t lds, hipStream_t s, const fxk::DpcArgs& a) {
    return dispatch_int<2, 3>(sd, [&](auto SD) {
        return dispatch_int<1, fxk::DPC_MAXK>(degree, [&](auto K) {
            return dispatch_int<0, fxk::DPC_MAXORDER>(order, [&](auto ORDER) {
                return launch_wave64(fxk::dpc_kernel<SD(), K(), ORDER()>, grid, lds, s, a);
            });
        });
    });
}

}  // namespace

extern "C" {

int fx_dpc_abi_version(void) { return 1; }

int fx_dpc_descriptor(int sd, int degree, int* rows) {
    if (!rows) return fail(FX_EINVAL, "fx_dpc_descriptor: null result");
    if (sd != 2 && sd != 3) return fail(FX_EINVAL, "fx_dpc_descriptor: spatial dimension %d (quadrilaterals and hexahedra)", sd);
    if (degree < 1 || degree > 64) return fail(FX_EINVAL, "fx_dpc_descriptor: degree %d (1..64)", degree);
    const int ndof = fxk::dpc_fill(sd, degree, nullptr);
    std::vector<int> packed((size_t)ndof);
    fxk::dpc_fill(sd, degree, packed.data());
    for (int i = 0; i < ndof; ++i)
        for (int j = 0; j <= sd; ++j) rows[(size_t)i * (sd + 1) + j] = fxk::dpc_alpha(packed[i], j);
    return FX_OK;
}

int fx_dpc_kernel(int sd, int degree, int order, int npts, char* buf, int n) {
    if (!buf || n <= 0) return fail(FX_EINVAL, "fx_dpc_kernel: no buffer");
    DpcPlan p;
    const int rc = make_plan("fx_dpc_kernel", sd, degree, order, npts, &p);
    if (rc != FX_OK) return rc;
    snprintf(buf, (size_t)n, "fxk::dpc_kernel<%d,%d,%d> %s P=%d", sd, degree, order, p.image ? "image" : "stream", p.P);
    return FX_OK;
}

int fx_dpc_tabulate_batch(fx_ctx* ctx, int sd, int degree, const double* lam0, const double* G, int order, int64_t nreq,
                          int npts, const double* pts, double* out, void* stream) {
    const char* who = "fx_dpc_tabulate_batch";
    if (!ctx || !lam0 || !G) return fail(FX_EINVAL, "%s: null context or barycentric map", who);
    if (nreq < 0) return fail(FX_EINVAL, "%s: negative degree, order or count", who);
    DpcPlan p;
    const int rc = make_plan(who, sd, degree, order, npts, &p);
    if (rc != FX_OK) return rc;
    for (int i = 0; i < (sd + 1) * sd; ++i)
        if (!std::isfinite(G[i])) return fail(FX_EINVAL, "%s: the barycentric map is not finite", who);
    for (int i = 0; i <= sd; ++i)
        if (!std::isfinite(lam0[i])) return fail(FX_EINVAL, "%s: the barycentric map is not finite", who);
    if (nreq == 0 || npts == 0) return FX_OK;
    if (!pts || !out) return fail(FX_EINVAL, "%s: null device pointer", who);

    int device = 0, num_cu = 0, lds_per_cu = 0;
    fx::ctx_facts(ctx, &device, &num_cu, &lds_per_cu);
    if ((long long)p.lds > (long long)lds_per_cu) return fail(FX_ENOTIMPL, "%s: %zu bytes of LDS", who, p.lds);
    fxk::DpcArgs a;
    memset(&a, 0, sizeof a);
    a.pts = pts;
    a.out = out;
    for (int i = 0; i <= sd; ++i) a.lam0[i] = lam0[i];
    for (int i = 0; i < (sd + 1) * sd; ++i) a.G[i] = G[i];
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
