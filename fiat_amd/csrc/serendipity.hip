// Host side of the Serendipity kernels (serendipity.hpp): libfiat_amd_serendipity.so, a companion of libfiat_amd.so
// (include/fiat_amd_serendipity.h).  It links against the main library and uses its error slot and contexts.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/fiat_amd_serendipity.h"
#include "serendipity.hpp"
#include "host_common.hpp"

namespace {

// which instance and route a shape takes
struct SerPlan {
    bool generic;
    int P, image, ndof, ntab;
    long long reqsize;
    size_t lds;
};

int make_plan(const char* who, int sd, int degree, int order, int npts, SerPlan* p) {
    if (sd != 2 && sd != 3) return fail(FX_EINVAL, "%s: spatial dimension %d (quadrilaterals and hexahedra)", who, sd);
    if (degree < 1) return fail(FX_EINVAL, "%s: degree %d (>= 1)", who, degree);
    if (order < 0 || npts < 0) return fail(FX_EINVAL, "%s: negative order or count", who);
    if (degree > fxk::SER_GEN_MAXK) return fail(FX_ENOTIMPL, "%s: degree %d > %d", who, degree, fxk::SER_GEN_MAXK);
    if (order > fxk::SER_GEN_MAXORDER) return fail(FX_ENOTIMPL, "%s: derivative order %d > %d", who, order, fxk::SER_GEN_MAXORDER);
    p->ndof = fxk::ser_fill(sd, degree, nullptr);
    p->ntab = (int)(sd == 2 ? (order + 1) * (order + 2) / 2 : (order + 1) * (order + 2) * (order + 3) / 6);
    p->reqsize = (long long)p->ntab * p->ndof * npts;
    if (p->reqsize >= (1LL << 31)) return fail(FX_ENOTIMPL, "%s: request of %lld entries", who, p->reqsize);
    p->generic = degree > fxk::SER_SPEC_MAXK || order > fxk::SER_SPEC_MAXORDER;
    // (the generic instance streams: no image, its LDS holds the dof table and the lanes' 1-D tables)
    const ItemPlan ip = plan_items(npts, p->reqsize, p->generic ? 0 : fxk::SER_IMAGE_BYTES, true);
    p->P = ip.P;
    p->image = ip.image;
    p->lds = p->generic ? fxk::ser_generic_lds(sd, degree, order, p->ndof) : ip.image_bytes;
    return FX_OK;
}

hipError_t launch(bool generic, int sd, int degree, int order, unsigned grid, size_t lds, hipStream_t s, const fxk::SerArgs& a) {
    return dispatch_int<2, 3>(sd, [&](auto SD) {
        if (generic) return launch_wave64(fxk::serendipity_generic<SD()>, grid, lds, s, a);
        return dispatch_int<1, fxk::SER_SPEC_MAXK>(degree, [&](auto K) {
            return dispatch_int<0, fxk::SER_SPEC_MAXORDER>(order, [&](auto ORDER) {
                return launch_wave64(fxk::serendipity_kernel<SD(), K(), ORDER()>, grid, lds, s, a);
            });
        });
    });
}

}  // namespace

extern "C" {

int fx_serendipity_abi_version(void) { return 1; }

int fx_serendipity_dims(int sd, int degree, int* ndof) {
    if (!ndof) return fail(FX_EINVAL, "fx_serendipity_dims: null result");
    if (sd != 2 && sd != 3) return fail(FX_EINVAL, "fx_serendipity_dims: spatial dimension %d (quadrilaterals and hexahedra)", sd);
    if (degree < 1) return fail(FX_EINVAL, "fx_serendipity_dims: degree %d (>= 1)", degree);
    *ndof = fxk::ser_fill(sd, degree, nullptr);
    return FX_OK;
}

int fx_serendipity_descriptor(int sd, int degree, int* rows) {
    int ndof = 0;
    if (!rows) return fail(FX_EINVAL, "fx_serendipity_descriptor: null result");
    if (sd != 2 && sd != 3) return fail(FX_EINVAL, "fx_serendipity_descriptor: spatial dimension %d (quadrilaterals and hexahedra)", sd);
    if (degree < 1 || degree > 253) return fail(FX_EINVAL, "fx_serendipity_descriptor: degree %d (1..253)", degree);
    ndof = fxk::ser_fill(sd, degree, nullptr);
    std::vector<int> packed((size_t)ndof);
    fxk::ser_fill(sd, degree, packed.data());
    for (int i = 0; i < ndof; ++i) {
        rows[(size_t)i * (1 + sd)] = fxk::ser_minus(packed[i]) ? -1 : 1;
        for (int d = 0; d < sd; ++d) rows[(size_t)i * (1 + sd) + 1 + d] = fxk::ser_code(packed[i], d);
    }
    return FX_OK;
}

int fx_serendipity_kernel(int sd, int degree, int order, int npts, char* buf, int n) {
    if (!buf || n <= 0) return fail(FX_EINVAL, "fx_serendipity_kernel: no buffer");
    SerPlan p;
    const int rc = make_plan("fx_serendipity_kernel", sd, degree, order, npts, &p);
    if (rc != FX_OK) return rc;
    if (p.generic) snprintf(buf, (size_t)n, "fxk::serendipity_generic<%d> stream P=%d", sd, p.P);
    else snprintf(buf, (size_t)n, "fxk::serendipity_kernel<%d,%d,%d> %s P=%d", sd, degree, order, p.image ? "image" : "stream", p.P);
    return FX_OK;
}

int fx_serendipity_tabulate_batch(fx_ctx* ctx, int sd, int degree, const double* lo, const double* hi, int order,
                                  int64_t nreq, int npts, const double* pts, double* out, void* stream) {
    const char* who = "fx_serendipity_tabulate_batch";
    if (!ctx || !lo || !hi) return fail(FX_EINVAL, "%s: null context or box", who);
    if (nreq < 0) return fail(FX_EINVAL, "%s: negative order or count", who);
    SerPlan p;
    const int rc = make_plan(who, sd, degree, order, npts, &p);
    if (rc != FX_OK) return rc;
    for (int d = 0; d < sd; ++d)
        if (!(hi[d] != lo[d])) return fail(FX_EINVAL, "%s: empty box in direction %d", who, d);
    if (nreq == 0 || npts == 0) return FX_OK;
    if (!pts || !out) return fail(FX_EINVAL, "%s: null device pointer", who);

    int device = 0, num_cu = 0, lds_per_cu = 0;
    fx::ctx_facts(ctx, &device, &num_cu, &lds_per_cu);
    if ((long long)p.lds > (long long)lds_per_cu) return fail(FX_ENOTIMPL, "%s: %zu bytes of LDS", who, p.lds);
    fxk::SerArgs a;
    memset(&a, 0, sizeof a);
    a.pts = pts;
    a.out = out;
    for (int d = 0; d < 3; ++d) {
        a.v0[d] = d < sd ? lo[d] : 0.0;
        a.v1[d] = d < sd ? hi[d] : 1.0;
    }
    a.nreq = nreq;
    a.npts = npts;
    a.ndof = p.ndof;
    a.ntab = p.ntab;
    a.P = p.P;
    a.image = p.image;
    a.degree = degree;
    a.order = order;
    a.nitems = (nreq + p.P - 1) / p.P;
    FX_HIP_TRY(hipSetDevice(device));
    FX_HIP_TRY(launch(p.generic, sd, degree, order, item_grid(a.nitems, num_cu, 64), p.lds, (hipStream_t)stream, a));
    return FX_OK;
}

}  // extern "C"
