// Host side of the term-table kernel (sforms.hpp): libfiat_amd_sforms.so, a companion of libfiat_amd.so
// (include/fiat_amd_sforms.h).  It links against the main library and uses its error slot and contexts.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/fiat_amd_sforms.h"
#include "sforms.hpp"
#include "host_common.hpp"
#include <memory>

struct fx_sforms_element {
    int device, sd, degree, nrows;
    DeviceBuffer<double> coef;  // [nrows * sd]
    DeviceBuffer<int> codes;    // [nrows * sd]
};

namespace {

// which route a shape takes
struct SfPlan {
    int P, image, ntab, budget;
    long long reqsize;
    size_t lds;
};

int check_shape(const char* who, int sd, int degree, int nrows) {
    if (sd != 2 && sd != 3) return fail(FX_EINVAL, "%s: spatial dimension %d (quadrilaterals and hexahedra)", who, sd);
    if (degree < 1) return fail(FX_EINVAL, "%s: degree %d (>= 1)", who, degree);
    if (degree > fxk::SF_MAXK) return fail(FX_ENOTIMPL, "%s: degree %d > %d", who, degree, fxk::SF_MAXK);
    if (nrows < 1) return fail(FX_EINVAL, "%s: %d rows", who, nrows);
    return FX_OK;
}

int make_plan(const char* who, int sd, int degree, int nrows, int order, int npts, SfPlan* p) {
    const int rc = check_shape(who, sd, degree, nrows);
    if (rc != FX_OK) return rc;
    if (order < 0 || npts < 0) return fail(FX_EINVAL, "%s: negative order or count", who);
    if (order > fxk::SF_MAXORDER) return fail(FX_ENOTIMPL, "%s: derivative order %d > %d", who, order, fxk::SF_MAXORDER);
    p->ntab = (int)(sd == 2 ? (order + 1) * (order + 2) / 2 : (order + 1) * (order + 2) * (order + 3) / 6);
    p->reqsize = (long long)p->ntab * nrows * sd * npts;
    if (p->reqsize >= (1LL << 31)) return fail(FX_ENOTIMPL, "%s: request of %lld entries", who, p->reqsize);
    p->budget = fxk::sf_image_budget(sd, degree, order);
    const ItemPlan ip = plan_items(npts, p->reqsize, p->budget, true);
    p->P = ip.P;
    p->image = ip.image;
    p->lds = fxk::sf_tables_bytes(sd, degree, order) + ip.image_bytes;  // the 1-D tables, then the image
    return FX_OK;
}

hipError_t launch(int sd, int order, unsigned grid, size_t lds, hipStream_t s, const fxk::SfArgs& a) {
    return dispatch_int<2, 3>(sd, [&](auto SD) {
        return dispatch_int<0, fxk::SF_MAXORDER>(order, [&](auto ORDER) {
            return launch_wave64(fxk::sforms_kernel<SD(), ORDER()>, grid, lds, s, a);
        });
    });
}

}  // namespace

extern "C" {

int fx_sforms_abi_version(void) { return 1; }

int fx_sforms_element_create(fx_ctx* ctx, int sd, int degree, int nrows, const double* coef, const int* codes,
                             fx_sforms_element** out) {
    const char* who = "fx_sforms_element_create";
    if (!ctx || !coef || !codes || !out) return fail(FX_EINVAL, "%s: null argument", who);
    const int rc = check_shape(who, sd, degree, nrows);
    if (rc != FX_OK) return rc;
    if ((long long)nrows * sd >= (1LL << 24)) return fail(FX_ENOTIMPL, "%s: %d rows", who, nrows);
    const int nf = fxk::sf_ncodes(degree);
    const size_t n = (size_t)nrows * sd;
    const size_t npad = (n + fxk::SF_CHUNK - 1) / fxk::SF_CHUNK * fxk::SF_CHUNK;  // the kernel fetches whole chunks
    std::vector<int> packed(npad, 0);
    std::vector<double> padded(npad, 0.0);
    std::copy(coef, coef + n, padded.begin());
    for (size_t e = 0; e < n; ++e) {
        if (!(coef[e] == coef[e]) || coef[e] - coef[e] != 0.0) return fail(FX_EINVAL, "%s: entry %zu: coefficient not finite", who, e);
        if (coef[e] == 0.0) continue;
        int c[3] = {0, 0, 0};
        for (int d = 0; d < sd; ++d) {
            c[d] = codes[e * sd + d];
            if (c[d] < 0 || c[d] >= nf) return fail(FX_EINVAL, "%s: entry %zu: code %d outside the 1-D family (0..%d)", who, e, c[d], nf - 1);
        }
        packed[e] = fxk::sf_pack(c[0], c[1], c[2]);
    }
    int device = 0, num_cu = 0, lds_per_cu = 0;
    fx::ctx_facts(ctx, &device, &num_cu, &lds_per_cu);
    FX_HIP_TRY(hipSetDevice(device));
    std::unique_ptr<fx_sforms_element> el(new fx_sforms_element{device, sd, degree, nrows, {}, {}});
    hipError_t e = el->coef.upload(padded.data(), npad);
    if (e == hipSuccess) e = el->codes.upload(packed.data(), npad);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? FX_ENOMEM : FX_EHIP, "%s: %s", who, hipGetErrorString(e));
    *out = el.release();
    return FX_OK;
}

int fx_sforms_element_destroy(fx_sforms_element* el) {
    delete el;
    return FX_OK;
}

int fx_sforms_kernel(int sd, int degree, int nrows, int order, int npts, char* buf, int n) {
    if (!buf || n <= 0) return fail(FX_EINVAL, "fx_sforms_kernel: no buffer");
    SfPlan p;
    const int rc = make_plan("fx_sforms_kernel", sd, degree, nrows, order, npts, &p);
    if (rc != FX_OK) return rc;
    snprintf(buf, (size_t)n, "fxk::sforms_kernel<%d,%d> %s P=%d budget=%d", sd, order, p.image ? "image" : "stream", p.P, p.budget);
    return FX_OK;
}

int fx_sforms_tabulate_batch(fx_ctx* ctx, const fx_sforms_element* el, const double* lo, const double* hi, int order,
                             int64_t nreq, int npts, const double* pts, double* out, void* stream) {
    const char* who = "fx_sforms_tabulate_batch";
    if (!ctx || !el || !lo || !hi) return fail(FX_EINVAL, "%s: null context, element or box", who);
    if (nreq < 0) return fail(FX_EINVAL, "%s: negative order or count", who);
    SfPlan p;
    const int rc = make_plan(who, el->sd, el->degree, el->nrows, order, npts, &p);
    if (rc != FX_OK) return rc;
    for (int d = 0; d < el->sd; ++d)
        if (!(hi[d] != lo[d])) return fail(FX_EINVAL, "%s: empty box in direction %d", who, d);
    if (nreq == 0 || npts == 0) return FX_OK;
    if (!pts || !out) return fail(FX_EINVAL, "%s: null device pointer", who);

    int device = 0, num_cu = 0, lds_per_cu = 0;
    fx::ctx_facts(ctx, &device, &num_cu, &lds_per_cu);
    if (device != el->device) return fail(FX_EINVAL, "%s: the element lives on device %d, the context on %d", who, el->device, device);
    if ((long long)p.lds > (long long)lds_per_cu) return fail(FX_ENOTIMPL, "%s: %zu bytes of LDS", who, p.lds);
    fxk::SfArgs a;
    memset(&a, 0, sizeof a);
    a.pts = pts;
    a.out = out;
    a.coef = el->coef.get();
    a.codes = el->codes.get();
    for (int d = 0; d < 3; ++d) {
        a.v0[d] = d < el->sd ? lo[d] : 0.0;
        a.v1[d] = d < el->sd ? hi[d] : 1.0;
    }
    a.nreq = nreq;
    a.npts = npts;
    a.nrows = el->nrows;
    a.ntab = p.ntab;
    a.P = p.P;
    a.image = p.image;
    a.degree = el->degree;
    a.nitems = (nreq + p.P - 1) / p.P;
    FX_HIP_TRY(hipSetDevice(device));
    FX_HIP_TRY(launch(el->sd, order, item_grid(a.nitems, num_cu, 64), p.lds, (hipStream_t)stream, a));
    return FX_OK;
}

}  // extern "C"
