// Host side of the Serendipity kernels (serendipity.hpp): libfiat_amd_serendipity.so, a companion of libfiat_amd.so
// (include/fiat_amd_serendipity.h).  It links against the main library and uses its error slot and contexts.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/fiat_amd_serendipity.h"
#include "serendipity.hpp"

namespace fx {
int set_error(int code, const char* msg);  // api.hip (libfiat_amd.so)
void ctx_facts(const fx_ctx* ctx, int* device, int* num_cu, int* lds_per_cu);
}  // namespace fx

namespace {

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return fx::set_error(code, buf);
}

#define SER_HIP_TRY(expr)                                                         \
    do {                                                                          \
        hipError_t e_ = (expr);                                                   \
        if (e_ != hipSuccess) {                                                   \
            (void)hipGetLastError();                                              \
            return fail(FX_EHIP, "%s: %s", #expr, hipGetErrorString(e_));         \
        }                                                                         \
    } while (0)

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
    const int whole = npts > 0 && npts <= 64 ? 64 / npts : 1;  // whole requests per 64 lanes
    p->P = whole;
    p->image = 0;
    p->lds = 0;
    if (p->generic) {
        p->lds = fxk::ser_generic_lds(sd, degree, order, p->ndof);
    } else if (p->reqsize > 0 && p->reqsize * 8 <= fxk::SER_IMAGE_BYTES) {
        // the item shrinks to the requests whose tables fit the image
        p->image = 1;
        p->P = (int)std::min<long long>(whole, fxk::SER_IMAGE_BYTES / (p->reqsize * 8));
        p->lds = (size_t)(((long long)p->P * p->reqsize + 1) & ~1LL) * 8;
    }
    return FX_OK;
}

template <int SD, int K, int ORDER> hipError_t launch_one(dim3 grid, size_t lds, hipStream_t s, const fxk::SerArgs& a) {
    hipLaunchKernelGGL((fxk::serendipity_kernel<SD, K, ORDER>), grid, dim3(64), lds, s, a);
    return hipGetLastError();
}

template <int SD, int K> hipError_t launch_order(int order, dim3 grid, size_t lds, hipStream_t s, const fxk::SerArgs& a) {
    if (order == 0) return launch_one<SD, K, 0>(grid, lds, s, a);
    if (order == 1) return launch_one<SD, K, 1>(grid, lds, s, a);
    return launch_one<SD, K, 2>(grid, lds, s, a);
}

template <int SD> hipError_t launch_degree(int K, int order, dim3 grid, size_t lds, hipStream_t s, const fxk::SerArgs& a) {
    switch (K) {
        case 1: return launch_order<SD, 1>(order, grid, lds, s, a);
        case 2: return launch_order<SD, 2>(order, grid, lds, s, a);
        case 3: return launch_order<SD, 3>(order, grid, lds, s, a);
        case 4: return launch_order<SD, 4>(order, grid, lds, s, a);
        case 5: return launch_order<SD, 5>(order, grid, lds, s, a);
        default: return launch_order<SD, 6>(order, grid, lds, s, a);
    }
}

template <int SD> hipError_t launch_generic(dim3 grid, size_t lds, hipStream_t s, const fxk::SerArgs& a) {
    auto kern = fxk::serendipity_generic<SD>;
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, grid, dim3(64), lds, s, a);
    return hipGetLastError();
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
    const dim3 grid((unsigned)std::max<long long>(1, std::min<long long>(a.nitems, (long long)num_cu * 64)));
    SER_HIP_TRY(hipSetDevice(device));
    if (p.generic) SER_HIP_TRY(sd == 2 ? launch_generic<2>(grid, p.lds, (hipStream_t)stream, a) : launch_generic<3>(grid, p.lds, (hipStream_t)stream, a));
    else SER_HIP_TRY(sd == 2 ? launch_degree<2>(degree, order, grid, p.lds, (hipStream_t)stream, a) : launch_degree<3>(degree, order, grid, p.lds, (hipStream_t)stream, a));
    return FX_OK;
}

}  // extern "C"
