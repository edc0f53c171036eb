// Host side of the H(div) trace kernel (trace.hpp): libfiat_amd_trace.so, a companion of libfiat_amd.so
// (include/fiat_amd_trace.h).  It links against the main library and uses its error slot and contexts.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../include/fiat_amd_trace.h"
#include "trace.hpp"
#include "host_common.hpp"

namespace {

// which instance and route a shape takes
struct TracePlan {
    int K;  // template degree: -1 for the run-time-degree instance
    int P, image, nf;
    long long reqsize;
    size_t lds;
};

int make_plan(const char* who, int fd, int degree, int nfac, int npts, TracePlan* p) {
    if (fd < 0 || fd > 2) return fail(FX_EINVAL, "%s: facet dimension %d (0..2)", who, fd);
    if (degree < 0 || npts < 0) return fail(FX_EINVAL, "%s: negative degree or count", who);
    if (nfac < 1 || nfac > 4) return fail(FX_EINVAL, "%s: %d facets (1..4)", who, nfac);
    if (fd == 0 && degree > 0) return fail(FX_ENOTIMPL, "%s: degree %d on a point (0)", who, degree);
    if (degree > fxk::TRACE_MAXGEN) return fail(FX_ENOTIMPL, "%s: degree %d (0..%d)", who, degree, fxk::TRACE_MAXGEN);
    p->K = degree <= fxk::TRACE_MAXK ? degree : -1;
    p->nf = fxk::trace_nf(fd, degree);
    p->reqsize = (long long)nfac * p->nf * npts;
    if (p->reqsize >= (1LL << 31)) return fail(FX_ENOTIMPL, "%s: request of %lld entries", who, p->reqsize);
    const long long cbytes = p->K >= 0 ? (((long long)p->nf * p->nf + 1) & ~1LL) * 8 : 0;  // the LDS-resident matrix
    const ItemPlan ip = plan_items(npts, p->reqsize, fxk::TRACE_LDS_BYTES - cbytes, true);
    p->P = ip.P;
    p->image = ip.image;
    p->lds = (size_t)cbytes + ip.image_bytes;
    return FX_OK;
}

// the three-term coefficients of the run-time-degree instance, by value
fxk::TraceRec make_rec(int fd, int degree) {
    fxk::TraceRec rec;
    memset(&rec, 0, sizeof rec);
    for (int p = 0; p <= degree; ++p) {
        rec.a1[p] = fxk::trace_a1(p);
        rec.a2[p] = fxk::trace_a2(p);
    }
    if (fd == 2)
        for (int q = 1; q <= degree; ++q)
            for (int p = 0; p + q <= degree; ++p)
                for (int w = 0; w < 3; ++w) rec.b[(p + q) * (p + q + 1) / 2 + q][w] = fxk::trace_b(p, q, w);
    return rec;
}

template <int FD, int K> hipError_t launch_one(unsigned grid, size_t lds, hipStream_t s, const fxk::TraceArgs& a) {
    if constexpr (K < 0) return launch_wave64(fxk::trace_kernel<FD, K>, grid, lds, s, a, make_rec(FD, a.degree));
    else return launch_wave64(fxk::trace_kernel<FD, K>, grid, lds, s, a, fxk::TraceNoRec{});
}

hipError_t launch(int fd, int K, unsigned grid, size_t lds, hipStream_t s, const fxk::TraceArgs& a) {
    if (fd == 0) return launch_one<0, 0>(grid, lds, s, a);  // a point carries the constant
    return dispatch_int<1, 2>(fd, [&](auto FD) {
        if (K < 0) return launch_one<FD(), -1>(grid, lds, s, a);  // the run-time-degree instance
        return dispatch_int<0, fxk::TRACE_MAXK>(K, [&](auto KK) { return launch_one<FD(), KK()>(grid, lds, s, a); });
    });
}

}  // namespace

extern "C" {

int fx_trace_abi_version(void) { return 1; }

int fx_trace_kernel(int fd, int degree, int nfac, int npts, char* buf, int n) {
    if (!buf || n <= 0) return fail(FX_EINVAL, "fx_trace_kernel: no buffer");
    TracePlan p;
    const int rc = make_plan("fx_trace_kernel", fd, degree, nfac, npts, &p);
    if (rc != FX_OK) return rc;
    snprintf(buf, (size_t)n, "fxk::trace_kernel<%d,%d> %s P=%d", fd, p.K, p.image ? "image" : "stream", p.P);
    return FX_OK;
}

int fx_trace_tabulate_batch(fx_ctx* ctx, int fd, int degree, int nfac, int mode, int facet, const int* facets, const double* C,
                            const double* lam0, const double* G, int64_t nreq, int npts, const double* pts, double* out,
                            void* stream) {
    const char* who = "fx_trace_tabulate_batch";
    if (!ctx) return fail(FX_EINVAL, "%s: null context", who);
    if (nreq < 0) return fail(FX_EINVAL, "%s: negative degree or count", who);
    if (mode < FX_TRACE_IDENTIFY || mode > FX_TRACE_FACETS) return fail(FX_EINVAL, "%s: mode %d (0..2)", who, mode);
    TracePlan p;
    const int rc = make_plan(who, fd, degree, nfac, npts, &p);
    if (rc != FX_OK) return rc;
    const int sd = fd + 1;
    if (mode == FX_TRACE_IDENTIFY) {
        if (nfac != sd + 1) return fail(FX_EINVAL, "%s: facets are identified on simplices (%d facets, not %d)", who, sd + 1, nfac);
        if (!lam0 || !G) return fail(FX_EINVAL, "%s: null barycentric map", who);
        for (int i = 0; i < (sd + 1) * sd; ++i)
            if (!std::isfinite(G[i])) return fail(FX_EINVAL, "%s: the barycentric map is not finite", who);
        for (int i = 0; i <= sd; ++i)
            if (!std::isfinite(lam0[i])) return fail(FX_EINVAL, "%s: the barycentric map is not finite", who);
    }
    if (mode == FX_TRACE_ONE_FACET && (facet < 0 || facet >= nfac))
        return fail(FX_EINVAL, "%s: facet %d of %d", who, facet, nfac);
    if (nreq == 0 || npts == 0) return FX_OK;
    if (!out || !C || (!pts && (fd > 0 || mode == FX_TRACE_IDENTIFY))) return fail(FX_EINVAL, "%s: null device pointer", who);
    if (mode == FX_TRACE_FACETS && !facets) return fail(FX_EINVAL, "%s: null facet numbers", who);

    int device = 0, num_cu = 0, lds_per_cu = 0;
    fx::ctx_facts(ctx, &device, &num_cu, &lds_per_cu);
    if ((long long)p.lds > (long long)lds_per_cu) return fail(FX_ENOTIMPL, "%s: %zu bytes of LDS", who, p.lds);
    fxk::TraceArgs a;
    memset(&a, 0, sizeof a);
    a.pts = pts;
    a.facets = facets;
    a.C = C;
    a.out = out;
    if (mode == FX_TRACE_IDENTIFY) {
        for (int i = 0; i <= sd; ++i) a.lam0[i] = lam0[i];
        for (int i = 0; i < (sd + 1) * sd; ++i) a.G[i] = G[i];
    }
    a.nreq = nreq;
    a.npts = npts;
    a.P = p.P;
    a.image = p.image;
    a.mode = mode;
    a.facet = facet;
    a.nfac = nfac;
    a.degree = degree;
    a.swap = fd == 0;
    a.nitems = (nreq + p.P - 1) / p.P;
    FX_HIP_TRY(hipSetDevice(device));
    FX_HIP_TRY(launch(fd, p.K, item_grid(a.nitems, num_cu, 64), p.lds, (hipStream_t)stream, a));
    return FX_OK;
}

}  // extern "C"
