// Host side of the Bernstein kernels (bernstein.hpp): fx_bernstein_tabulate_batch / _shared.  Its own translation unit,
// compiled beside api.hip and wg.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>

#include "../../include/fiat_amd.h"
#include "bernstein.hpp"
#include "host_common.hpp"

namespace {

constexpr int BERN_MAX_ORDER = 8;        // on the element's own cell
constexpr int BERN_MAX_ORDER_CELLS = 4;  // with per-request cells (the chain-rule coefficients of every request in LDS)

// E = inverse of [v1-v0 | ... | vsd-v0] (host form of bern_cell), v0, G = d lambda / dx [(sd+1)][sd]
bool host_bary(int sd, const double* v, double* E, double* v0, double* G) {
    double e[3][3];
    for (int r = 0; r < sd; ++r) {
        v0[r] = v[r];
        for (int c = 0; c < sd; ++c) e[r][c] = v[(c + 1) * sd + r] - v[r];
    }
    double det;
    if (sd == 1) {
        det = e[0][0];
        if (det == 0.0) return false;
        E[0] = 1.0 / det;
    } else if (sd == 2) {
        det = e[0][0] * e[1][1] - e[0][1] * e[1][0];
        if (det == 0.0) return false;
        const double inv = 1.0 / det;
        E[0] = e[1][1] * inv;
        E[1] = -e[0][1] * inv;
        E[2] = -e[1][0] * inv;
        E[3] = e[0][0] * inv;
    } else {
        const double c00 = e[1][1] * e[2][2] - e[1][2] * e[2][1];
        const double c01 = e[1][2] * e[2][0] - e[1][0] * e[2][2];
        const double c02 = e[1][0] * e[2][1] - e[1][1] * e[2][0];
        det = e[0][0] * c00 + e[0][1] * c01 + e[0][2] * c02;
        if (det == 0.0) return false;
        const double inv = 1.0 / det;
        E[0] = c00 * inv;
        E[1] = (e[0][2] * e[2][1] - e[0][1] * e[2][2]) * inv;
        E[2] = (e[0][1] * e[1][2] - e[0][2] * e[1][1]) * inv;
        E[3] = c01 * inv;
        E[4] = (e[0][0] * e[2][2] - e[0][2] * e[2][0]) * inv;
        E[5] = (e[0][2] * e[1][0] - e[0][0] * e[1][2]) * inv;
        E[6] = c02 * inv;
        E[7] = (e[0][1] * e[2][0] - e[0][0] * e[2][1]) * inv;
        E[8] = (e[0][0] * e[1][1] - e[0][1] * e[1][0]) * inv;
    }
    for (int d = 0; d < sd; ++d) {
        double s = 0.0;
        for (int i = 0; i < sd; ++i) {
            G[(i + 1) * sd + d] = E[i * sd + d];
            s += E[i * sd + d];
        }
        G[d] = -s;
    }
    return true;
}

hipError_t launch(bool spec, int sd, int n, int order, unsigned grid, size_t lds, hipStream_t s, const fxk::BernArgs& a) {
    return dispatch_int<1, 3>(sd, [&](auto SD) {
        if (!spec) return launch_wave64(fxk::tabulate_bernstein_generic<SD()>, grid, lds, s, a);
        return dispatch_int<0, fxk::BERN_SPEC_MAXN>(n, [&](auto N) {
            return dispatch_int<0, 2>(order, [&](auto ORDER) {
                return launch_wave64(fxk::tabulate_bernstein<SD(), N(), ORDER()>, grid, lds, s, a);
            });
        });
    });
}

int bernstein_launch(const char* who, fx_ctx* ctx, int sd, int n, const double* cell, int order, int64_t nreq, int npts,
                     const double* pts, const double* verts, double* out, void* stream, bool shared) {
    if (!ctx) return fail(FX_EINVAL, "%s: null context", who);
    if (sd < 1 || sd > 3) return fail(FX_EINVAL, "%s: spatial dimension %d (simplices of dimension 1..3)", who, sd);
    if (n < 0 || order < 0 || nreq < 0 || npts < 0) return fail(FX_EINVAL, "%s: negative degree, order or count", who);
    if (n > fxk::BERN_MAXN) return fail(FX_ENOTIMPL, "%s: degree %d > %d", who, n, fxk::BERN_MAXN);
    const bool cells = verts != nullptr;
    if (shared && !cells) return fail(FX_EINVAL, "%s: the shared route needs the cells (verts)", who);
    const int maxo = cells ? BERN_MAX_ORDER_CELLS : BERN_MAX_ORDER;
    if (order > maxo)
        return fail(FX_ENOTIMPL, "%s: derivative order %d > %d%s", who, order, maxo, cells ? " with per-request cells" : "");
    if (!cell) return fail(FX_EINVAL, "%s: null cell", who);
    fxk::BernArgs a;
    memset(&a, 0, sizeof a);
    if (!host_bary(sd, cell, a.E, a.v0, a.G)) return fail(FX_EINVAL, "%s: degenerate cell", who);
    if (nreq == 0 || npts == 0) return FX_OK;
    if (!pts || !out) return fail(FX_EINVAL, "%s: null device pointer", who);

    int device = 0, num_cu = 0, lds_per_cu = 0;
    fx::ctx_facts(ctx, &device, &num_cu, &lds_per_cu);
    const int ntab = fxk::bern_binom(sd + order, sd), ndof = fxk::bern_binom(n + sd, sd);
    const long long reqsize = (long long)ntab * ndof * npts;
    a.pts = pts;
    a.verts = verts;
    a.out = out;
    a.nreq = nreq;
    a.npts = npts;
    a.n = n;
    a.order = order;
    a.ntab = ntab;
    a.ndof = ndof;
    a.shared = shared ? 1 : 0;
    const bool spec = n <= fxk::BERN_SPEC_MAXN && order <= 2;
    const ItemPlan ip = plan_items(npts, reqsize, fxk::BERN_IMAGE_BYTES, false);  // (the generic instance takes its P only)
    int P = ip.P, per_cu = 64;
    size_t lds;
    if (spec) {
        a.image = ip.image;
        lds = ip.image_bytes;
        a.stage_doubles = (int)(lds / 8);
    } else {
        const int csize = fxk::bern_coef_size(sd, order);
        if (cells) {  // one coefficient block per request of the item
            P = std::max(1, std::min(P, fxk::BERN_IMAGE_BYTES / (csize * 8)));
            a.stage_doubles = P * csize;
        } else {
            a.stage_doubles = csize;
        }
        lds = (size_t)a.stage_doubles * 8;
        if ((long long)lds > lds_per_cu) return fail(FX_ENOTIMPL, "%s: %zu B of chain-rule coefficients exceed the LDS", who, lds);
        per_cu = 8;
    }
    a.P = P;
    a.nitems = (nreq + P - 1) / P;
    FX_HIP_TRY(hipSetDevice(device));
    FX_HIP_TRY(launch(spec, sd, n, order, item_grid(a.nitems, num_cu, per_cu), lds, (hipStream_t)stream, a));
    return FX_OK;
}

}  // namespace

extern "C" {

int fx_bernstein_tabulate_batch(fx_ctx* ctx, int sd, int n, const double* cell, int order, int64_t nreq, int npts,
                                const double* pts, const double* verts, double* out, void* stream) {
    return bernstein_launch("fx_bernstein_tabulate_batch", ctx, sd, n, cell, order, nreq, npts, pts, verts, out, stream, false);
}

int fx_bernstein_tabulate_shared(fx_ctx* ctx, int sd, int n, const double* cell, int order, int64_t nreq, int npts,
                                 const double* ref_pts, const double* verts, double* out, void* stream) {
    return bernstein_launch("fx_bernstein_tabulate_shared", ctx, sd, n, cell, order, nreq, npts, ref_pts, verts, out, stream, true);
}

}  // extern "C"
