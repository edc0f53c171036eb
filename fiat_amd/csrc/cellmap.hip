// Host side of the Q1 cell-map kernels (cellmap.hpp): libfiat_amd_cellmap.so, a companion of libfiat_amd.so
// (include/fiat_amd_cellmap.h).  It links against the main library and uses its error slot and contexts.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "../../include/fiat_amd_cellmap.h"
#include "cellmap.hpp"
#include "host_common.hpp"

namespace {

const char* const MAP_NAMES[3] = {"affine", "covariant", "contravariant"};

int check_box(const char* who, int sd, const double* lo, const double* hi) {
    if (!lo || !hi) return fail(FX_EINVAL, "%s: null box", who);
    for (int d = 0; d < sd; ++d)
        if (!std::isfinite(lo[d]) || !std::isfinite(hi[d]) || !(hi[d] > lo[d]))
            return fail(FX_EINVAL, "%s: the box needs finite lo < hi in every direction", who);
    return FX_OK;
}

// ---- the general pass ----------------------------------------------------------------------------------------------------
struct ApplyPlan {
    int P, ntab;
    long long reqsize;
};

int plan_apply(const char* who, int sd, int mapping, int order, int npts, int nrows, int vdim, ApplyPlan* p) {
    if (sd != 2 && sd != 3) return fail(FX_EINVAL, "%s: spatial dimension %d (quadrilaterals and hexahedra)", who, sd);
    if (order < 0 || npts < 0 || nrows < 0) return fail(FX_EINVAL, "%s: negative order or count", who);
    if (mapping < 0) return fail(FX_EINVAL, "%s: mapping %d", who, mapping);
    if (mapping > FX_MAP_CONTRAVARIANT_PIOLA) return fail(FX_ENOTIMPL, "%s: mapping %d (affine and the single Piola maps)", who, mapping);
    if (order > fxk::CM_MAXORDER)
        return fail(FX_ENOTIMPL, "%s: derivative order %d > %d (needs more derivatives of the cell map)", who, order, fxk::CM_MAXORDER);
    if (vdim != 1 && vdim != sd) return fail(FX_EINVAL, "%s: %d components (1 or %d)", who, vdim, sd);
    if (mapping != FX_MAP_AFFINE && vdim != sd) return fail(FX_EINVAL, "%s: a Piola map needs %d components", who, sd);
    p->ntab = 1 + sd * order;
    p->reqsize = (long long)p->ntab * nrows * vdim * npts;
    if (p->reqsize >= (1LL << 31)) return fail(FX_EINVAL, "%s: request of %lld entries", who, p->reqsize);
    p->P = plan_items(npts, 0, 0, false).P;
    return FX_OK;
}

hipError_t launch_apply(int sd, int order, int mapping, unsigned grid, hipStream_t s, const fxk::CmApplyArgs& a) {
    return dispatch_int<2, 3>(sd, [&](auto SD) {
        return dispatch_int<0, fxk::CM_MAXORDER>(order, [&](auto ORDER) {
            return dispatch_int<0, 2>(mapping, [&](auto MAP) {
                return launch_wave64(fxk::cellmap_apply_kernel<SD(), ORDER(), MAP()>, grid, 0, s, a);
            });
        });
    });
}

// ---- the fused kernel ----------------------------------------------------------------------------------------------------
struct TensorPlan {
    int P, image, ndof, ntab;
    long long reqsize;
    size_t lds;
};

int plan_tensor(const char* who, int sd, int nn, int order, long long npts, TensorPlan* p) {
    if (sd != 2 && sd != 3) return fail(FX_EINVAL, "%s: spatial dimension %d (quadrilaterals and hexahedra)", who, sd);
    if (order < 0 || npts < 0 || nn < 1) return fail(FX_EINVAL, "%s: negative order or count", who);
    if (nn < fxk::CM_MINNN || nn > fxk::CM_MAXNN)
        return fail(FX_ENOTIMPL, "%s: factors of %d nodes (%d..%d)", who, nn, fxk::CM_MINNN, fxk::CM_MAXNN);
    if (order > fxk::CM_MAXORDER)
        return fail(FX_ENOTIMPL, "%s: derivative order %d > %d (needs more derivatives of the cell map)", who, order, fxk::CM_MAXORDER);
    p->ndof = sd == 2 ? nn * nn : nn * nn * nn;
    p->ntab = 1 + sd * order;
    p->reqsize = (long long)p->ntab * p->ndof * npts;
    if (npts >= (1LL << 31) || p->reqsize >= (1LL << 31)) return fail(FX_EINVAL, "%s: request of %lld entries", who, p->reqsize);
    const ItemPlan ip = plan_items((int)npts, p->reqsize, fxk::CM_IMAGE_BYTES, true);
    p->P = ip.P;
    p->image = ip.image;
    p->lds = ip.image_bytes;
    return FX_OK;
}

// q^sd points of a tensor grid; false where that is 2^31 or more (checked factor by factor: the product never overflows)
bool grid_points(int sd, int q, long long* npts) {
    long long n = 1;
    for (int f = 0; f < (sd == 3 ? 3 : 2); ++f) {
        if (q > 0 && n > ((1LL << 31) - 1) / q) return false;
        n *= q;
    }
    *npts = n;
    return true;
}

// Node data of the factors on the device, [sd][CM_LINE] (cellmap.hpp CmTensorArgs::lines): weights and differentiation matrix
// as make_dmat builds them (FIAT/barycentric_interpolation.py:50-59).  One buffer per (device, node arrays), made at the first
// call that names them (hipMalloc and a synchronous copy: not inside a stream capture) and kept: a launch in flight may still
// read it.  The cache holds at most CM_MAX_LINE_SETS sets; a new set beyond that waits for the devices to go idle, frees every
// buffer and starts the cache again, so a caller that keeps changing its nodes holds a bounded amount of device memory.
constexpr size_t CM_MAX_LINE_SETS = 64;
struct LinesKey {
    int device, sd, nn;
    std::vector<double> nodes;
    bool operator<(const LinesKey& o) const {
        if (device != o.device) return device < o.device;
        if (sd != o.sd) return sd < o.sd;
        if (nn != o.nn) return nn < o.nn;
        return nodes < o.nodes;
    }
};
std::mutex g_lines_mutex;
// (never destroyed: the buffers stay, as they always have, until the process ends -- freeing them from a static destructor would
// call into a runtime that may be gone)
std::map<LinesKey, DeviceBuffer<double>>& g_lines = *new std::map<LinesKey, DeviceBuffer<double>>;

int device_lines(const char* who, int device, int sd, int nn, const double* nodes, const double** out) {
    LinesKey key{device, sd, nn, std::vector<double>(nodes, nodes + (size_t)sd * nn)};
    std::lock_guard<std::mutex> lock(g_lines_mutex);
    auto it = g_lines.find(key);
    if (it != g_lines.end()) {
        *out = it->second.get();
        return FX_OK;
    }
    if (g_lines.size() >= CM_MAX_LINE_SETS) {
        for (auto& kv : g_lines) {  // (no launch may still read a buffer that is freed)
            FX_HIP_TRY(hipSetDevice(kv.first.device));
            FX_HIP_TRY(hipDeviceSynchronize());
        }
        for (auto& kv : g_lines) {
            FX_HIP_TRY(hipSetDevice(kv.first.device));
            FX_HIP_TRY(kv.second.reset());
        }
        g_lines.clear();
    }
    std::vector<double> buf((size_t)sd * fxk::CM_LINE, 0.0);
    for (int f = 0; f < sd; ++f) {
        const double* x = nodes + (size_t)f * nn;
        double* xs = buf.data() + (size_t)f * fxk::CM_LINE;
        double* w = xs + nn;
        double* D = xs + 2 * nn;
        for (int j = 0; j < nn; ++j) {
            xs[j] = x[j];
            double p = 1.0;
            for (int i = 0; i < nn; ++i)
                if (i != j) p *= x[j] - x[i];
            w[j] = 1.0 / p;
        }
        // D[i][j] = phi_i'(x_j) = (w_i / w_j) / (x_j - x_i); columns sum to zero (the basis sums to one)
        for (int i = 0; i < nn; ++i)
            for (int j = 0; j < nn; ++j)
                if (j != i) D[i * nn + j] = (w[i] / w[j]) / (x[j] - x[i]);
        for (int j = 0; j < nn; ++j) {
            double s = 0.0;
            for (int i = 0; i < nn; ++i)
                if (i != j) s += D[i * nn + j];
            D[j * nn + j] = -s;
        }
    }
    DeviceBuffer<double> d;
    FX_HIP_TRY(hipSetDevice(device));
    const hipError_t e = d.upload(buf.data(), buf.size());
    if (e != hipSuccess) return fail(FX_EHIP, "%s: %s", who, hipGetErrorString(e));
    *out = d.get();
    g_lines.emplace(std::move(key), std::move(d));
    return FX_OK;
}

hipError_t launch_tensor(int sd, int nn, int order, bool grid_in, unsigned grid, size_t lds, hipStream_t s, const fxk::CmTensorArgs& a) {
    return dispatch_int<2, 3>(sd, [&](auto SD) {
        return dispatch_int<fxk::CM_MINNN, fxk::CM_MAXNN>(nn, [&](auto NN) {
            return dispatch_int<0, fxk::CM_MAXORDER>(order, [&](auto ORDER) {
                if (grid_in) return launch_wave64(fxk::cellmap_tensor_kernel<SD(), NN(), ORDER(), true>, grid, lds, s, a);
                return launch_wave64(fxk::cellmap_tensor_kernel<SD(), NN(), ORDER(), false>, grid, lds, s, a);
            });
        });
    });
}

int tensor_launch(const char* who, fx_ctx* ctx, int sd, int nn, const double* nodes, const double* lo, const double* hi, int order,
                  int64_t nreq, long long npts, int q, bool grid_in, const double* pts, const double* corners, double* out,
                  void* stream) {
    if (!ctx || !nodes) return fail(FX_EINVAL, "%s: null context or nodes", who);
    if (nreq < 0) return fail(FX_EINVAL, "%s: negative order or count", who);
    TensorPlan p;
    int rc = plan_tensor(who, sd, nn, order, npts, &p);
    if (rc != FX_OK) return rc;
    rc = check_box(who, sd, lo, hi);
    if (rc != FX_OK) return rc;
    for (int f = 0; f < sd; ++f)
        for (int i = 0; i < nn; ++i) {
            if (!std::isfinite(nodes[f * nn + i])) return fail(FX_EINVAL, "%s: the nodes are not finite", who);
            for (int j = 0; j < i; ++j)
                if (nodes[f * nn + i] == nodes[f * nn + j]) return fail(FX_EINVAL, "%s: repeated interpolation node", who);
        }
    if (nreq == 0 || npts == 0) return FX_OK;
    if (!pts || !corners || !out) return fail(FX_EINVAL, "%s: null device pointer", who);
    int device = 0, num_cu = 0, lds_per_cu = 0;
    fx::ctx_facts(ctx, &device, &num_cu, &lds_per_cu);
    if ((long long)p.lds > (long long)lds_per_cu) return fail(FX_ENOTIMPL, "%s: %zu bytes of LDS", who, p.lds);
    fxk::CmTensorArgs a;
    memset(&a, 0, sizeof a);
    rc = device_lines(who, device, sd, nn, nodes, &a.lines);
    if (rc != FX_OK) return rc;
    a.pts = pts;
    a.corners = corners;
    a.out = out;
    for (int d = 0; d < sd; ++d) {
        a.lo[d] = lo[d];
        a.h[d] = hi[d] - lo[d];
    }
    a.nreq = nreq;
    a.npts = (int)npts;
    a.q = q;
    a.P = p.P;
    a.image = p.image;
    a.nitems = (nreq + p.P - 1) / p.P;
    FX_HIP_TRY(hipSetDevice(device));
    FX_HIP_TRY(launch_tensor(sd, nn, order, grid_in, item_grid(a.nitems, num_cu, 64), p.lds, (hipStream_t)stream, a));
    return FX_OK;
}

}  // namespace

extern "C" {

int fx_cellmap_abi_version(void) { return 1; }

int fx_cellmap_kernel(int sd, int nn, int mapping, int order, int nrows, int vdim, int npts, int grid, char* buf, int n) {
    const char* who = "fx_cellmap_kernel";
    if (!buf || n <= 0) return fail(FX_EINVAL, "%s: no buffer", who);
    if (nn == 0) {
        ApplyPlan p;
        const int rc = plan_apply(who, sd, mapping, order, npts, nrows, vdim, &p);
        if (rc != FX_OK) return rc;
        snprintf(buf, (size_t)n, "fxk::cellmap_apply_kernel<%d,%d,%d> %s P=%d", sd, order, mapping, MAP_NAMES[mapping], p.P);
        return FX_OK;
    }
    if (mapping != FX_MAP_AFFINE || vdim != 1) return fail(FX_EINVAL, "%s: the fused kernel serves scalar products", who);
    long long np = npts;
    if (grid) {
        if (npts < 0) return fail(FX_EINVAL, "%s: negative order or count", who);
        if (!grid_points(sd, npts, &np)) return fail(FX_EINVAL, "%s: a grid of %d points per direction has 2^31 points or more", who, npts);
    }
    TensorPlan p;
    const int rc = plan_tensor(who, sd, nn, order, np, &p);
    if (rc != FX_OK) return rc;
    snprintf(buf, (size_t)n, "fxk::cellmap_tensor_kernel<%d,%d,%d,%s> %s P=%d", sd, nn, order, grid ? "true" : "false",
             p.image ? "image" : "stream", p.P);
    return FX_OK;
}

int fx_cellmap_geometry(fx_ctx* ctx, int sd, const double* lo, const double* hi, int64_t nreq, int npts, const double* pts,
                        const double* corners, double* x, double* J, double* detJ, void* stream) {
    const char* who = "fx_cellmap_geometry";
    if (!ctx) return fail(FX_EINVAL, "%s: null context", who);
    if (sd != 2 && sd != 3) return fail(FX_EINVAL, "%s: spatial dimension %d (quadrilaterals and hexahedra)", who, sd);
    if (nreq < 0 || npts < 0) return fail(FX_EINVAL, "%s: negative count", who);
    const int rc = check_box(who, sd, lo, hi);
    if (rc != FX_OK) return rc;
    if (nreq == 0 || npts == 0) return FX_OK;
    if (!pts || !corners || !x || !J || !detJ) return fail(FX_EINVAL, "%s: null device pointer", who);
    int device = 0, num_cu = 0, lds_per_cu = 0;
    fx::ctx_facts(ctx, &device, &num_cu, &lds_per_cu);
    fxk::CmGeomArgs a;
    memset(&a, 0, sizeof a);
    a.pts = pts;
    a.corners = corners;
    a.x = x;
    a.J = J;
    a.det = detJ;
    for (int d = 0; d < sd; ++d) {
        a.lo[d] = lo[d];
        a.h[d] = hi[d] - lo[d];
    }
    a.total = (long long)nreq * npts;
    a.npts = npts;
    const unsigned grid = item_grid((a.total + 63) / 64, num_cu, 64);
    FX_HIP_TRY(hipSetDevice(device));
    const auto launch = [&](auto SD) { return launch_wave64(fxk::cellmap_geometry_kernel<SD()>, grid, 0, (hipStream_t)stream, a); };
    FX_HIP_TRY((dispatch_int<2, 3>(sd, launch)));
    return FX_OK;
}

int fx_cellmap_apply(fx_ctx* ctx, int sd, int mapping, int order, int64_t nreq, int npts, int nrows, int vdim, const double* lo,
                     const double* hi, const double* pts, const double* corners, const double* in, double* out, void* stream) {
    const char* who = "fx_cellmap_apply";
    if (!ctx) return fail(FX_EINVAL, "%s: null context", who);
    if (nreq < 0) return fail(FX_EINVAL, "%s: negative order or count", who);
    ApplyPlan p;
    int rc = plan_apply(who, sd, mapping, order, npts, nrows, vdim, &p);
    if (rc != FX_OK) return rc;
    rc = check_box(who, sd, lo, hi);
    if (rc != FX_OK) return rc;
    if (nreq == 0 || npts == 0 || nrows == 0) return FX_OK;
    if (!pts || !corners || !in || !out) return fail(FX_EINVAL, "%s: null device pointer", who);
    if (in == out && order == 0 && mapping == FX_MAP_AFFINE) return FX_OK;  // values of a scalar: nothing changes
    int device = 0, num_cu = 0, lds_per_cu = 0;
    fx::ctx_facts(ctx, &device, &num_cu, &lds_per_cu);
    fxk::CmApplyArgs a;
    memset(&a, 0, sizeof a);
    a.pts = pts;
    a.corners = corners;
    a.in = in;
    a.out = out;
    for (int d = 0; d < sd; ++d) {
        a.lo[d] = lo[d];
        a.h[d] = hi[d] - lo[d];
    }
    a.nreq = nreq;
    a.npts = npts;
    a.nrows = nrows;
    a.vdim = vdim;
    a.P = p.P;
    a.nitems = (nreq + p.P - 1) / p.P;
    FX_HIP_TRY(hipSetDevice(device));
    FX_HIP_TRY(launch_apply(sd, order, mapping, item_grid(a.nitems, num_cu, 64), (hipStream_t)stream, a));
    return FX_OK;
}

int fx_cellmap_tensor_batch(fx_ctx* ctx, int sd, int nn, const double* nodes, const double* lo, const double* hi, int order,
                            int64_t nreq, int npts, const double* pts, const double* corners, double* out, void* stream) {
    return tensor_launch("fx_cellmap_tensor_batch", ctx, sd, nn, nodes, lo, hi, order, nreq, npts, 0, false, pts, corners, out, stream);
}

int fx_cellmap_tensor_grid_batch(fx_ctx* ctx, int sd, int nn, const double* nodes, const double* lo, const double* hi, int order,
                                 int64_t nreq, int q, const double* grid, const double* corners, double* out, void* stream) {
    if (q < 0) return fail(FX_EINVAL, "fx_cellmap_tensor_grid_batch: negative grid size");
    long long npts = 0;
    if (!grid_points(sd, q, &npts))
        return fail(FX_EINVAL, "fx_cellmap_tensor_grid_batch: a grid of %d points per direction has 2^31 points or more", q);
    return tensor_launch("fx_cellmap_tensor_grid_batch", ctx, sd, nn, nodes, lo, hi, order, nreq, npts, q, true, grid, corners, out,
                         stream);
}

}  // extern "C"
