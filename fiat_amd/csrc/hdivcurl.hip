// Host side of the H(div) / H(curl) kernels (hdivcurl.hpp): fx_hdivcurl_tabulate_batch / _grid_batch (the fused route) and
// fx_table_place_batch (the general route's placement pass).  Its own translation unit, compiled beside api.hip, wg.hip and
// bernstein.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>

#include "../../include/fiat_amd.h"
#include "hdivcurl.hpp"
#include "host_common.hpp"

namespace fx {
void line_facts(const fx_line_element* e, fxk::LineDesc* L);
}  // namespace fx

namespace {

// instances: quadrilaterals K = 1..4, hexahedra K = 1..3, orders 0..2
constexpr int HDC_MAXK_QUAD = 4, HDC_MAXK_HEX = 3, HDC_MAX_ORDER = 2;

template <int SD, int MAXK>
hipError_t launch_sd(int K, int order, int kind, bool grid_mode, unsigned grid, size_t lds, hipStream_t s, const fxk::HdcArgs& a) {
    return dispatch_int<1, MAXK>(K, [&](auto KK) {
        return dispatch_int<0, HDC_MAX_ORDER>(order, [&](auto ORDER) {
            return dispatch_int<fxk::HDC_DIV, fxk::HDC_CURL>(kind, [&](auto KIND) {
                return grid_mode ? launch_wave64(fxk::hdivcurl_kernel<SD, KK(), ORDER(), KIND(), true>, grid, lds, s, a)
                                 : launch_wave64(fxk::hdivcurl_kernel<SD, KK(), ORDER(), KIND(), false>, grid, lds, s, a);
            });
        });
    });
}

int hdivcurl_launch(const char* who, fx_ctx* ctx, int sd, int kind, const fx_line_element* C, const fx_line_element* D,
                    const int* offset, const int* sign, int order, int64_t nreq, int npts, int q, const double* pts, double* out,
                    void* stream, bool grid_mode) {
    if (!ctx || !C || !D || !offset || !sign) return fail(FX_EINVAL, "%s: null context, factor or descriptor", who);
    if (sd != 2 && sd != 3) return fail(FX_EINVAL, "%s: spatial dimension %d (quadrilaterals and hexahedra)", who, sd);
    if (kind != FX_HDIV && kind != FX_HCURL) return fail(FX_EINVAL, "%s: kind %d (FX_HDIV or FX_HCURL)", who, kind);
    if (order < 0 || nreq < 0 || npts < 0 || q < 0) return fail(FX_EINVAL, "%s: negative order or count", who);
    fxk::LineDesc LC, LD;
    fx::line_facts(C, &LC);
    fx::line_facts(D, &LD);
    const int K = LD.nn;
    if (LC.nn != K + 1) return fail(FX_EINVAL, "%s: C must have one node more than D (%d and %d nodes)", who, LC.nn, LD.nn);
    // blocks: all of one size, tiling the dofs [0, ndof) in some order
    const int nb = (int)(sd == 2 ? (K + 1) * K : (kind == FX_HDIV ? (K + 1) * K * K : (K + 1) * (K + 1) * K));
    int nblocks = 0;
    for (int c = 0; c < sd; ++c) {
        if (offset[c] >= 0) ++nblocks;
        if (offset[c] >= 0 && sign[c] != 1 && sign[c] != -1) return fail(FX_EINVAL, "%s: sign %d of component %d", who, sign[c], c);
    }
    if (nblocks == 0) return fail(FX_EINVAL, "%s: no block", who);
    const int ndof = nblocks * nb;
    for (int c = 0; c < sd; ++c) {
        if (offset[c] < 0) continue;
        if (offset[c] % nb != 0 || offset[c] + nb > ndof) return fail(FX_EINVAL, "%s: block offset %d of component %d out of range", who, offset[c], c);
        for (int c2 = 0; c2 < c; ++c2)
            if (offset[c2] == offset[c]) return fail(FX_EINVAL, "%s: blocks of components %d and %d overlap", who, c2, c);
    }
    if (order > HDC_MAX_ORDER) return fail(FX_ENOTIMPL, "%s: derivative order %d > %d", who, order, HDC_MAX_ORDER);
    if (K < 1 || K > (sd == 2 ? HDC_MAXK_QUAD : HDC_MAXK_HEX))
        return fail(FX_ENOTIMPL, "%s: no instance for %d-node factors on %s", who, K, sd == 2 ? "quadrilaterals" : "hexahedra");
    if (nreq == 0 || npts == 0) return FX_OK;
    if (!pts || !out) return fail(FX_EINVAL, "%s: null device pointer", who);

    int device = 0, num_cu = 0, lds_per_cu = 0;
    fx::ctx_facts(ctx, &device, &num_cu, &lds_per_cu);
    const int ntab = (int)(sd == 2 ? (order + 1) * (order + 2) / 2 : (order + 1) * (order + 2) * (order + 3) / 6);
    const long long reqsize = (long long)ntab * ndof * sd * npts;
    if (reqsize >= (1LL << 31)) return fail(FX_ENOTIMPL, "%s: request of %lld entries", who, reqsize);
    fxk::HdcArgs a;
    memset(&a, 0, sizeof a);
    a.pts = pts;
    a.out = out;
    a.C = LC;
    a.D = LD;
    for (int c = 0; c < 3; ++c) {
        a.off[c] = c < sd ? offset[c] : -1;
        a.sign[c] = c < sd && offset[c] >= 0 ? (double)sign[c] : 0.0;
    }
    a.nreq = nreq;
    a.npts = npts;
    a.q = q;
    a.ndof = ndof;
    const ItemPlan ip = plan_items(npts, reqsize, fxk::HDC_IMAGE_BYTES, false);
    a.P = ip.P;
    a.image = ip.image;
    a.nitems = (nreq + ip.P - 1) / ip.P;
    const unsigned grid = item_grid(a.nitems, num_cu, 64);
    FX_HIP_TRY(hipSetDevice(device));
    FX_HIP_TRY((sd == 2 ? launch_sd<2, HDC_MAXK_QUAD>(K, order, kind, grid_mode, grid, ip.image_bytes, (hipStream_t)stream, a)
                        : launch_sd<3, HDC_MAXK_HEX>(K, order, kind, grid_mode, grid, ip.image_bytes, (hipStream_t)stream, a)));
    return FX_OK;
}

}  // namespace

extern "C" {

int fx_hdivcurl_tabulate_batch(fx_ctx* ctx, int sd, int kind, const fx_line_element* C, const fx_line_element* D,
                               const int* offset, const int* sign, int order, int64_t nreq, int npts, const double* pts,
                               double* out, void* stream) {
    return hdivcurl_launch("fx_hdivcurl_tabulate_batch", ctx, sd, kind, C, D, offset, sign, order, nreq, npts, 0, pts, out,
                           stream, false);
}

int fx_hdivcurl_tabulate_grid_batch(fx_ctx* ctx, int sd, int kind, const fx_line_element* C, const fx_line_element* D,
                                    const int* offset, const int* sign, int order, int64_t nreq, int q, const double* grid,
                                    double* out, void* stream) {
    if (q < 0 || q > 64) return fail(q < 0 ? FX_EINVAL : FX_ENOTIMPL, "fx_hdivcurl_tabulate_grid_batch: grid size %d", q);
    int npts = 1;
    for (int d = 0; d < sd && d < 3; ++d) npts *= q;
    return hdivcurl_launch("fx_hdivcurl_tabulate_grid_batch", ctx, sd, kind, C, D, offset, sign, order, nreq, npts, q, grid,
                           out, stream, true);
}

int fx_table_place_batch(fx_ctx* ctx, int ntab, int64_t nreq, int npts, int rows_src, int vdim_src, const double* src,
                         int rows_dst, int vdim_dst, int row_offset, const int* comp_src, const int* comp_sign, double* dst,
                         void* stream) {
    if (!ctx || !comp_src || !comp_sign) return fail(FX_EINVAL, "fx_table_place_batch: null context or component map");
    if (ntab < 0 || nreq < 0 || npts < 0 || rows_src < 0 || rows_dst < 0) return fail(FX_EINVAL, "fx_table_place_batch: negative count");
    if (vdim_src < 1 || vdim_src > 9 || vdim_dst < 1 || vdim_dst > 9) return fail(FX_EINVAL, "fx_table_place_batch: value sizes %d, %d (1..9)", vdim_src, vdim_dst);
    if (row_offset < 0 || row_offset + rows_src > rows_dst) return fail(FX_EINVAL, "fx_table_place_batch: rows [%d, %d) outside [0, %d)", row_offset, row_offset + rows_src, rows_dst);
    fxk::PlaceArgs a;
    memset(&a, 0, sizeof a);
    for (int c = 0; c < vdim_dst; ++c) {
        if (comp_src[c] >= vdim_src) return fail(FX_EINVAL, "fx_table_place_batch: source component %d of %d", comp_src[c], vdim_src);
        a.comp[c] = comp_src[c] < 0 ? -1 : comp_src[c];
        a.sign[c] = (double)comp_sign[c];
    }
    const long long total = (long long)nreq * ntab * rows_src * vdim_dst * npts;
    if (total == 0) return FX_OK;
    if (!src || !dst) return fail(FX_EINVAL, "fx_table_place_batch: null device pointer");
    int device = 0, num_cu = 0, lds_per_cu = 0;
    fx::ctx_facts(ctx, &device, &num_cu, &lds_per_cu);
    a.src = src;
    a.dst = dst;
    a.nrows = (long long)nreq * ntab * rows_src;
    a.rows_src = rows_src;
    a.vdim_src = vdim_src;
    a.rows_dst = rows_dst;
    a.vdim_dst = vdim_dst;
    a.row_offset = row_offset;
    a.npts = npts;
    const dim3 grid((unsigned)std::max<long long>(1, std::min<long long>((total + 255) / 256, (long long)num_cu * 32)));
    FX_HIP_TRY(hipSetDevice(device));
    hipLaunchKernelGGL(fxk::table_place_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
    FX_HIP_TRY(hipGetLastError());
    return FX_OK;
}

}  // extern "C"
