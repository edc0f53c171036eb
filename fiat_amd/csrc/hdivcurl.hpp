// H(div) / H(curl) tensor-product elements on quadrilaterals and hexahedra, fused (gfx950): RTCF / RTCE / NCF / NCE as
// Firedrake composes them, and their single summands.
//
// Reference behaviour: Hdiv / Hcurl (FIAT/hdivcurl.py:13-254) place the table of a product of 1-D elements into one
// component of a vector field, with a sign; EnrichedElement (FIAT/enriched.py:88-112) concatenates the dofs of its summands.
// Walked down to the 1-D factors (fiat_amd/hdivcurl.py), such an element is a set of BLOCKS, at most one per component c:
// block c is the product over the directions d of C (a 1-D Lagrange element with K+1 nodes) or D (K nodes) -- H(div): C
// where d == c, H(curl): D where d == c -- its dofs a contiguous range from off[c], row-major over (x, y[, z]), times a
// sign.  Every dof has exactly one nonzero component; FIAT's layout [ndof][sd][npts] still holds the zeros of the others.
//
// Lane <-> (request, point), as tensor_small_kernel: the lane evaluates C and D and their derivatives at its point in
// registers (compile-time node counts), then writes every table and dof: the signed product into the block's component and
// zeros into the other components.  Blocks, directions and dofs are compile-time loops, so no array is indexed at run time.
// An item of P whole requests (P * npts <= 64; one request in chunks of 64 points beyond) goes through a per-wave LDS image
// and leaves as whole-line non-temporal stores (store.hpp flush_item) where it fits HDC_IMAGE_BYTES; larger requests stream: every
// lane stores its own entries with plain stores, and the L2 joins the partial lines of neighbouring lanes and rows.
#pragma once
#include <hip/hip_runtime.h>

#include "line_basis.hpp"
#include "store.hpp"

namespace fxk {

constexpr int HDC_DIV = 0, HDC_CURL = 1;
constexpr int HDC_IMAGE_BYTES = 40 * 1024;  // largest per-wave LDS image; larger items stream

struct HdcArgs {
    const double* pts;  // [nreq][npts][sd], GRID: [nreq][sd][q] 1-D coordinates of a tensor grid
    double* out;        // [nreq][ntab][ndof][sd][npts]
    LineDesc C, D;      // K + 1 and K nodes
    double sign[3];     // of each component's block
    int off[3];         // first dof of each component's block, -1: no block
    long long nreq, nitems;
    int npts, q, ndof;
    int P;              // whole requests per item
    int image;          // 1: per-wave LDS image of the item, 0: streaming stores
};

// is direction d of block c the K+1-node factor C?
template <int KIND> constexpr bool hdc_is_c(int c, int d) { return KIND == HDC_DIV ? d == c : d != c; }

// block c: every table and dof of this lane's point.  dst = the lane's (t = 0, first dof of the block, component 0) entry, in
// the image or in HBM; npts / rstride = sd * npts (doubles per dof row) / tstride = ndof * rstride (per table).  The row
// pointer advances by rstride per dof: the offsets are runtime values, and a compile-time multiple of each per store would
// be hoisted out of the item loop as hundreds of live registers (measured: 512 VGPRs and scratch on hexahedra).
template <int SD, int K, int ORDER, int KIND, int CB>
__device__ __forceinline__ void hdc_block(const double (&TC)[SD][ORDER + 1][K + 1], const double (&TD)[SD][ORDER + 1][K],
                                          double sign, double* dst, int npts, int rstride, int tstride) {
    constexpr TensorAlpha<SD, ORDER> AL{};
    constexpr int NTAB = TensorAlpha<SD, ORDER>::NTAB;
    constexpr int n0 = hdc_is_c<KIND>(CB, 0) ? K + 1 : K;
    constexpr int n1 = hdc_is_c<KIND>(CB, 1) ? K + 1 : K;
    constexpr int n2 = SD == 3 ? (hdc_is_c<KIND>(CB, 2) ? K + 1 : K) : 1;
    // the block's factors, direction by direction (register renames: every index is a constant)
    double F[SD][ORDER + 1][K + 1];
#pragma unroll
    for (int d = 0; d < SD; ++d)
#pragma unroll
        for (int k = 0; k <= ORDER; ++k)
#pragma unroll
            for (int i = 0; i <= K; ++i) F[d][k][i] = hdc_is_c<KIND>(CB, d) ? TC[d][k][i] : (i < K ? TD[d][k][i] : 0.0);
    double* trow = dst;
#pragma unroll
    for (int t = 0; t < NTAB; ++t) {
        double* row = trow;
#pragma unroll
        for (int i0 = 0; i0 < n0; ++i0) {
#pragma unroll
            for (int i1 = 0; i1 < n1; ++i1) {
                const double v01 = sign * F[0][AL.a[t][0]][i0] * F[1][AL.a[t][1]][i1];
#pragma unroll
                for (int i2 = 0; i2 < n2; ++i2) {
                    double v = v01;
                    if constexpr (SD == 3) v *= F[2][AL.a[t][2]][i2];
                    double* e = row;
#pragma unroll
                    for (int c = 0; c < SD; ++c) {
                        *e = c == CB ? v : 0.0;
                        e += npts;
                    }
                    row += rstride;
                }
            }
        }
        trow += tstride;
    }
}

template <int SD, int K, int ORDER, int KIND, bool GRID>
__global__ __launch_bounds__(64) void hdivcurl_kernel(const HdcArgs a) {
    static_assert(SD == 2 || SD == 3, "quadrilaterals and hexahedra");
    constexpr int NTAB = TensorAlpha<SD, ORDER>::NTAB;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int lane = threadIdx.x & 63;
    const int npts = a.npts;
    const int rstride = SD * npts;
    const int tstride = a.ndof * rstride;
    const long long reqsize = (long long)NTAB * tstride;
    for (long long item = blockIdx.x; item < a.nitems; item += gridDim.x) {
        const long long r0 = item * a.P;
        const long long left = a.nreq - r0;
        const int Pcur = left < a.P ? (int)left : a.P;
        const int nslots = Pcur * npts;
        double* gout = a.out + (size_t)r0 * reqsize;
        for (int s0 = 0; s0 < nslots; s0 += 64) {
            const int slot = s0 + lane;
            const bool active = slot < nslots;
            const int rl = active ? slot / npts : 0;
            const int pl = active ? slot - rl * npts : 0;
            const long long r = r0 + rl;
            // C and D and their derivatives at this lane's point: T?[d][k][i] = k-th derivative of basis function i at x_d
            double TC[SD][ORDER + 1][K + 1], TD[SD][ORDER + 1][K];
#pragma unroll
            for (int d = 0; d < SD; ++d) {
                double x;
                if constexpr (GRID) {
                    const int q = a.q;
                    int j = pl;  // point = row-major (j0, j1[, j2])
                    if (d == 0) j = SD == 2 ? pl / q : pl / (q * q);
                    else if (d == 1) j = SD == 2 ? pl % q : (pl / q) % q;
                    else j = pl % q;
                    x = a.pts[((size_t)r * SD + d) * q + j];
                } else {
                    x = a.pts[((size_t)r * npts + pl) * SD + d];
                }
                lagrange_values_n<K + 1>(a.C, x, TC[d][0]);
                lagrange_values_n<K>(a.D, x, TD[d][0]);
#pragma unroll
                for (int k = 1; k <= ORDER; ++k) {
                    lagrange_diff_n<K + 1>(a.C, TC[d][k - 1], TC[d][k]);
                    lagrange_diff_n<K>(a.D, TD[d][k - 1], TD[d][k]);
                }
            }
            if (!active) continue;
            // (opaque per item: the strides stay single registers instead of hoisted multiples, see hdc_block)
            int np = npts, rs = rstride, ts = tstride;
            asm volatile("" : "+v"(np), "+v"(rs), "+v"(ts));
            double* base = (a.image ? lds : gout) + (size_t)rl * reqsize + pl;
            if (a.off[0] >= 0) hdc_block<SD, K, ORDER, KIND, 0>(TC, TD, a.sign[0], base + a.off[0] * rs, np, rs, ts);
            if (a.off[1] >= 0) hdc_block<SD, K, ORDER, KIND, 1>(TC, TD, a.sign[1], base + a.off[1] * rs, np, rs, ts);
            if constexpr (SD == 3)
                if (a.off[2] >= 0) hdc_block<SD, K, ORDER, KIND, 2>(TC, TD, a.sign[2], base + a.off[2] * rs, np, rs, ts);
        }
        if (a.image) flush_item(gout, lds, (long long)Pcur * reqsize, lane);
    }
}

// General route: the table of one leaf of the composition (nreq, ntab, rows_src, vdim_src, npts) placed into the rows
// [row_offset, row_offset + rows_src) of the output (nreq, ntab, rows_dst, vdim_dst, npts): component c of the output is
// sign[c] * component comp[c] of the leaf, or zero (comp[c] < 0).  One thread per output entry of those rows, all
// components written, so the output needs no memset when the leaves tile its rows.
struct PlaceArgs {
    const double* src;
    double* dst;
    long long nrows;  // nreq * ntab * rows_src
    int rows_src, vdim_src, rows_dst, vdim_dst, row_offset, npts;
    int comp[9];
    double sign[9];
};

__global__ __launch_bounds__(256) void table_place_kernel(const PlaceArgs a) {
    const long long per_row = (long long)a.vdim_dst * a.npts;
    const long long total = a.nrows * per_row;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        const long long row = e / per_row;  // (request, table, leaf row)
        const int rem = (int)(e - row * per_row);
        const int c = rem / a.npts, p = rem - c * a.npts;
        const long long rt = row / a.rows_src;  // request * ntab + table
        const int i = (int)(row - rt * a.rows_src);
        int sc = -1;
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 9; ++k)  // (compile-time indices: the two kernarg arrays stay out of scratch)
            if (k == c) {
                sc = a.comp[k];
                s = a.sign[k];
            }
        const double v = sc >= 0 ? s * a.src[((size_t)row * a.vdim_src + sc) * a.npts + p] : 0.0;
        a.dst[(((size_t)rt * a.rows_dst + a.row_offset + i) * a.vdim_dst + c) * a.npts + p] = v;
    }
}

}  // namespace fxk
