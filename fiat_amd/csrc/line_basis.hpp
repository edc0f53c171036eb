// 1-D Lagrange bases of the tensor-product kernels (gfx950): node data, the barycentric evaluation in registers, and the
// derivative multi-indices of a product of interval factors.  Shared by aux_kernels.hpp / tensor_small.hpp (api.hip) and
// hdivcurl.hpp (hdivcurl.hip): device functions and types only, no kernels, so every translation unit may include it.
#pragma once
#include <hip/hip_runtime.h>

namespace fxk {

// ---------------------------------------------------------------------------
// 1-D Lagrange basis by the second barycentric formula
// (barycentric_interpolation.py:22-47).  tab layout [k][i] in registers of the
// calling lane for one point; NN_MAX bounds the node count.
constexpr int NN_MAX = 16;

struct LineDesc {
    const double* nodes;  // [nn]
    const double* wts;    // [nn] barycentric weights
    const double* dmat;   // [nn][nn] differentiation matrix
    int nn;
};

// values phi[i] at x; exact Kronecker delta when x hits a node
// (barycentric_interpolation.py:35-40: NaN -> 1 after the normalisation).
// (node data through the constant address space: never written while a kernel runs, so the loads are scalar)
typedef const __attribute__((address_space(4))) double LineConst;

__device__ __forceinline__ void lagrange_values(const LineDesc& L, double x, double* phi) {
    LineConst* nodes = (LineConst*)(unsigned long long)L.nodes;
    LineConst* wts = (LineConst*)(unsigned long long)L.wts;
    double sum = 0.0;
    int hit = -1;
#pragma unroll
    for (int i = 0; i < NN_MAX; ++i) {
        if (i < L.nn) {
            double d = x - nodes[i];
            if (d == 0.0) hit = i;
            double t = wts[i] / d;
            phi[i] = t;
            sum += t;
        }
    }
    double inv = 1.0 / sum;
#pragma unroll
    for (int i = 0; i < NN_MAX; ++i) {
        if (i < L.nn) phi[i] = (hit >= 0) ? ((i == hit) ? 1.0 : 0.0) : phi[i] * inv;
    }
}

// out = dmat . in
__device__ __forceinline__ void lagrange_diff(const LineDesc& L, const double* in, double* out) {
    LineConst* dmat = (LineConst*)(unsigned long long)L.dmat;
#pragma unroll
    for (int i = 0; i < NN_MAX; ++i) {
        if (i < L.nn) {
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < NN_MAX; ++j)
                if (j < L.nn) s += dmat[i * L.nn + j] * in[j];
            out[i] = s;
        }
    }
}

// the same with a compile-time node count: every index is a constant, the node data are uniform loads
template <int NN> __device__ __forceinline__ void lagrange_values_n(const LineDesc& L, double x, double (&phi)[NN]) {
    LineConst* nodes = (LineConst*)(unsigned long long)L.nodes;
    LineConst* wts = (LineConst*)(unsigned long long)L.wts;
    double sum = 0.0;
    int hit = -1;
#pragma unroll
    for (int i = 0; i < NN; ++i) {
        const double d = x - nodes[i];
        if (d == 0.0) hit = i;
        const double t = wts[i] / d;
        phi[i] = t;
        sum += t;
    }
    const double inv = 1.0 / sum;
#pragma unroll
    for (int i = 0; i < NN; ++i) phi[i] = hit >= 0 ? (i == hit ? 1.0 : 0.0) : phi[i] * inv;
}

template <int NN> __device__ __forceinline__ void lagrange_diff_n(const LineDesc& L, const double (&in)[NN], double (&out)[NN]) {
    LineConst* dmat = (LineConst*)(unsigned long long)L.dmat;
#pragma unroll
    for (int i = 0; i < NN; ++i) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < NN; ++j) s += dmat[i * NN + j] * in[j];
        out[i] = s;
    }
}

// derivative multi-indices in mis() order (polynomial_set.py:23-32), at compile time
template <int NF, int ORDER> struct TensorAlpha {
    static constexpr int NTAB = NF == 2 ? (ORDER + 1) * (ORDER + 2) / 2 : (ORDER + 1) * (ORDER + 2) * (ORDER + 3) / 6;
    int a[NTAB][3];
    constexpr TensorAlpha() : a{} {
        int t = 0;
        for (int k = 0; k <= ORDER; ++k) {
            if (NF == 2) {
                for (int i = 0; i <= k; ++i) {
                    a[t][0] = k - i;
                    a[t][1] = i;
                    a[t][2] = 0;
                    ++t;
                }
            } else {
                for (int i = 0; i <= k; ++i)
                    for (int j = 0; j <= i; ++j) {
                        a[t][0] = k - i;
                        a[t][1] = i - j;
                        a[t][2] = j;
                        ++t;
                    }
            }
        }
    }
};

}  // namespace fxk
