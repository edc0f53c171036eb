// Host scaffold of the main library (api.hip) and the wave-per-item kernel families (bernstein, hdivcurl, serendipity, sforms,
// dpc, trace, hierarchical, evaluate, cellmap .hip): the error slot, the device buffers, the item plan, the grid and the launch.  Everything has internal linkage: each family is
// its own translation unit, most of them their own library, and none exports these names.  What a family keeps for itself:
// its validation and message texts, its Args, its kernel and its item loop.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <type_traits>

#include "../../include/fiat_amd.h"
#include "device_buffer.hpp"

namespace fx {
int set_error(int code, const char* msg);  // api.hip (libfiat_amd.so): one error slot, shared contexts
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

#define FX_HIP_TRY(expr)                                                          \
    do {                                                                          \
        hipError_t e_ = (expr);                                                   \
        if (e_ != hipSuccess) {                                                   \
            (void)hipGetLastError();                                              \
            return fail(FX_EHIP, "%s: %s", #expr, hipGetErrorString(e_));         \
        }                                                                         \
    } while (0)

// The one place where device memory is allocated and freed (device_buffer.hpp).
struct HipMemory {
    using error_t = hipError_t;
    using stream_t = hipStream_t;
    static constexpr hipError_t ok = hipSuccess;
    static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
    static hipError_t free(void* p) { return hipFree(p); }
    static hipError_t copy_in(void* dst, const void* src, size_t bytes) { return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice); }
    static hipError_t zero(void* dst, size_t bytes) { return hipMemset(dst, 0, bytes); }
    static hipError_t alloc_async(void** p, size_t bytes, hipStream_t s) { return hipMallocAsync(p, bytes, s); }
    static hipError_t free_async(void* p, hipStream_t s) { return hipFreeAsync(p, s); }
    static void clear_error() { (void)hipGetLastError(); }
};
template <class T> using DeviceBuffer = fx::DeviceBuffer<T, HipMemory>;
template <class T> using StreamScratch = fx::StreamScratch<T, HipMemory>;

// How the requests of a launch are grouped into items, one wave each.  An item is P whole requests, as many as 64 lanes
// hold at one point per lane (one request in chunks of 64 points beyond).  Where requests of `reqsize` doubles fit
// `budget_bytes` the item goes through a per-wave LDS image (rounded to whole 16-byte chunks) and is flushed from there
// (store.hpp flush_item); otherwise the lanes stream their entries.  shrink: P shrinks to the requests that fit together
// (every request that fits alone takes the image); !shrink: P stays, and the image is taken where all P fit.
struct ItemPlan {
    int P, image;
    size_t image_bytes;
};

ItemPlan plan_items(int npts, long long reqsize, long long budget_bytes, bool shrink) {
    ItemPlan p{npts > 0 && npts <= 64 ? 64 / npts : 1, 0, 0};
    if (reqsize <= 0) return p;
    const long long fit = budget_bytes / (reqsize * 8);
    if (fit >= (shrink ? 1 : p.P)) {
        p.image = 1;
        p.P = (int)std::min<long long>(p.P, fit);
        p.image_bytes = (size_t)(((long long)p.P * reqsize + 1) & ~1LL) * 8;
    }
    return p;
}

// workgroups of a launch: one per item up to per_cu per compute unit, the kernels loop over the rest
unsigned item_grid(long long nitems, int num_cu, int per_cu) {
    return (unsigned)std::max<long long>(1, std::min<long long>(nitems, (long long)num_cu * per_cu));
}

// one-wave workgroups; more than 48 KB of dynamic LDS has to be allowed per kernel first
template <class... Params, class... Args>
hipError_t launch_wave64(void (*kernel)(Params...), unsigned grid, size_t lds, hipStream_t s, const Args&... args) {
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(64), lds, s, args...);
    return hipGetLastError();
}

// f(std::integral_constant<int, v>{}) for a run-time v in [LO, HI]: the template arguments of a launch.  Validation runs
// before; a value outside the range launches nothing.
template <int LO, int HI, class F> hipError_t dispatch_int(int v, F&& f) {
    if (v == LO) return f(std::integral_constant<int, LO>{});
    if constexpr (LO < HI) return dispatch_int<LO + 1, HI>(v, f);
    else return hipErrorInvalidValue;
}

}  // namespace
