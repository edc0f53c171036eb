// Output stores of the tabulation kernels and the phase fence of a wave (gfx950).
#pragma once
#include <hip/hip_runtime.h>
#include "ablation.hpp"

#ifndef FX_NT_STORES
#define FX_NT_STORES 1
#endif

namespace fxk {

__device__ __forceinline__ void wave_lds_fence() {
    // LDS operations of one wave complete in order; this only stops the compiler from
    // moving LDS accesses of different lanes across a phase boundary.  The fences are
    // restricted to the LDS address space ("local"): an unrestricted release fence makes
    // hipcc wait vmcnt(0), i.e. for every outstanding HBM store of the wave -- measured
    // to serialise the store phase with the next request's compute.
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
}

// Output tables are written once and read by later kernels: non-temporal stores let the L2
// stream them out instead of holding them as dirty lines until an eviction is forced
// (measured on the P3 tet benchmark, K-streamed kernel, same box and run, interleaved:
// 330 -> 301 us per 100 000 requests).
template <class T> __device__ __forceinline__ void stream_store(T* p, const T& v) {
#if FX_NT_STORES
    __builtin_nontemporal_store(v, p);
#else
    *p = v;
#endif
}

// One wave copies a contiguous block of `nch` 16-byte chunks from its LDS image to global memory.  The block (an item of
// whole requests) starts anywhere in a 128-byte line.  The body goes out as non-temporal stores that cover WHOLE lines
// (lane i of an instruction takes chunk head + 64 it + i: every instruction starts on a line boundary); the partial first
// and last line of the block are shared with the neighbouring blocks, which other waves write at other times, and go out as
// PLAIN masked stores: a non-temporal partial write leaves the L2 at once and the two parts of the line reach memory as
// separate masked writes, a plain one waits in the L2 for its other part.  Round 3, lane-local kernel, 50 shapes, interleaved
// A/B (tools/map_ab.sh): geometric mean of the launch times 0.956 of the plain loop over all chunks, best 0.81, worst 1.04;
// all-plain stores: 1.18.  (RT2 requests, which are not line multiples either: simplex_pair.hpp)
template <class V2> __device__ __forceinline__ void flush_block(V2* g2, const V2* s2, int nch, int lane) {
    const int shift = (int)((reinterpret_cast<unsigned long long>(g2) >> 4) & 7ull);
    const int head = min(nch, (8 - shift) & 7);
    const int body_end = head + ((nch - head) & ~7);
    if (lane < head) g2[lane] = s2[lane];
    for (int i = head + lane; i < body_end; i += 64) stream_store(&g2[i], s2[i]);
    if (body_end + lane < nch) g2[body_end + lane] = s2[body_end + lane];
}

// One wave writes the LDS image of its item, `total` doubles that are contiguous in global memory from `gout`, and gives the
// image back: as 16-byte chunks through flush_block where the block allows it (an even total from a 16-byte boundary; an
// `out=` view or an odd request may start 8 bytes off), one double per lane and step otherwise.
__device__ __forceinline__ void flush_item(double* gout, const double* img, long long total, int lane) {
    wave_lds_fence();
    if ((total & 1) == 0 && (reinterpret_cast<unsigned long long>(gout) & 15ull) == 0) {
        typedef double chunk __attribute__((ext_vector_type(2)));
        flush_block(reinterpret_cast<chunk*>(gout), reinterpret_cast<const chunk*>(img), (int)(total >> 1), lane);
    } else {
        for (long long i = lane; i < total; i += 64) gout[i] = img[i];
    }
    wave_lds_fence();  // the next item overwrites the image
}

}  // namespace fxk
