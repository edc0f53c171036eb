// fiat_amd/csrc/device_buffer.hpp on a counting heap that can be told to fail its k-th allocation or copy: ownership across
// moves, the failure contract of upload / alloc, build-then-commit of a handle with five buffers under a failure at each of
// its ten steps, and the stream-ordered scratch.  Built with -fsanitize=address,undefined by tests/test_plan_sanitizers.py;
// a leak or a double free ends the run.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <utility>
#include <vector>

#include "../../fiat_amd/csrc/device_buffer.hpp"

#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

namespace {

struct Heap {
    using error_t = int;
    using stream_t = int;
    static constexpr int ok = 0;
    static std::set<void*> live;
    static int ops, fail_at, frees, async_frees, last_free_stream, sticky;

    // the k-th allocation or copy (from 1) since arm(k) fails; 0: none does
    static void arm(int k) {
        ops = 0;
        fail_at = k;
    }
    static bool failing() { return ++ops == fail_at; }
    static int alloc(void** p, size_t bytes) {
        if (failing()) return sticky = 2;
        *p = std::malloc(bytes ? bytes : 1);
        live.insert(*p);
        return ok;
    }
    static int free(void* p) {
        CHECK(live.erase(p) == 1);  // freed once, and only what was allocated
        std::free(p);
        ++frees;
        return ok;
    }
    static int copy_in(void* dst, const void* src, size_t bytes) {
        CHECK(live.count(dst) == 1);
        if (failing()) return sticky = 3;
        std::memcpy(dst, src, bytes);
        return ok;
    }
    static int zero(void* dst, size_t bytes) {
        CHECK(live.count(dst) == 1);
        if (failing()) return sticky = 4;
        std::memset(dst, 0, bytes);
        return ok;
    }
    static int alloc_async(void** p, size_t bytes, int) { return alloc(p, bytes); }
    static int free_async(void* p, int s) {
        last_free_stream = s;
        ++async_frees;
        return free(p);
    }
    static void clear_error() { sticky = 0; }
};
std::set<void*> Heap::live;
int Heap::ops = 0, Heap::fail_at = 0, Heap::frees = 0, Heap::async_frees = 0, Heap::last_free_stream = -1, Heap::sticky = 0;

template <class T> using Buffer = fx::DeviceBuffer<T, Heap>;

void moves() {
    const double one[3] = {1.0, 2.0, 3.0};
    {
        Buffer<double> a;
        CHECK(!a && a.get() == nullptr);
        CHECK(a.reset() == Heap::ok && Heap::frees == 0);  // reset on empty
        CHECK(a.upload(one, 3) == Heap::ok && a && a.get()[2] == 3.0);
        double* pa = a.get();
        Buffer<double> b(std::move(a));  // move construction
        CHECK(!a && b.get() == pa && Heap::live.size() == 1);
        Buffer<double> c;
        CHECK(c.alloc(5, true) == Heap::ok && c.get()[4] == 0.0 && Heap::live.size() == 2);
        double* pc = c.get();
        const int before = Heap::frees;
        c = std::move(b);  // move assignment: the target's old allocation goes, exactly once
        CHECK(Heap::frees == before + 1 && Heap::live.count(pc) == 0 && c.get() == pa && !b);
        Buffer<double>& alias = c;
        c = std::move(alias);  // self-move
        CHECK(c.get() == pa && Heap::frees == before + 1 && Heap::live.size() == 1);
        CHECK(c.upload(one, 2, 4) == Heap::ok && Heap::live.size() == 1);  // a second upload replaces the first
        CHECK(c.upload(nullptr, 0, 1) == Heap::ok && c);                    // nothing to copy: room only
    }
    CHECK(Heap::live.empty());
}

void failed_uploads() {
    const int v[4] = {1, 2, 3, 4};
    for (int k = 1; k <= 2; ++k) {  // 1: at the allocation, 2: at the copy
        Buffer<int> a;
        Heap::arm(k);
        CHECK(a.upload(v, 4) != Heap::ok);
        CHECK(!a && Heap::live.empty() && Heap::sticky == 0);
        Heap::arm(k);
        CHECK(a.alloc(4, true) != Heap::ok);
        CHECK(!a && Heap::live.empty() && Heap::sticky == 0);
    }
    Buffer<int> keep;  // a failed upload on a buffer that holds something: empty afterwards, nothing leaked
    Heap::arm(0);
    CHECK(keep.upload(v, 4) == Heap::ok);
    Heap::arm(2);
    CHECK(keep.upload(v, 4) != Heap::ok && !keep && Heap::live.empty());
    Heap::arm(0);
}

// a handle as the library's: five buffers and the scalars derived with them
struct Handle {
    Buffer<double> cmat, afrag, split;
    Buffer<int> eint, kstart;
    int ndof = 0, vdim = 0, MT = 0, KS = 0;
};
struct Snapshot {
    const void* p[5];
    int s[4];
};
Snapshot snapshot(const Handle& h) {
    Snapshot s;
    std::memset(&s, 0, sizeof s);
    const void* p[5] = {h.cmat.get(), h.afrag.get(), h.split.get(), h.eint.get(), h.kstart.get()};
    const int v[4] = {h.ndof, h.vdim, h.MT, h.KS};
    std::memcpy(s.p, p, sizeof p);
    std::memcpy(s.s, v, sizeof v);
    return s;
}

int set_coeffs(Handle& h, int ndof, int vdim) {
    const int rows = ndof * vdim;
    std::vector<double> C((size_t)rows * 4, 1.5);
    std::vector<int> I((size_t)rows, 7);
    Buffer<double> cmat, afrag, split;
    Buffer<int> eint, kstart;
    int e;
    if ((e = cmat.upload(C.data(), C.size())) != Heap::ok) return e;
    if ((e = afrag.upload(C.data(), C.size())) != Heap::ok) return e;
    if ((e = split.upload(C.data(), C.size())) != Heap::ok) return e;
    if ((e = eint.upload(I.data(), I.size())) != Heap::ok) return e;
    if ((e = kstart.upload(I.data(), I.size())) != Heap::ok) return e;
    h.cmat = std::move(cmat);
    h.afrag = std::move(afrag);
    h.split = std::move(split);
    h.eint = std::move(eint);
    h.kstart = std::move(kstart);
    h.ndof = ndof;
    h.vdim = vdim;
    h.MT = (rows + 15) / 16;
    h.KS = 1;
    return Heap::ok;
}

void build_then_commit() {
    {
        Handle h;
        Heap::arm(0);
        CHECK(set_coeffs(h, 6, 1) == Heap::ok && Heap::live.size() == 5);
        for (int k = 1; k <= 10; ++k) {  // five allocations and five copies
            const Snapshot before = snapshot(h);
            const size_t live = Heap::live.size();
            Heap::arm(k);
            CHECK(set_coeffs(h, 4, 2) != Heap::ok);
            const Snapshot after = snapshot(h);
            CHECK(std::memcmp(&before, &after, sizeof before) == 0);
            CHECK(Heap::live.size() == live && Heap::sticky == 0);
            for (const void* p : before.p) CHECK(Heap::live.count(const_cast<void*>(p)) == 1);
        }
        Heap::arm(11);  // (no eleventh step)
        CHECK(set_coeffs(h, 4, 2) == Heap::ok && h.ndof == 4 && h.vdim == 2 && Heap::live.size() == 5);
        Heap::arm(0);
    }
    CHECK(Heap::live.empty());
}

void stream_scratch() {
    {
        fx::StreamScratch<double, Heap> s;
        CHECK(s.get() == nullptr);
        CHECK(s.alloc(16, 42) == Heap::ok && s.get() && Heap::live.size() == 1);
        CHECK(Heap::async_frees == 0);
    }
    CHECK(Heap::live.empty() && Heap::async_frees == 1 && Heap::last_free_stream == 42);  // on scope exit, on its stream
    {
        fx::StreamScratch<double, Heap> s;
        Heap::arm(1);
        CHECK(s.alloc(16, 7) != Heap::ok && s.get() == nullptr && Heap::sticky == 0);
        Heap::arm(0);
    }
    CHECK(Heap::async_frees == 1);  // nothing to release
}

}  // namespace

int main() {
    moves();
    failed_uploads();
    build_then_commit();
    stream_scratch();
    CHECK(Heap::live.empty());
    std::printf("buffers ok\n");
    return 0;
}
