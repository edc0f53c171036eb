// Which work counter (work_queue.hpp) a launch of a dynamically scheduled kernel gets.  Host code without HIP calls: what it
// needs from the runtime -- the stream's id, the id of the capture in progress, device memory for more counters -- comes in
// as arguments and a callback, so that the rule runs on the CPU against simulated streams (tests/native/counter_handout.cpp).
//
// The kernels trust their counter completely: they draw chunk ids from it, count finished workgroups in it, and the last
// workgroup zeroes it.  Two launches that run at the same time on one counter each leave part of their tables unwritten.
// So the rule is: launches share a counter only if the device orders them.
//   * DIRECT launches: one counter per stream, for the life of the context.  Launches of one stream run one after the
//     other, whatever their number; launches of different streams never meet on a counter.
//   * CAPTURED launches (the stream is capturing into a graph): the graph bakes the counter's address in and may be replayed
//     any number of times, on any stream, beside any direct launch.  They get a counter per (stream, capture), drawn from
//     the same never-recycled sequence, so no direct launch and no other capture ever receives it.  The launches one stream
//     contributes to one capture are ordered inside the graph and share it.
// A counter once handed out is never handed to another stream or capture: indices only grow.  Counters are added a block at a
// time when a stream is seen for the first time; a capture may not allocate (the runtime refuses allocations while a
// stream captures), so direct launches keep RESERVE counters unassigned for the captures that follow them, and a capture
// that finds none left is refused (NO_SPARE) -- never given a counter in use.
// Not covered: one captured graph instantiated twice with both instances in flight at once (the two share every address
// the graph holds, its counters and its outputs alike).
//
// Not thread-safe: a context is driven by one host thread at a time (include/fiat_amd.h).
#pragma once
#include <unordered_map>

namespace fx {

class CounterHandout {
  public:
    static constexpr int BLOCK = 64;    // counters added at a time
    static constexpr int RESERVE = 16;  // unassigned counters kept back for captures
    enum { NO_SPARE = -1, GROW_FAILED = -2 };

    int capacity() const { return cap_; }

    // grow(first, count) -> bool: make counters first .. first + count - 1 exist, zeroed.
    // Called when the context is created: the first block, so that captures find counters before any direct launch.
    template <class Grow> bool reserve(Grow&& grow) { return cap_ - next_ >= RESERVE || add_block(grow); }

    // Index of the counter for a launch on the stream `stream_id` (one id per stream: the handle, which the caller keeps
    // alive while work is pending); `capture_id` = 0 for a direct launch, else the unique id of the capture the stream is part of.
    template <class Grow> int acquire(unsigned long long stream_id, unsigned long long capture_id, Grow&& grow) {
        if (capture_id == 0) {
            int idx;
            auto it = direct_.find(stream_id);
            if (it != direct_.end()) {
                idx = it->second;
            } else {
                if (next_ == cap_ && !add_block(grow)) return GROW_FAILED;
                idx = next_++;
                direct_.emplace(stream_id, idx);
            }
            if (cap_ - next_ < RESERVE) (void)add_block(grow);  // (a failure shows when the counters are needed)
            return idx;
        }
        auto it = captured_.find(stream_id);
        if (it != captured_.end() && it->second.capture == capture_id) return it->second.index;
        if (next_ == cap_) return NO_SPARE;
        const Captured c{capture_id, next_++};
        if (it != captured_.end()) it->second = c;  // (the stream's earlier capture has ended: its entry is not needed again)
        else captured_.emplace(stream_id, c);
        return c.index;
    }

  private:
    struct Captured {
        unsigned long long capture;
        int index;
    };
    template <class Grow> bool add_block(Grow&& grow) {
        if (!grow(cap_, (int)BLOCK)) return false;
        cap_ += BLOCK;
        return true;
    }
    std::unordered_map<unsigned long long, int> direct_;
    std::unordered_map<unsigned long long, Captured> captured_;
    int next_ = 0, cap_ = 0;
};

}  // namespace fx
