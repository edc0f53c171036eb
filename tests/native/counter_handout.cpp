// The hand-out of work counters (fiat_amd/csrc/counter_handout.hpp) against simulated streams, on the CPU.
//
// Model: a stream is a FIFO of launches; the launch at its head may be running, the ones behind it wait for it.  A launch
// uses its counter while it runs.  The hand-out requests no waits between streams, so launches are ordered only within a
// stream, and the property is: at no step of a schedule do the heads of two streams hold the same counter.  It is checked
// after every step (plan, replay, completion) of every schedule.
//
// The same schedules run against the rule this hand-out replaced (a pool of 64 counters handed to consecutive launches
// round-robin): the checker must see that rule fail wherever a launch meets the one planned 64 before it, or it proves nothing.
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <map>
#include <string>
#include <vector>

#include "../../fiat_amd/csrc/counter_handout.hpp"

namespace {

struct PerStream {  // the rule under test
    fx::CounterHandout h;
    int grows = 0, grows_in_capture = 0;
    bool capturing = false;
    PerStream() { h.reserve([this](int, int) { ++grows; return true; }); }
    int plan(int stream, unsigned long long capture) {
        capturing = capture != 0;
        return h.acquire((unsigned long long)stream, capture, [this](int first, int count) {
            if (first != h.capacity() || count != fx::CounterHandout::BLOCK) std::abort();
            ++grows;
            if (capturing) ++grows_in_capture;
            return true;
        });
    }
};

struct Modulo64 {  // the former rule: counter = launch number mod 64, whatever the stream
    unsigned seq = 0;
    int plan(int, unsigned long long) { return (int)(seq++ % 64); }
};

template <class Policy> struct Sim {
    Policy policy;
    std::map<int, std::deque<int>> streams;  // stream -> counters of its pending launches, head first
    long steps = 0, violations = 0;
    std::string first;

    void check(const char* what) {
        ++steps;
        std::map<int, int> held;  // counter -> stream whose head holds it
        for (const auto& s : streams) {
            if (s.second.empty()) continue;
            const int c = s.second.front();
            auto it = held.find(c);
            if (it != held.end()) {
                if (violations++ == 0)
                    first = std::string(what) + ": streams " + std::to_string(it->second) + " and " + std::to_string(s.first) +
                            " both run on counter " + std::to_string(c);
            } else {
                held[c] = s.first;
            }
        }
    }
    int plan_only(int stream, unsigned long long capture) {  // a captured launch: planned, not run
        const int c = policy.plan(stream, capture);
        if (c < 0) {
            std::printf("hand-out refused a launch (%d)\n", c);
            std::exit(1);
        }
        return c;
    }
    void launch(int stream) {  // a direct launch
        streams[stream].push_back(plan_only(stream, 0));
        check("launch");
    }
    void replay(int stream, int counter) {  // a graph node with its counter baked in
        streams[stream].push_back(counter);
        check("replay");
    }
    void complete(int stream) {
        streams[stream].pop_front();
        check("complete");
    }
    void drain() {
        for (auto& s : streams)
            while (!s.second.empty()) complete(s.first);
    }
};

// ---- the schedules -----------------------------------------------------------------------------------------------------
template <class S> void one_stream(S& sim) {  // 1 000 launches, the device ten behind the host
    for (int i = 0; i < 1000; ++i) {
        sim.launch(0);
        if (i >= 10) sim.complete(0);
    }
    sim.drain();
}

template <class S> void interleaved(S& sim, int nstreams) {  // evenly interleaved, every stream a few launches behind
    for (int i = 0; i < 400; ++i)
        for (int s = 0; s < nstreams; ++s) {
            sim.launch(s);
            if (i >= 3) sim.complete(s);
        }
    sim.drain();
}

template <class S> void lagging(S& sim, int lag) {  // stream 0 held back with `lag` pending launches while stream 1 runs on
    for (int i = 0; i < lag; ++i) sim.launch(0);
    for (int i = 0; i < 300; ++i) {
        sim.launch(1);
        sim.complete(1);
    }
    // the gate opens: both streams go on, stream 0 keeps its lag
    for (int i = 0; i < 300; ++i) {
        sim.launch(0);
        sim.launch(1);
        sim.complete(0);
        sim.complete(1);
    }
    sim.drain();
}

template <class S> void many_streams(S& sim) {  // 70 streams with one pending launch each, twice
    for (int round = 0; round < 2; ++round) {
        for (int s = 0; s < 70; ++s) sim.launch(s);
        for (int s = 0; s < 70; ++s) sim.complete(s);
    }
}

template <class S> void captured(S& sim, int replay_stream) {
    // a launch captured on stream 5 after a warm-up there; its counter is fixed for ever.  The graph is replayed on
    // `replay_stream` (the capture stream itself, or another) against 200 direct launches on stream 6 and further direct
    // launches on stream 5.
    sim.launch(5);
    sim.complete(5);
    const int baked = sim.plan_only(5, 1001);
    (void)sim.plan_only(5, 1001);  // the capture's second launch on that stream
    for (int i = 0; i < 200; ++i) {
        sim.replay(replay_stream, baked);
        sim.launch(6);
        if (replay_stream != 5) sim.launch(5);
        sim.complete(6);
        if (replay_stream != 5) sim.complete(5);
        sim.complete(replay_stream);
    }
    // a second capture on the same stream while the first graph is still being replayed elsewhere
    const int baked2 = sim.plan_only(5, 1002);
    sim.replay(7, baked);
    sim.replay(8, baked2);
    sim.complete(7);
    sim.complete(8);
}

struct Case {
    const char* name;
    long new_violations, old_violations;
    bool old_must_fail;
};

template <class F> Case run(const char* name, bool old_must_fail, F&& schedule) {
    Sim<PerStream> a;
    schedule(a);
    Sim<Modulo64> b;
    schedule(b);
    std::printf("%-34s per-stream: %ld violations in %ld steps%s%s | mod 64: %ld violations%s%s\n", name, a.violations, a.steps,
                a.violations ? " -- " : "", a.first.c_str(), b.violations, b.violations ? " -- first: " : "", b.first.c_str());
    if (a.policy.grows_in_capture) {
        std::printf("%s: the hand-out allocated during a capture\n", name);
        std::exit(1);
    }
    return {name, a.violations, b.violations, old_must_fail};
}

}  // namespace

int main() {
    std::vector<Case> cases;
    cases.push_back(run("one stream, 1000 launches", false, [](auto& s) { one_stream(s); }));
    cases.push_back(run("two streams interleaved", false, [](auto& s) { interleaved(s, 2); }));
    cases.push_back(run("three streams interleaved", false, [](auto& s) { interleaved(s, 3); }));
    cases.push_back(run("lag 63", false, [](auto& s) { lagging(s, 63); }));
    cases.push_back(run("lag 64", true, [](auto& s) { lagging(s, 64); }));
    cases.push_back(run("lag 65", true, [](auto& s) { lagging(s, 65); }));
    cases.push_back(run("lag 500", true, [](auto& s) { lagging(s, 500); }));
    cases.push_back(run("70 streams, one launch each", true, [](auto& s) { many_streams(s); }));
    cases.push_back(run("captured, replayed on a third stream", true, [](auto& s) { captured(s, 9); }));
    cases.push_back(run("captured, replayed on its own", true, [](auto& s) { captured(s, 5); }));
    int bad = 0;
    for (const Case& c : cases) {
        if (c.new_violations) ++bad;
        if (c.old_must_fail && !c.old_violations) {
            std::printf("%s: the checker did not see the mod-64 rule fail\n", c.name);
            ++bad;
        }
    }

    // steady state allocates nothing: a thousand launches on three known streams add no block
    {
        PerStream p;
        for (int s = 0; s < 3; ++s) p.plan(s, 0);
        const int before = p.grows;
        for (int i = 0; i < 1000; ++i) p.plan(i % 3, 0);
        if (p.grows != before) {
            std::printf("launches on known streams allocated %d blocks\n", p.grows - before);
            ++bad;
        }
    }
    // the launches one stream adds to one capture are ordered inside the graph: one counter; another stream of the same
    // capture (a fork) gets its own
    {
        PerStream p;
        const int a = p.plan(5, 77), b = p.plan(5, 77), c = p.plan(6, 77), d = p.plan(5, 78);
        if (a != b || c == a || d == a || d == c) {
            std::printf("counters within captures: %d %d %d %d\n", a, b, c, d);
            ++bad;
        }
    }
    // captures never allocate; when the spare counters are used up they are refused, and a direct launch restores the reserve
    {
        PerStream p;
        int served = 0, c = 0;
        std::map<int, int> seen;
        for (unsigned long long id = 1; id <= 100; ++id) {
            c = p.plan(3, id);
            if (c < 0) break;
            if (seen.count(c)) {
                std::printf("two captures share counter %d\n", c);
                ++bad;
            }
            seen[c] = 1;
            ++served;
        }
        if (c != fx::CounterHandout::NO_SPARE || served != fx::CounterHandout::BLOCK || p.grows_in_capture) {
            std::printf("exhausted captures: served %d, last answer %d, %d blocks allocated in capture\n", served, c, p.grows_in_capture);
            ++bad;
        }
        const int d = p.plan(3, 0);
        const int again = p.plan(3, 200);
        if (d < 0 || again < 0 || seen.count(d) || seen.count(again) || d == again || p.grows_in_capture) {
            std::printf("after the reserve was restored: direct %d, captured %d\n", d, again);
            ++bad;
        }
    }
    // an allocation failure is reported, not papered over with a counter in use
    {
        fx::CounterHandout h;
        const int r = h.acquire(1, 0, [](int, int) { return false; });
        if (r != fx::CounterHandout::GROW_FAILED) {
            std::printf("failed growth answered %d\n", r);
            ++bad;
        }
    }
    if (bad) {
        std::printf("%d failures\n", bad);
        return 1;
    }
    std::printf("hand-out ok\n");
    return 0;
}
