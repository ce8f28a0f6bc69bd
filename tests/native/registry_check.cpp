// CPU check of csrc/registry.hpp with a stub engine (no HIP): the ownership rules behind InitAlgorithm / gsc_release_algorithm /
// gsc_replace_algorithm.  The stub "proves" by sleeping and stamps its key into the result; its destructor poisons it, and prove_batch aborts
// on a poisoned object — a call that outlives its engine ends the program.  Built and run by tests/test_registry_host.py, once plainly and once
// with -fsanitize=thread; prints one line per check and REGISTRY-OK at the end.
#if defined(__SANITIZE_THREAD__) && defined(__GNUC__) && !defined(__clang__)
// The -fsanitize=thread build only: libstdc++ waits on the steady clock with pthread_cond_clockwait, which older ThreadSanitizer runtimes do
// not intercept — they then believe the mutex stayed locked over the wait and report every later lock of it.  Without the macro the timed
// waits of dispatch.hpp go through pthread_cond_timedwait, which every runtime knows; the code under test is the same.
#include <bits/c++config.h>
#undef _GLIBCXX_USE_PTHREAD_COND_CLOCKWAIT
#endif
#include "../../gnark-symmetric-crypto_amd/csrc/registry.hpp"
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <thread>

using namespace gsc;

#define CHECK(c) do { if (!(c)) { printf("FAILED %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

static std::atomic<int> g_alive{0}, g_max_alive{0}, g_built{0};

struct StubEngine {
    static constexpr uint32_t LIVE = 0xA11FE5u, DEAD = 0xDEADDEADu;
    volatile uint32_t magic = LIVE; const int key; const int batch_us;
    StubEngine(int k, int us) : key(k), batch_us(us) { const int n = ++g_alive; int m = g_max_alive.load(); while (n > m && !g_max_alive.compare_exchange_weak(m, n)) {} g_built++; }
    ~StubEngine() { magic = DEAD; g_alive--; }
    void prove_batch(const ProofRequest*, size_t n, ProofResult* res, DebugVectors*, bool) {
        if (magic != LIVE) { printf("FAILED prove_batch on a destroyed engine\n"); fflush(stdout); abort(); }
        std::this_thread::sleep_for(std::chrono::microseconds(batch_us));
        if (magic != LIVE) { printf("FAILED engine destroyed under a running batch\n"); fflush(stdout); abort(); }
        for (size_t i = 0; i < n; i++) { res[i].status = 0; res[i].proof[0] = (uint8_t)key; res[i].proof_len = 1; }
    }
    size_t devices() const { return 1; }
    size_t max_batch() const { return 64; }
    size_t lanes() const { return 2; }
};
using StubServed = Served<StubEngine>;
using Reg = Registry<StubServed>;

static std::unique_ptr<StubServed> make(int key, int us) { return std::unique_ptr<StubServed>(new StubServed(std::unique_ptr<StubEngine>(new StubEngine(key, us)), "key" + std::to_string(key))); }
static void sleep_ms(int ms) { std::this_thread::sleep_for(std::chrono::milliseconds(ms)); }
static auto no_retire = [](StubServed&) {};

// one call as capi.cpp makes it: a snapshot at entry, the proof through the micro-batcher (direct = false) or straight on the engine.
// Returns the key that served it, 0 for "not initialised".
// served (optional) counts the call as through BEFORE its snapshot is given back: a release that has drained the engine has seen every such count.
static int call(Reg& reg, size_t id, bool direct, std::atomic<int>* entered = nullptr, std::atomic<int>* served = nullptr) {
    Reg::Ref snap = reg.snapshot(id);
    if (entered) (*entered)++;
    if (!snap) return 0;
    ProofRequest req{}; ProofResult res;
    if (direct) snap->algo->prove_batch(&req, 1, &res, nullptr, false);
    else snap->batcher->submit(req, res);
    if (served) (*served)++;
    return res.proof[0];
}

int main() {
    {   // release waits for the calls in flight and for the callers parked in the micro-batcher; all of them are served by the old engine
        Reg reg;
        CHECK(reg.init(0, [] { return make(1, 60000); }) && reg.generation(0) == 1);
        std::atomic<int> entered{0}, done{0}, wrong{0};
        std::vector<std::thread> th;
        // 2 straight on the engine, 6 through the batcher: its two workers take a batch each, the callers that arrive under them stay parked
        for (int i = 0; i < 8; i++) th.emplace_back([&, i] { if (call(reg, 0, i < 2, &entered, &done) != 1) wrong++; });
        while (entered.load() < 8) sleep_ms(1);
        sleep_ms(5);
        int done_at_retire = -1;
        CHECK(reg.release(0, [&](StubServed&) { done_at_retire = done.load(); }));
        const int done_at_return = done.load(), alive_at_return = g_alive.load();
        for (auto& t : th) t.join();
        printf("release under 8 calls: %d through when the idle engine was handed over, %d when release returned\n", done_at_retire, done_at_return);
        CHECK(done_at_retire == 8 && done_at_return == 8 && wrong.load() == 0 && alive_at_return == 0);
        CHECK(reg.generation(0) == 0 && !reg.snapshot(0) && call(reg, 0, false) == 0);
        CHECK(!reg.release(0, no_retire));                                  // a second release: nothing there
        CHECK(reg.init(0, [] { return make(1, 100); }) && reg.generation(0) == 1 && call(reg, 0, false) == 1);      // as on a fresh registry
        CHECK(reg.release(0, no_retire) && g_alive.load() == 0);
    }
    {   // a call that entered before a swap finishes on the old engine; one that entered after it runs on the new one, while the old one still drains
        Reg reg;
        CHECK(reg.init(1, [] { return make(1, 150000); }));
        std::atomic<int> entered{0}; int got_a = -1, got_b = -1; std::atomic<bool> a_done{false}, replace_done{false}; bool b_before_replace_returned = false;
        std::thread a([&] { got_a = call(reg, 1, false, &entered); a_done = true; });
        while (entered.load() < 1) sleep_ms(1);
        std::thread b([&] { while (reg.generation(1) != 2) sleep_ms(1); got_b = call(reg, 1, true); b_before_replace_returned = !replace_done.load(); });
        bool a_done_at_retire = false;
        CHECK(reg.replace(1, [](const StubServed& old) { return make(old.algo->key + 1, 1000); }, [&](StubServed& s) { a_done_at_retire = a_done.load() && s.algo->key == 1; }) == 1);
        replace_done = true;
        const int alive = g_alive.load();
        a.join(); b.join();
        printf("swap: the call before it got key %d, the call after it key %d (%s the old engine had drained)\n", got_a, got_b, b_before_replace_returned ? "before" : "after");
        CHECK(got_a == 1 && got_b == 2 && a_done_at_retire && alive == 1 && b_before_replace_returned && reg.generation(1) == 2);
        // a build that throws: the old engine serves on, the generation does not move, nothing of the attempt is left
        const int built = g_built.load();
        bool threw = false;
        try { reg.replace(1, [](const StubServed&) -> std::unique_ptr<StubServed> { auto half = make(9, 10); throw std::runtime_error("pk: refused"); }, no_retire); }
        catch (const std::runtime_error&) { threw = true; }
        CHECK(threw && g_built.load() == built + 1 && g_alive.load() == 1 && reg.generation(1) == 2 && call(reg, 1, false) == 2);
        // ... and so for init on an empty id, and replace of an empty id never builds
        threw = false;
        try { reg.init(2, []() -> std::unique_ptr<StubServed> { throw std::runtime_error("r1cs: refused"); }); } catch (const std::runtime_error&) { threw = true; }
        CHECK(threw && reg.generation(2) == 0 && !reg.snapshot(2));
        CHECK(reg.replace(2, [](const StubServed&) { return make(5, 10); }, no_retire) == -1 && g_built.load() == built + 1);
        CHECK(reg.init(2, [] { return make(5, 10); }) && call(reg, 2, true) == 5);      // the lifecycle mutex was given back by the throwing calls
        CHECK(reg.release(1, no_retire) && reg.release(2, no_retire) && g_alive.load() == 0);
        printf("a refused build leaves the old engine serving\n");
    }
    {   // other ids stay reachable while one id builds; two concurrent inits of one id end with one engine
        Reg reg;
        CHECK(reg.init(0, [] { return make(1, 100); }));
        std::atomic<bool> building{false}, built{false}; std::atomic<int> builds{0}, inits_true{0};
        auto slow = [&] { builds++; building = true; sleep_ms(200); built = true; return make(7, 100); };
        std::thread t1([&] { if (reg.init(1, slow)) inits_true++; }), t2([&] { if (reg.init(1, slow)) inits_true++; });
        while (!building.load()) sleep_ms(1);
        int lookups = 0; double worst_ms = 0;
        while (!built.load() && lookups < 100) {
            const auto t0 = std::chrono::steady_clock::now();
            const bool ok = call(reg, 0, true) == 1 && !reg.snapshot(1) && reg.generation(1) == 0 && reg.generation(0) == 1;
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (!ok) { printf("FAILED lookup %d beside the build\n", lookups); return 1; }
            worst_ms = ms > worst_ms ? ms : worst_ms; lookups++;
        }
        const bool still_building = !built.load();
        t1.join(); t2.join();
        printf("beside a 200 ms build: %d calls of another id, the slowest %.2f ms\n", lookups, worst_ms);
        CHECK(lookups == 100 && still_building && worst_ms < 100);
        CHECK(builds.load() == 1 && inits_true.load() == 1 && reg.generation(1) == 1 && call(reg, 1, false) == 7 && g_alive.load() == 2);
        CHECK(reg.release(0, no_retire) && reg.release(1, no_retire) && g_alive.load() == 0);
    }
    {   // concurrent init, release and replace of one id beside callers: they serialise (never more than the serving engine and one being built),
        // every call is served by a key that existed or told "not initialised", and the end state is consistent
        Reg reg;
        g_max_alive = 0;
        std::atomic<bool> stop{false}; std::atomic<int> bad{0}, served{0}, refused{0}, next_key{1};
        std::vector<std::thread> callers, ops;
        for (int i = 0; i < 4; i++) callers.emplace_back([&, i] { while (!stop.load()) { const int k = call(reg, 0, i & 1); if (k == 0) refused++; else if (k > 0 && k < next_key.load()) served++; else bad++; } });
        for (int i = 0; i < 3; i++) ops.emplace_back([&, i] {
            std::mt19937 rnd(1234 + i);
            for (int k = 0; k < 60; k++) {
                switch (rnd() % 3) {
                    case 0: reg.init(0, [&] { return make(next_key++, 300); }); break;
                    case 1: reg.release(0, no_retire); break;
                    default: { const int r = reg.replace(0, [&](const StubServed&) { return make(next_key++, 300); }, no_retire); if (r != 1 && r != -1) bad++; }
                }
            }
        });
        for (auto& t : ops) t.join();
        stop = true;
        for (auto& t : callers) t.join();
        const bool there = (bool)reg.snapshot(0);
        printf("180 lifecycle operations beside 4 callers: %d calls served, %d told not initialised, at most %d engines alive, end state %s\n", served.load(), refused.load(), g_max_alive.load(), there ? "initialised" : "empty");
        CHECK(bad.load() == 0 && served.load() > 0 && g_max_alive.load() <= 2);
        CHECK(g_alive.load() == (there ? 1 : 0) && (reg.generation(0) != 0) == there);
        reg.release(0, no_retire);
        CHECK(g_alive.load() == 0 && reg.generation(0) == 0);
    }
    printf("REGISTRY-OK\n");
    return 0;
}
