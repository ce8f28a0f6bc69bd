// Who owns an algorithm's engine, and for how long: the registry behind InitAlgorithm / gsc_release_algorithm / gsc_replace_algorithm
// (DESIGN.md §3.9), the micro-batcher in front of an engine, and the two as one object.  Host-only code with no HIP in it, templated on the
// engine type like dispatch.hpp: capi.cpp instantiates it with Algorithm, tests/native/registry_check.cpp with a stub engine on CPU.
//
// The rules:
//   * the registry holds one std::shared_ptr per id; an entry point takes ONE snapshot (Ref) when it enters and works on it until it leaves —
//     whatever is released or swapped in meanwhile, a call is served whole by the engine it found;
//   * the registry mutex is held to copy or swap a pointer, never across a build: callers of every id go on while one id builds;
//   * init, release and replace of one id serialise on that id's lifecycle mutex;
//   * an engine leaves in three steps: out of the registry (new calls no longer see it), drained (every call that holds a snapshot of it has
//     left, the callers parked in its micro-batcher served), then destroyed by the thread that retired it — never by a caller's thread.
#pragma once
#include "dispatch.hpp"
#include "engine.hpp"
#include <condition_variable>
#include <cstdlib>
#include <deque>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

namespace gsc {

// Micro-batching: concurrent single-proof Prove() callers (the reference is called from many goroutines / FFI threads:
// libraries/core_test.go:44-111) are gathered into ONE device batch instead of running one proof each, back to back.
// Worker threads — one per (device, lane) of the algorithm's engine — drain the queue; WHEN a worker takes HOW MANY callers is
// csrc/dispatch.hpp's BatchScheduler (tested on CPU with a stub engine): a lone caller on an idle device goes at once; while every
// device has a batch on it the callers that arrive form the next one; the callers of a batch that has just completed are waited for
// as long as they keep coming back (GSC_LINGER_US, default 300 us, sets the windows; 0 = never wait on an idle device); a burst is
// shared out over the free devices and every share goes out as one device batch to the least-loaded engine replica.
// Engine: prove_batch(const ProofRequest*, size_t, ProofResult*, DebugVectors*, bool whole), devices(), max_batch(), lanes().
template <class Engine>
class Batcher {
  public:
    explicit Batcher(Engine* a) : algo_(a), sched_(a->devices() ? a->devices() : 1, a->max_batch(), linger_from_env()) {
        // one worker per (device, lane): a second batch per device is started when enough callers are queued for it (dispatch.hpp)
        const size_t nw = (a->lanes() ? a->lanes() : 1) * (a->devices() ? a->devices() : 1);
        for (size_t i = 0; i < nw; i++) workers_.emplace_back([this] { run(); });
    }
    // the callers still queued are served before the workers leave (wait_for_batch hands out what is queued after `stop`)
    ~Batcher() { { std::lock_guard<std::mutex> l(mu_); stop_ = true; } sched_.cv.notify_all(); for (auto& w : workers_) if (w.joinable()) w.join(); }
    // blocks until the proof is done; throws std::runtime_error if the device batch failed
    void submit(const ProofRequest& req, ProofResult& out) {
        Item it{&req, &out, false, std::string(), &it};
        { std::unique_lock<std::mutex> l(mu_); q_.push_back(&it); sched_.arrived(); done_cv_.wait(l, [&] { return it.done; }); }
        if (!it.error.empty()) throw std::runtime_error(it.error);
    }
    // A small call of several statements (ProveBatch / gsc_prove_raw with up to SMALL_CALL statements): its statements queue like single
    // callers, so concurrent small calls share device batches whatever entry point they came through.
    static constexpr size_t SMALL_CALL = 32;
    void submit_many(const ProofRequest* reqs, size_t n, ProofResult* out) {
        std::vector<Item> items(n);
        {
            std::unique_lock<std::mutex> l(mu_);
            for (size_t i = 0; i < n; i++) { items[i] = Item{&reqs[i], &out[i], false, std::string(), items.data()}; q_.push_back(&items[i]); }
            sched_.arrived(n);
            done_cv_.wait(l, [&] { for (const Item& it : items) if (!it.done) return false; return true; });
        }
        for (const Item& it : items) if (!it.error.empty()) throw std::runtime_error(it.error);
    }
  private:
    struct Item { const ProofRequest* req; ProofResult* res; bool done; std::string error; const void* call; };      // call: the same for all statements of one submit_many
    static int linger_from_env() { const char* e = getenv("GSC_LINGER_US"); return e && *e ? atoi(e) : 300; }
    void run() {
        for (;;) {
            std::vector<Item*> take;
            {
                std::unique_lock<std::mutex> l(mu_);
                const size_t want = sched_.wait_for_batch(l, [&] { return q_.size(); }, stop_);
                if (!want) return;                         // stopped, nothing queued
                while (!q_.empty() && take.size() < want) { take.push_back(q_.front()); q_.pop_front(); }
                sched_.started(take.size());
            }
            // Whatever happens below — a device error, an allocation failure, anything thrown — the callers parked on done_cv_ are released
            // and the scheduler hears of the completion: nobody is left waiting on a batch that died.
            std::string err; std::vector<ProofResult> res;
            try {
                std::vector<ProofRequest> reqs(take.size()); res.resize(take.size());
                for (size_t i = 0; i < take.size(); i++) reqs[i] = *take[i]->req;
                algo_->prove_batch(reqs.data(), reqs.size(), res.data(), nullptr, true);      // whole: one device batch on ONE replica (plan_shares)
            } catch (const std::exception& e) { err = e.what(); if (err.empty()) err = "proving failed"; }
            catch (...) { err = "proving failed (unknown error)"; }
            {
                std::lock_guard<std::mutex> l(mu_);
                for (size_t i = 0; i < take.size(); i++) { if (err.empty() && i < res.size()) *take[i]->res = res[i]; take[i]->error = err; take[i]->done = true; }
                size_t calls = 0; const void* prev = nullptr;      // (the statements of a call are queued back to back)
                for (Item* it : take) { if (it->call != prev) calls++; prev = it->call; }
                sched_.completed(take.size(), calls);
            }
            done_cv_.notify_all();
        }
    }
    Engine* algo_; BatchScheduler sched_; bool stop_ = false;
    std::mutex mu_; std::condition_variable done_cv_; std::deque<Item*> q_; std::vector<std::thread> workers_;
};

// What the registry serves under an id: the engine, the micro-batcher in front of it, and the name of the key it was built from.
template <class Engine>
struct Served {
    std::unique_ptr<Engine> algo;
    std::string key_id;                               // first 16 hex digits of SHA-256 of the proving key's bytes (gsc_describe)
    std::unique_ptr<Batcher<Engine>> batcher;         // declared after algo: destroyed first
    Served(std::unique_ptr<Engine> a, std::string key) : algo(std::move(a)), key_id(std::move(key)), batcher(new Batcher<Engine>(algo.get())) {}
};

template <class S, size_t N = 3>
class Registry {
    // one served object and the calls that hold a snapshot of it
    struct Live {
        std::unique_ptr<S> s; uint64_t gen = 0;
        std::mutex mu; std::condition_variable cv; size_t users = 0;
        void leave() { std::lock_guard<std::mutex> l(mu); if (--users == 0) cv.notify_all(); }
        void drain() { std::unique_lock<std::mutex> l(mu); cv.wait(l, [&] { return users == 0; }); }
    };
  public:
    // One call's snapshot: empty (the id is not initialised) or the served object, which stays whole until the Ref is gone.
    class Ref {
      public:
        Ref() = default;
        Ref(Ref&& o) noexcept : live_(std::move(o.live_)) {}
        Ref& operator=(Ref&& o) noexcept { if (this != &o) { reset(); live_ = std::move(o.live_); } return *this; }
        Ref(const Ref&) = delete; Ref& operator=(const Ref&) = delete;
        ~Ref() { reset(); }
        explicit operator bool() const { return (bool)live_; }
        S* operator->() const { return live_->s.get(); }
        S& operator*() const { return *live_->s; }
        uint64_t generation() const { return live_ ? live_->gen : 0; }
        void reset() { if (live_) { live_->leave(); live_.reset(); } }
      private:
        friend class Registry;
        explicit Ref(std::shared_ptr<Live> l) : live_(std::move(l)) {}
        std::shared_ptr<Live> live_;
    };

    Ref snapshot(size_t id) {
        if (id >= N) return Ref();
        std::lock_guard<std::mutex> l(mu_);
        std::shared_ptr<Live> live = slot_[id];
        if (!live) return Ref();
        { std::lock_guard<std::mutex> u(live->mu); live->users++; }      // under mu_: a retiring thread that swapped the slot sees every user that saw the old pointer
        return Ref(std::move(live));
    }
    // 0 while not initialised; 1 after init; +1 per replace; 0 again after a release
    uint64_t generation(size_t id) {
        if (id >= N) return 0;
        std::lock_guard<std::mutex> l(mu_);
        return slot_[id] ? slot_[id]->gen : 0;
    }

    // build() -> std::unique_ptr<S>, called only when the id is not initialised, outside the registry mutex; what it throws goes to the caller
    // and leaves the id as it was.  false: the id was initialised already (build never ran); true: build's object serves, generation 1.
    template <class Build>
    bool init(size_t id, Build build) {
        std::lock_guard<std::mutex> life(life_[id]);
        { std::lock_guard<std::mutex> l(mu_); if (slot_[id]) return false; }
        auto live = std::make_shared<Live>();
        live->s = build(); live->gen = 1;
        std::lock_guard<std::mutex> l(mu_);
        slot_[id] = std::move(live);
        return true;
    }
    // Takes the id out (from that instant snapshots are empty), waits for every call that had entered, runs retire(S&) on the idle object and
    // destroys it.  false: the id was not initialised.
    template <class Retire>
    bool release(size_t id, Retire retire) {
        if (id >= N) return false;
        std::lock_guard<std::mutex> life(life_[id]);
        std::shared_ptr<Live> old;
        { std::lock_guard<std::mutex> l(mu_); old.swap(slot_[id]); }
        if (!old) return false;
        finish(*old, retire);
        return true;
    }
    // build(const S& serving) -> std::unique_ptr<S> beside the serving object, outside the registry mutex; what it throws goes to the caller, the
    // serving object has served throughout and keeps serving, the generation does not move.  Then the swap (generation + 1), and the old object
    // leaves as in release.  -1: the id is not initialised; 1: swapped.
    template <class Build, class Retire>
    int replace(size_t id, Build build, Retire retire) {
        if (id >= N) return -1;
        std::lock_guard<std::mutex> life(life_[id]);
        std::shared_ptr<Live> old;
        { std::lock_guard<std::mutex> l(mu_); old = slot_[id]; }
        if (!old) return -1;
        auto live = std::make_shared<Live>();
        live->s = build(static_cast<const S&>(*old->s)); live->gen = old->gen + 1;      // old->s: only the lifecycle mutex's holder ever resets it
        { std::lock_guard<std::mutex> l(mu_); slot_[id] = std::move(live); }
        finish(*old, retire);
        return 1;
    }
  private:
    template <class Retire>
    static void finish(Live& old, Retire& retire) {
        old.drain();
        retire(*old.s);
        old.s.reset();
    }
    std::mutex mu_;                       // the slots; held to copy or swap a pointer only
    std::mutex life_[N];                  // init / release / replace of one id, for their whole duration
    std::shared_ptr<Live> slot_[N];
};

}  // namespace gsc
