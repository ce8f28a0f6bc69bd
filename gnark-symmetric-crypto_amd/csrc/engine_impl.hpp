// The engine behind one algorithm on one device: key tables (engine_tables.hip), the per-batch device pipeline (engine_prove.hip;
// its routing policy: chunk_route.hpp) and the lanes that carry batches.  Internal to the library: engine.hpp is the interface capi.cpp sees; engine.hip holds the replica
// dispatch (Algorithm).  Reference counterpart: the per-cipher prover objects of libraries/prover/impl/provers.go:61-77
// (baseProver{r1cs, pk}: SetParams -> tables, Prove -> pipeline).
#pragma once
#include "engine.hpp"
#include "chunk_route.hpp"
#include "formats.hpp"
#include "kernels.hpp"
#include "wit_small.hpp"
#include "solver_tables.hpp"
#include "msm_set.hpp"
#include "wipe_plan.hpp"
#include "prove_check.hpp"
#include <atomic>
#include <chrono>
#include <cstring>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

namespace gsc {

// page-locked host memory: the staging buffers of a lane (uploads and downloads are then real asynchronous DMA, not driver-staged copies)
template <class T>
struct PinnedBuf {
    T* p = nullptr; size_t n = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete; PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf() { if (p) (void)hipHostFree(p); }
    void alloc(size_t count) { if (p) { (void)hipHostFree(p); p = nullptr; } n = count; if (count) { HIP_CHECK(hipHostMalloc((void**)&p, count * sizeof(T), hipHostMallocDefault)); memset(p, 0, count * sizeof(T)); } }
    size_t bytes() const { return n * sizeof(T); }
};

// Encoded points of a key as the walk of formats.hpp leaves them: x at a fixed stride (32 B in G1, 64 B in G2, flag bits in place) and,
// when some element is raw, y at the same stride (the Y bytes of the raw elements; empty for a compressed-only set).
struct KeyPoints {
    std::vector<uint8_t> x, y;
    KeyPoints() = default;
    KeyPoints(const std::vector<uint8_t>& x_, const std::vector<uint8_t>& y_ = {}) : x(x_), y(y_) {}
};
// The production decode of a key's points, on `stream` (synchronised before returning): the compressed elements by k_decompress_*, the raw
// ones by k_decode_raw_* (only launched when there are any), and for G2 the subgroup test over every finite point.  out: device memory for
// x.size() / stride points; returns one status byte per point (0 decoded, 1 refused, 2 the point at infinity).  No key, no engine needed.
std::vector<uint8_t> decode_g1_points(const KeyPoints& pts, G1Aff* out, hipStream_t stream);
std::vector<uint8_t> decode_g2_points(const KeyPoints& pts, G2Aff* out, hipStream_t stream);

// (one MSM set of the key, its tables and the launch sequence of a call over it: MsmSet, msm_build_tables, msm_run — msm_set.hpp)

// The engines' streams come from a process-wide pool and go back to it, drained, when an engine goes: the HIP runtime binds a stream to one of
// its hardware queues when the stream is created, and a queue keeps the scratch memory its kernels needed for the life of the process.  An
// engine built after a release on NEW streams lands on other queues, and the process grows by their scratch (measured once per queue: 632 MiB at
// the next init, 250 MiB at its first call) — on the streams of the engine before it, it does not.  A stream is pooled under
// (device, kind, role): kind = its priority level or STREAM_PLAIN (hipStreamCreate), role = what it does in the engine (STREAM_ROLE_INIT, or
// 3 * lane + 0 / 1 / 2 for a lane's main / side / third stream), so that a queue sees the kernels it has seen.  Pooled streams are never destroyed.
constexpr int STREAM_PLAIN = 1 << 30, STREAM_ROLE_INIT = -1;
hipStream_t stream_take(int device, int kind, int role);            // the device is current; throws on a HIP error
void stream_give(int device, int kind, int role, hipStream_t s);    // waits for the stream's work first

// bytes the complete prover replicas on a device hold (AlgorithmImpl::accounted; gsc_memory_info): engine_tables.hip
std::atomic<size_t>& prover_bytes_on(int device);

// (the solver's tables — program, schedule, coefficients, the small-integer program — and the circuit's sizes: SolverTables, solver_tables.hpp)
class AlgorithmImpl : public SolverTables {
  public:
    Cipher cipher; EngineConfig cfg;
    size_t domain_n = 0; int L = 0;
    // lanes are handed out one chunk at a time; concurrent calls (and the chunks of one call) take whichever lane is free
    std::mutex pool_mu; std::condition_variable pool_cv; std::vector<uint8_t> lane_busy;
    // a free lane that can hold n statements — the smallest such lane, so that small calls leave the full-capacity lanes to big ones
    size_t acquire_lane(int want = -1, size_t n = 0) {
        std::unique_lock<std::mutex> l(pool_mu);
        size_t got = 0;
        pool_cv.wait(l, [&] {
            bool found = false;
            for (size_t i = 0; i < lane_busy.size(); i++) {
                if (lane_busy[i] || (want >= 0 && (size_t)want != i) || lanes[i]->cap < n) continue;
                if (!found || lanes[i]->cap < lanes[got]->cap) { got = i; found = true; }
            }
            return found;
        });
        lane_busy[got] = 1;
        return got;
    }
    std::atomic<int> calls_in_flight{0};
    int cu_count = 256;                 // compute units of the device: the resident witness kernel needs one per workgroup
    // After a resident launch gave up (CUs held by someone else), the next few_skip calls of this replica go level by level at once
    // instead of spinning through the same timeouts; the penalty doubles up to 4096 calls and is forgotten after a success.
    std::atomic<uint32_t> few_skip{0}; std::atomic<uint32_t> few_penalty{16};
    std::mutex stat_mu; KernelStat last_stat;      // timing of the chunk that finished last on this replica
    // The self-check (prove_check.hpp): this replica's context, or none while the check is off.  A chunk takes the pointer when it starts and is
    // checked under that key, whatever is loaded meanwhile; the context's buffers are no part of any lane (public data only, never wiped).
    std::mutex check_mu; std::shared_ptr<ProveCheckCtx> check;
    std::shared_ptr<ProveCheckCtx> check_now() { std::lock_guard<std::mutex> l(check_mu); return check; }
    // TEST HOOK: the one-shot change gsc_debug_prove_corrupt armed (Algorithm's word: 1 << 63 | mode << 40 | which << 32 | index; 0: none)
    std::atomic<uint64_t>* corrupt = nullptr;
    void release_lane(size_t i) { { std::lock_guard<std::mutex> l(pool_mu); lane_busy[i] = 0; } pool_cv.notify_all(); }
    hipStream_t stream = nullptr;   // init-time work; proving runs on the lanes' streams
    size_t table_bytes = 0;
    std::vector<uint8_t> row_class;    // per scalar row (wire), predicted by calibrate(): 0 = always 0 or 1, 1 = also -1, else the largest bit length seen (255 = unknown)

    std::vector<uint8_t> row_class_a, row_class_b;      // the calibration classes of the rows of a and b (the small-integer path's byte planes)
    void init_small(const SolverProgram& sp);
    std::atomic<uint64_t> small_fallbacks{0};      // chunks that had to be solved again generically (gsc_describe)
    // NTT
    DevBuf<int32_t> tw_fwd, tw_inv, tw_inv_plain, qr; DevBuf<fe> scale_mid, scale_mid_plain, scale_out, dom;   // dom: omega, omega_inv, g, g_inv, n_inv, 16/n
    // MSM sets
    MsmSet<G1Aff> mA, mB1, mK, mZ, mZfew, mPed, mPedSigma; MsmSet<G2Aff> mB2;     // mPed*: Pedersen commitment bases (AES-V2)
    // Evaluation-form quotient (k_quot_bases.hip, cfg.quotient_eval): mZ then holds the bases V_i (scalars: d on the zeta-coset, launch_compute_d)
    // and mC the bases U_i of the constraint rows (scalars: the solver's c, laid out like a wire set from row_class_c); calls that take the
    // latency layout mZfew keep the coefficient form (it holds the key's own Z).
    bool quotient_eval = false; MsmSet<G1Aff> mC; std::vector<uint8_t> row_class_c;
    // ... and the last quotient kernel writes the digits of d itself (launch_compute_d_digits): mZ's table positions follow quot_digit_index,
    // whole batches skip the recoding pass; the other sets recode into a (small) digit buffer of their own meanwhile (Lane::d_digits_w)
    bool fuse_z_digits = false;
    // The fold (k_quot_bases.hip): with m constraints on a domain of n only m - 1 of the d_i are independent of c; the bases of the others went into U and V
    // (U', V': valid only as a pair — mC and mZ are both folded or neither), mZ walks m - 1 bases.  fold_why: why not, for gsc_describe.
    std::string fold_why = "GSC_QUOTIENT_FOLD=0";
    // ... and the evaluation-form quotient computes d for the live table positions only (launch_compute_d*'s live; cfg.quotient_live_tiles).  0: for all n —
    // the sets are not folded, or the knob is off
    size_t quot_live = 0;
    // U' and V' (table order, m and m - 1 points) from U and V; false (and fold_why) when a folded V base is the point at infinity
    bool fold_quotient_bases(const DevBuf<G1Aff>& d_U, const std::vector<uint8_t>& stU, const DevBuf<G1Aff>& d_V, const std::vector<uint8_t>& stV, const std::vector<uint32_t>& rowsZ,
                             DevBuf<G1Aff>& d_U2, std::vector<uint8_t>& stU2, DevBuf<G1Aff>& d_V2, std::vector<uint8_t>& stV2);
    // batch buffers: one set per lane.  A lane = a HIP stream with its own witness / polynomial / partial-sum buffers; with more than
    // one full lane big batches are cut into chunks that the lanes prove concurrently.  Measured on MI355X: for FULL
    // batches two lanes do not beat one (the MSM kernels fill the chip; chaining the heavy phases so that only the witness stage
    // overlaps was measured in round 3: no gain either), so ChaCha20-V3 has one full lane; calls of a few dozen to a few hundred
    // statements under-fill the chip and do gain from running side by side: the small lanes.
    struct Lane {
        hipStream_t stream = nullptr, side = nullptr, side2 = nullptr;      // side: the assembly's scalar multiplications, beside the MSMs; side2: the B2 sum of a latency-path call
        hipEvent_t ev_ab = nullptr, ev_fs = nullptr, ev_b2 = nullptr, ev_s2 = nullptr;
        hipEvent_t ev_ws = nullptr;     // the wire-set MSMs of a call whose quotient runs beside them are through (stage accounting)
        hipEvent_t ev_wa = nullptr, ev_wa_done = nullptr;      // phase A of the wipe may start (main stream) / is through (third stream)
        hipEvent_t ev_few = nullptr;    // completion of this lane's latest k_solver_few launch (FewSolverChain)
        hipEvent_t ev[7] = {};          // 0..4 stage boundaries, 5..6 bracket the dominant kernel (Z-table MSM gather-accumulate)
        float stage_ms[4] = {0, 0, 0, 0}; float msm_z_kernel_ms = 0; size_t last_batch = 0;
        // pinned staging: inputs / randomness / masks up, proof coordinates / flags / status / commitment points and the small result words down
        PinnedBuf<uint8_t> h_in, h_rs, h_mask, h_out, h_flags, h_cpts; PinnedBuf<uint32_t> h_status; PinnedBuf<GlvSplit> h_glv; PinnedBuf<unsigned long long> h_words;
        // the small result words: [0] the resident solver's two sync words, [1] the small-integer path's flag, [2 .. 46) clock stamps
        uint32_t* h_fsync() const { return reinterpret_cast<uint32_t*>(h_words.p); }
        uint32_t& h_wsflag() const { return *reinterpret_cast<uint32_t*>(h_words.p + 1); }
        unsigned long long* h_clk() const { return h_words.p + 2; }
        KernelStat stat;                // of the chunk this lane proved last
        DevBuf<unsigned long long> d_clk;      // clock stamps: [0, 32) eight waves of the Z kernel (MsmWinArgs::clk); [32, 44) the three transform kernels (GSC_TRACE_HOST)
        size_t n_real = 0;              // statements of the chunk being proved (the batch is padded to a multiple of 64)
        size_t cap = 0;
        DevBuf<uint8_t> d_inputs, d_rs, d_out, d_flags, d_mask_in, d_cpts; DevBuf<uint32_t> d_status, d_fsync; DevBuf<GlvSplit> d_glv;
        DevBuf<fe> d_mask, d_commit; DevBuf<G1Xyzz> d_sumD, d_sumPok;
        DevBuf<fe> d_W, d_A, d_B, d_C;
        bool small_active = false;      // the chunk being proved left W, A, B, C as byte planes (the 32-byte matrices then only hold the rows marked wide)
        DevBuf<int8_t> d_W8, d_A8, d_B8, d_C8; DevBuf<uint32_t> d_wsflag;      // byte planes of the small-integer witness path; its "a prediction failed" flag
        DevBuf<G1Xyzz> d_part1a, d_part1b, d_sumA, d_sumB1, d_sumK, d_sumZ, d_sumC, d_tmp; DevBuf<G2Xyzz> d_part2a, d_part2b, d_sumB2;
        DevBuf<uint4> d_digits_s2; DevBuf<uint8_t> d_gok_s2;                                        // side2's digits (its partial sums are the G2 buffers, which nothing else uses)
        DevBuf<uint4> d_digits_s; DevBuf<uint8_t> d_gok_s; DevBuf<G1Xyzz> d_part1c, d_part1d;      // the side stream's MSM scratch (A and B1 of a latency-path call)
        DevBuf<uint4> d_digits;                                                   // signed digits [window][octet][proof]
        DevBuf<uint4> d_digits_w;      // fuse_z_digits: the digits of every set but Z (Z's are written by the last quotient kernel into d_digits and must survive until its sum runs)
        // per-window sums [window][proof] and flat-part sums [proof], one pair per set: the Horner passes of several sets are deferred
        // and run as one launch (MsmHornerJobs), so their inputs must not share storage
        static constexpr int NSETS = 8;      // A, B1, K, Z, Ped, PedSigma, Z (latency layout), C (evaluation-form quotient)
        DevBuf<G1Xyzz> d_sj1[NSETS], d_flat1[NSETS]; DevBuf<G2Xyzz> d_sj2, d_flat2;
        MsmHornerJobs pending1{}, pending2{};
        DevBuf<uint8_t> d_gok;                                                    // bit-group verdicts [group][wave of 64 proofs]
        // The region table (wipe_plan.hpp): every device allocation above, by name, as alloc_lane made it; allocated = what the DevBufs really took
        struct Region { int region; uint8_t* p; size_t bytes; };
        std::vector<Region> regions; size_t allocated = 0;
        template <class T> void reg(int region, DevBuf<T>& b) { if (b.p) regions.push_back(Region{region, reinterpret_cast<uint8_t*>(b.p), b.bytes()}); }
        // what the scratch buffers need for a chunk of 64 (k + 1) columns, in bytes (alloc_lane sized them by the largest; a chunk writes no further than its own)
        struct ScratchNeed { size_t part1a = 0, part1b = 0, part2a = 0, part2b = 0, digits = 0, digits_w = 0, gok = 0, sj1[8] = {0, 0, 0, 0, 0, 0, 0, 0}, sj2 = 0; };
        std::vector<ScratchNeed> need_at;
        bool wipe_a_pending = false;    // phase A of the chunk being proved is enqueued: phase B waits for it
        ~Lane() { if (ev_few) { for (int d = 0; d < 64; d++) { FewSolverChain& c = few_solver_chain(d); std::lock_guard<std::mutex> lk(c.m); if (c.last == ev_few) c.last = nullptr; } (void)hipEventDestroy(ev_few); }
                  for (auto& e : ev) if (e) (void)hipEventDestroy(e); if (ev_ws) (void)hipEventDestroy(ev_ws); if (ev_wa) (void)hipEventDestroy(ev_wa); if (ev_wa_done) (void)hipEventDestroy(ev_wa_done); if (ev_ab) (void)hipEventDestroy(ev_ab); if (ev_fs) (void)hipEventDestroy(ev_fs); if (ev_b2) (void)hipEventDestroy(ev_b2); if (ev_s2) (void)hipEventDestroy(ev_s2); if (side2) stream_give(device, kind[2], 3 * index + 2, side2); if (side) stream_give(device, kind[1], 3 * index + 1, side); if (stream) stream_give(device, kind[0], 3 * index, stream); }
        int device = 0, index = 0, kind[3] = {STREAM_PLAIN, STREAM_PLAIN, STREAM_PLAIN};      // where the three streams go back to (stream_give)
    };
    std::vector<std::unique_ptr<Lane>> lanes;
    size_t cap = 0;                     // proofs per full lane = the largest chunk
    size_t full_lanes = 0;              // lanes [0, full_lanes) hold `cap` proofs; the rest are small lanes (SMALL_LANE_CAP)
    static constexpr size_t SMALL_LANE_CAP = 1024;     // with full lanes larger than this; half of it otherwise (alloc in engine_tables.hip)

    AlgorithmImpl(Cipher c, const uint8_t* pk, size_t pk_len, const uint8_t* r1cs, size_t r1cs_len, const EngineConfig& cf);
    ~AlgorithmImpl() { prover_bytes_on(cfg.device) -= accounted; lanes.clear(); if (stream) stream_give(cfg.device, STREAM_PLAIN, STREAM_ROLE_INIT, stream); }
    // device bytes of the key tables and of every lane (alloc_lane's tally); accounted: what the constructor added to prover_bytes_on(device)
    size_t held_bytes() const { size_t b = table_bytes; for (auto& ln : lanes) b += ln->allocated; return b; }
    size_t accounted = 0;

    std::unique_ptr<SolverProgram> init_program(const R1csFile& cs);

    static void pack_inputs(const ProofRequest* reqs, size_t n, size_t B, uint8_t* h_in, uint8_t* h_rs);      // 176 B and 64 B per column

    // Which wires are bits?  Nothing in an R1CS says so, but it is a property of the circuit, not of the statement: solve 64
    // pseudo-random statements once and call a wire a bit when it is 0 or 1 in all of them.  This is only a PREDICTION used to
    // lay out the wire MSMs (bit wires first, in groups of eight with subset-sum tables); k_msm re-checks every group for
    // every wave of proofs and falls back to the digit tables, so a wrong prediction costs time, never correctness.
    void calibrate();

    // decode the points of `pts` (either encoding, element by element) into out[0 ...] on the init stream; returns per-point status
    // (decode_g1_points / decode_g2_points below: G2 includes the subgroup test)
    std::vector<uint8_t> decompress_g1(const KeyPoints& pts, G1Aff* out) { return decode_g1_points(pts, out, stream); }
    std::vector<uint8_t> decompress_g2(const KeyPoints& pts, G2Aff* out) { return decode_g2_points(pts, out, stream); }

    static constexpr size_t EXPAND_MAX = 64;      // up to this many wide wires of a set are laid out as window octets of its flat part
    static constexpr int EXPAND_C = 15, NARROW_MAX_BITS = 14;

    // Lays out one MSM set and builds its tables.  uniform = true (Z): every base gets a full row, windowed kernel.  Otherwise the
    // bases are sorted by what calibrate() saw on their wires: values in {-1, 0, 1} -> bit groups of eight; values of up to
    // NARROW_MAX_BITS bits (with the margin) -> flat rows of that length; the rest (r, s, the lookup argument's products and inverses)
    // are wide: a few of them become window octets of the flat part, many get the windowed kernel and a Horner pass.
    template <class AffT, class XyzzT, class Decomp>
    // classes: the predicted class per scalar row (default: row_class, the wires); zero_row: a scalar row that is always zero (padding slots; default:
    // row n_wires + 3 of W); latency_layout: also build the (base, window) rows of the windowed part for calls with a handful of statements
    void build_set(MsmSet<AffT>& set, const KeyPoints& raw, size_t point_bytes, const std::vector<uint32_t>& rows, int c, const char* what, Decomp decomp, bool uniform, int expand_cv = 0,
                   const std::vector<uint8_t>* classes = nullptr, uint32_t zero_row = 0xFFFFFFFFu, bool latency_layout = true);
    void init_key(const R1csFile& cs, const PkFile& key);

    void alloc_lane(Lane& ln, size_t B);

    // (slices and scratch of an MSM call: msm_geometry, msm_layout.hpp)
    RouteFacts route_facts() const { return RouteFacts{small.ok, has_commitment, quotient_eval, fuse_z_digits, mZfew.nflat != 0, mA.latency_flat(), mB1.latency_flat(), mB2.latency_flat()}; }
    // one chunk of statements on its way through the stages of prove_chunk: what it is, the route it takes (decided once, read by every stage)
    struct Chunk {
        const ProofRequest* reqs; size_t n, B; DebugVectors* dbg; ChunkRoute rt;
        std::chrono::steady_clock::time_point t_start, t_enqueued, t_done;      // host clock: entry, everything enqueued, results back (GSC_TRACE_HOST)
        std::shared_ptr<ProveCheckCtx> check = nullptr;      // the self-check context loaded when the chunk started (none: not checked)
        uint64_t corrupt = 0;                                // TEST HOOK: the armed change this chunk took (AlgorithmImpl::corrupt)
        std::vector<uint8_t> verdict = {};                   // with check: one byte per statement, 0 = not to be released
        bool check_fell_back = false;
    };
    MsmLaunchOpts msm_opts;      // win_slice: cfg.win_slice (GSC_WIN_SLICE, test hooks); the rest the engine's own choice
    // the byte plane that stands for the scalar matrix `scalars` in the chunk this lane is proving (none: the matrix holds every row)
    MsmCtx with_plane(MsmCtx c, const Lane& ln, const fe* scalars) const {
        if (!ln.small_active) return c;
        if (scalars == ln.d_W.p) { c.plane = ln.d_W8.p; c.plane_rows = n_wires; c.plane_stride = small.rows_per_group; }
        else if (scalars == ln.d_C.p) { c.plane = ln.d_C8.p; c.plane_rows = n_constraints; c.plane_stride = n_constraints; }
        return c;
    }
    int set_index(const MsmSet<G1Aff>& set) const { const MsmSet<G1Aff>* all[Lane::NSETS] = {&mA, &mB1, &mK, &mZ, &mPed, &mPedSigma, &mZfew, &mC}; for (int k = 0; k < Lane::NSETS; k++) if (all[k] == &set) return k; return 0; }
    // The lane adapters of msm_run (msm_set.hpp): which stream, which digit buffer, which scratch, the byte plane.  scalars: the wire matrix W
    // (Montgomery; wire sets) or h (canonical; Z).  The Horner pass is queued in the lane's pending jobs (flush_horner).
    // side = true: on the lane's side stream with scratch buffers of its own (flat sets of calls with a handful of statements only)
    // digits_ready: the windowed part's digits are already in the lane's digit buffer (fuse_z_digits): no recoding pass
    void run_msm_g1(Lane& ln, const Chunk& ck, const MsmSet<G1Aff>& set, const fe* scalars, int mont, G1Xyzz* sum, bool timed = false, bool side = false, bool digits_ready = false);
    void run_msm_g2(Lane& ln, const Chunk& ck, const MsmSet<G2Aff>& set, const fe* scalars, int mont, G2Xyzz* sum, bool side = false);
    template <class AffT> void flush_horner(MsmHornerJobs& pending, size_t B, hipStream_t s) { launch_msm_horner<AffT>(pending, B, s); pending.n = 0; }

    void fetch_column(Lane& ln, const fe* mat, size_t rows, size_t B, size_t col, std::vector<uint8_t>& out);
    // The statement's secrets must not outlive the call in device memory (the witness of these circuits IS a cipher key): enqueued behind a
    // chunk's last kernel, clears the key wires (32-byte rows and byte plane), the rows of r, s, -rs, the raw input records, the prover
    // randomness, its endomorphism split and the commitment mask.  (The reference leaves all of this to Go's garbage collector.)
    // That is the wipe of the rounds before 14 (the secret inputs only), kept for A/B timing (GSC_WIPE=0, test hooks only).  The full wipe (cfg.wipe_full, the default) brings EVERY secret
    // region of the lane (wipe_plan.hpp) back to its idle image: phase A beside the Z sum on the lane's low-priority stream, phase B behind the
    // assembly; a latency call: one launch behind the assembly.
    void wipe_secrets(Lane& ln, size_t B, bool small_call);
    WipePlan plan_wipe(const Lane& ln, const Chunk& ck) const;
    void run_wipe(Lane& ln, const std::vector<WipeItem>& items, hipStream_t s, unsigned max_blocks);
    void wipe_phase_a(Lane& ln, const Chunk& ck);      // from stage_msms, at the trigger
    void wipe_phase_b(Lane& ln, const Chunk& ck);      // from stage_assembly
    void wipe_whole(Lane& ln, hipStream_t s);          // every secret region over its whole allocation (alloc_lane; a call that leaves by an exception)
    // test knob GSC_FAIL_AFTER_STAGE: a host exception behind stage k's enqueue
    void fail_after(int stage) const { if (cfg.fail_after_stage == stage) throw std::runtime_error("GSC_FAIL_AFTER_STAGE=" + std::to_string(stage) + ": test failure injected"); }
    // TEST HOOK: non-zero bytes left in those areas over all lanes (after draining their streams)
    size_t secret_residue();
    // TEST HOOK: bytes off the idle image in every secret region of every lane, over the whole allocations (k_scan_idle); report: see gsc_debug_secret_scan
    size_t secret_scan(size_t lane_base, std::string& report, size_t& registered, size_t& allocated);

    // allow_few_solver / allow_small = false: the retries after the resident solver gave up / a small-integer prediction failed
    void prove_chunk(Lane& ln, const ProofRequest* reqs, size_t n, ProofResult* results, DebugVectors* dbg, bool allow_few_solver = true, bool allow_small = true);
    // the self-check of the chunk, from stage_assembly: enqueued on the lane's stream behind k_fin_combine; the pass is finished behind the lane's wait
    std::unique_ptr<ProveCheckPass> check_enqueue(Lane& ln, const Chunk& ck);
    // its stages, in this order; each enqueues on the lane's streams up to the stage event named (Lane::ev)
    void stage_upload(Lane& ln, const Chunk& ck);           // staging, the scalar split of a latency call: ev[0]
    void stage_witness(Lane& ln, const Chunk& ck);          // W, a, b, c (and the commitment in between): ev[1]
    void stage_early_sums(Lane& ln, const Chunk& ck);       // latency call: A, B1, B2 and the scalar multiplications on the side streams
    void stage_quotient(Lane& ln, const Chunk& ck);         // h or d over a: ev[2]
    void stage_msms(Lane& ln, const Chunk& ck);             // ev[3]
    void stage_assembly(Lane& ln, Chunk& ck);               // ev[4], results to the host, the secrets wiped; waits for the lane
    void stage_stat(Lane& ln, const Chunk& ck);             // stage times and the dominant kernel: ln.stat, last_stat
    void run_levels(Lane& ln, const Chunk& ck, SolverArgs& sa, uint32_t from, uint32_t to);      // witness levels [from, to) with the generic solver kernels
    void solve_small(Lane& ln, const Chunk& ck);            // the whole witness with the small-integer kernels
    void dump_solver_trace(Lane& ln, const unsigned long long* d_trace);      // GSC_SOLVER_TRACE
    void trace_chunk(Lane& ln, const Chunk& ck);            // GSC_TRACE_HOST

    // gnark proof.WriteTo: Ar | Bs | Krs compressed, u32be nbCommitments, commitments, CommitmentPok
    // released = false: the self-check did not accept the statement's points (status 3, no bytes)
    void serialize(const uint8_t* o, uint8_t flags, uint32_t status, const uint8_t* commitment_xy, const uint8_t* pok_xy, ProofResult& res, bool released = true) const;
};

}  // namespace gsc
