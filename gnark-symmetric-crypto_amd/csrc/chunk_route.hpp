// The route of one chunk of statements through the prover, decided once (AlgorithmImpl::prove_chunk) and read by every stage: which
// witness solver, which quotient form, which MSM kernels, what runs beside what.  A pure function of the call's size, the configuration
// and a few facts about the engine: no HIP, no state (tests/native/chunk_route_check.cpp pins every field on the CPU).
#pragma once
#include "engine.hpp"

namespace gsc {

// what the route depends on besides the configuration.  Fixed at InitAlgorithm (AlgorithmImpl::route_facts):
struct RouteFacts {
    bool small_ok = false;          // the circuit has a small-integer witness program (wit_small.hpp); implies no commitment
    bool has_commitment = false;
    bool quotient_eval = false, fuse_z_digits = false;      // what init_key built (the configuration's wishes, where the key allowed them)
    bool zfew_flat = false;         // the quotient bases have a latency layout (mZfew.nflat)
    bool a_flat = false, b1_flat = false, b2_flat = false;      // MsmSet::latency_flat() of the sets A, B1, B2
};
// ... and per call of prove_chunk:
struct RouteCall {
    bool dbg = false;               // debug vectors are wanted
    bool allow_few_solver = true;   // false: the retry after the resident solver gave up
    bool allow_small = true;        // false: the retry after a small-integer prediction failed
    bool skip_resident = false;     // the give-up penalty says: not this time (AlgorithmImpl::few_skip, consumed by the caller)
};

struct ChunkRoute {
    bool latency = false;           // the chunk takes the latency kernels: MSMs, quotient, assembly
    bool resident_wanted = false;   // the configuration would solve its witness with the resident kernel (k_solver_few)
    bool small = false;             // the witness is solved by the integer kernels on byte planes
    bool resident = false;          // ... by the resident kernel
    bool early_ab = false, early_b2 = false;      // the A and B1 sums (and the B2 sum) start on the side streams right after the witness
    bool use_zfew = false;          // the Z sum runs over the latency layout, which holds the key's own Z: coefficient form
    bool eval = false;              // the quotient in evaluation form
    bool z_digits_ready = false;    // ... whose last kernel writes the digits of d itself
    bool overlap_q = false;         // ... on the lane's third stream, beside the wire-set MSMs
    const char* kernel_name = "";   // the dominant kernel, as KernelStat names it (bench.py and the tests read these strings)
};

// batch calls smaller than this run the quotient beside the wire-set MSMs (cfg.overlap_quotient == 1): larger ones have nothing to gain,
// their tails are 1 % of the call
constexpr size_t OVERLAP_QUOTIENT_BELOW = 4096;

inline ChunkRoute chunk_route(size_t n, const EngineConfig& cfg, const RouteFacts& f, const RouteCall& call) {
    const size_t B = (n + 63) / 64 * 64;
    ChunkRoute r;
    // few_max <= MSM_FEW_PROOFS = 32 (AlgorithmImpl's constructor refuses anything else), so such a call is one 64-column batch
    r.latency = cfg.few_path && n <= (size_t)cfg.few_max;
    // NOT a function of few_path: GSC_FEW_PATH=0 alone leaves the resident solver on (a configuration that wants neither sets GSC_FEW_SOLVER=0 too)
    r.resident_wanted = n <= (size_t)cfg.few_max && B == 64 && cfg.few_solver;
    r.small = f.small_ok && call.allow_small && !cfg.solver_trace && (!r.latency || cfg.small_witness_few);
    r.resident = r.resident_wanted && call.allow_few_solver && !r.small && !call.skip_resident;      // (the small-integer path needs no resident grid)
    r.early_ab = r.latency && f.a_flat && f.b1_flat;
    r.early_b2 = r.early_ab && f.b2_flat;
    r.use_zfew = r.latency && f.zfew_flat;
    r.eval = f.quotient_eval && !r.use_zfew;
    r.z_digits_ready = r.eval && f.fuse_z_digits && !r.latency;
    r.overlap_q = r.z_digits_ready && !call.dbg && (cfg.overlap_quotient == 2 || (cfg.overlap_quotient && B < OVERLAP_QUOTIENT_BELOW));
    // a latency call's dominant kernel is its witness solver, a batch call's the Z-table gather-accumulate
    r.kernel_name = !r.latency ? "k_msm_win<Fp29f>"
                  : r.small ? "k_wit_chain + k_wit_rows"
                  : !r.resident ? "k_solver (one launch per level)"
                  : f.has_commitment ? "k_solver_few + commitment MSM" : "k_solver_few";
    return r;
}

}  // namespace gsc
