// The witness solver's device tables and launch sequences, shared by the engine (AlgorithmImpl derives from SolverTables) and the test hook
// gsc_debug_solve (solver_debug.hip): what InitAlgorithm builds and uploads from an R1csFile — the program and its level schedule, the layout for
// calls with a handful of statements, the count tables with their device check, coeff / coeff_inv, the lookup table, the small-integer program with
// its pads — and the loops that walk it: solver_run_levels (the generic kernels, batch or resident) and solver_run_small (the byte-plane kernels).
// Implementation: solver_tables.hip.  Reference counterpart: cs.Solve inside groth16.Prove (libraries/prover/impl/provers.go:148).
#pragma once
#include "formats.hpp"
#include "kernels.hpp"
#include "wit_small.hpp"
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

namespace gsc {

#define HIP_CHECK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) throw std::runtime_error(std::string("HIP error: ") + hipGetErrorString(e_) + " at " #expr); } while (0)

// the calling thread's device for what follows; throws when the process sees no HIP device at all (the hooks: after every refusal the host can decide)
inline void use_device(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) throw std::runtime_error("no HIP device available");
    HIP_CHECK(hipSetDevice(device));
}

// alloc_lane points this at the lane's byte count for its duration: every DevBuf the thread allocates meanwhile is counted, so that the lane's
// region table (wipe_plan.hpp) can be held against what was really allocated
inline thread_local size_t* devbuf_tally = nullptr;

template <class T>
struct DevBuf {
    T* p = nullptr; size_t n = 0;
    bool secret = false;      // a temporary that holds a call's data: zeroed before it is freed, also when an exception unwinds (like setup_dev.hip's Buf)
    DevBuf() = default;
    explicit DevBuf(size_t count, bool is_secret = false) : secret(is_secret) { alloc(count); }
    DevBuf(const DevBuf&) = delete; DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void release() { if (p) { if (secret) { (void)hipMemset(p, 0, n * sizeof(T)); (void)hipDeviceSynchronize(); } (void)hipFree(p); p = nullptr; } }
    void alloc(size_t count) { release(); n = count; if (count) { HIP_CHECK(hipMalloc((void**)&p, count * sizeof(T))); if (devbuf_tally) *devbuf_tally += count * sizeof(T); } }
    void upload(const T* src, size_t count, hipStream_t s) { HIP_CHECK(hipMemcpyAsync(p, src, count * sizeof(T), hipMemcpyHostToDevice, s)); }
    size_t bytes() const { return n * sizeof(T); }
};

// The resident solver kernel (k_solver_few) spins at device-wide barriers, so two of them must never share the device: each could
// hold CUs the other's missing workgroups are waiting for.  Launches are therefore chained on the device: a launch first makes its
// stream wait for the previous one's completion event (no host blocking).  Other processes on the same device are not covered —
// there the kernel's bounded polling gives up and the call is solved again with one launch per level (prove_chunk).
struct FewSolverChain { std::mutex m; hipEvent_t last = nullptr; };
FewSolverChain& few_solver_chain(int device);      // one per device, never destroyed (lanes may outlive static destructors): engine_prove.hip

struct SolverTables {
    size_t n_wires = 0, n_public = 0, n_inputs = 0, n_constraints = 0;      // n_inputs: public + secret wires (what k_assign_* writes)
    bool has_commitment = false;
    // program
    DevBuf<uint32_t> prog, sched, lookup_coeff; DevBuf<fe> coeff, coeff_inv;
    DevBuf<uint32_t> few_count_ops, few_count_qoff; std::vector<uint32_t> few_count_first;
    DevBuf<uint32_t> few_ops, few_terms, few_lstart;          // the same program laid out for k_solver_few (formats.hpp FewProgram)
    uint32_t n_levels = 0, commit_level = 0; std::vector<uint32_t> level_width; std::vector<uint8_t> level_kind; std::vector<uint32_t> level_long; int has_div = 0;
    // The small-integer witness path (wit_small.hpp): built for circuits that qualify (ChaCha20-V3); small.ok says so.
    // small keeps the sizes and the per-row classes; the item lists live on the device.
    SmallProgram small;
    DevBuf<uint32_t> ws_tiny, ws_parts, ws_bits, ws_twire, ws_levels, ws_rtiny, ws_rgen, ws_rtwire; DevBuf<long long> ws_tcoef, ws_rtcoef;
    DevBuf<uint8_t> ws_cls_a, ws_cls_b, ws_cls_c;      // per constraint row: 0 = byte plane, 1 = 32-byte element

    // Builds the solver program from cs and uploads it with everything the generic kernels read (stream is synchronised before returning).  Throws
    // std::runtime_error for a description the builders refuse, coefficient ids 0..4 that are not 0, 1, 2, -1, -2, or a count table whose index column
    // is not 0..n-1 (checked on the device).
    std::unique_ptr<SolverProgram> build_tables(const R1csFile& cs, hipStream_t stream);
    // The small-integer program from the class predictions (0 = bit, 1 = also -1, more = wide): integer coefficients from launch_coeff_small,
    // build_small_program, the item lists with their pads uploaded when the circuit qualifies (small.ok; small.why otherwise).
    void build_small_tables(const SolverProgram& sp, const std::vector<uint8_t>& class_w, const std::vector<uint8_t>& class_a, const std::vector<uint8_t>& class_b,
                            const std::vector<uint8_t>& class_c, hipStream_t stream);
};

// One walk over witness levels [from, to) with the generic kernels.  sa: the buffers of the call (W, A, B, C, status, mask, commit, batch, trace);
// resident: the first n columns by k_solver_few / k_solver_count_few, a run of generic levels being ONE launch that takes its place in the
// device's few_solver_chain (fsync: the two sync words, ev_few: the caller's completion event); otherwise one launch per level on all columns.
struct SolverWalk {
    size_t n = 0; bool resident = false;
    uint32_t workgroups = 0;          // resident grid: 0 = the measured choice (128 for 1-2 statements, 256 beyond); always clamped to cu_count
    int cu_count = 256, device = 0;
    bool test_abort = false;          // test: the barrier never fills
    uint32_t* fsync = nullptr; hipEvent_t ev_few = nullptr;
    uint32_t launches = 0, workgroups_used = 0;      // out: resident launches of this walk, and the grid of the last one
};
void solver_run_levels(const SolverTables& t, SolverArgs& sa, SolverWalk& w, uint32_t from, uint32_t to, hipStream_t stream);

// The whole witness with the small-integer kernels (t.small.ok): narrow the input rows of W, chain, rows; expand: every row also as a 32-byte element.
struct SmallBuffers { fe* W; fe* A; fe* B; fe* C; int8_t* W8; int8_t* A8; int8_t* B8; int8_t* C8; uint32_t* status; uint32_t* flag; };
void solver_run_small(const SolverTables& t, const SmallBuffers& b, size_t batch, bool expand, hipStream_t stream);

}  // namespace gsc
