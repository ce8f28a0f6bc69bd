// The prover's self-check as the engine sees it (gsc_prove_check_init, include/libprove.h): one context per engine replica — a verifying key
// on the replica's device with chunk buffers for the replica's largest lane (verify_gpu.cpp builds it exactly as gsc_verify_init builds a
// verifier's key) — and one pass per chunk, enqueued on the lane's stream behind the assembly.  The context's buffers hold public data only
// (the key's tables, the proofs' points, the public inputs, the randomizers) and are no part of any lane.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include <memory>
#include <mutex>
#include <vector>

namespace gsc {

struct ProveCheckCtx;      // verify_gpu.cpp

// The context for `algo` under the gnark VerifyingKey.WriteTo bytes `vk` on `device`, for chunks of up to `cap` statements.  nullptr (one line
// on stdout) for a key gsc_verify_init would refuse; throws std::runtime_error on a HIP error.
std::shared_ptr<ProveCheckCtx> prove_check_create(int algo, const uint8_t* vk, size_t len, int device, size_t cap);
size_t prove_check_device_bytes(const ProveCheckCtx& c);
// chunks checked, proofs checked, proofs refused by the check, chunks that needed the proof-by-proof pass
void prove_check_add_stats(const ProveCheckCtx& c, uint64_t out[4]);

// The lane's output buffers of the chunk (prove_check_kernels.hpp ProverOut) and the statements' public signals, n x 144 bytes
// ct | nonce | counter (little-endian for ChaCha20, big-endian for AES) | pt, as the caller's verifier would build them.
struct ProveCheckInput { const uint8_t* d_out; const uint8_t* d_cpts; const uint32_t* d_status; const uint8_t* d_flags; size_t B, n; const uint8_t* signals; };

// One chunk's pass.  The constructor takes the context (lanes of a replica share it: one pass at a time) and enqueues on `s` the uploads,
// k_check_prep, the batch check on the route the verifier takes for n items, and the copies of its result; finish(), called once `s` has been
// synchronised, gives one verdict byte per statement.  status / flags: the lane's status and flag words, now on the host.  When the batch check
// did not accept every statement the prover would release — its equation failed, or such a statement's points did not pass k_check_prep — it
// first runs the per-proof pairings over the same entries, which then decide, and synchronises `s` again.  A statement the prover has refused
// already has verdict 0 and counts for nothing.  Throws on a HIP error.
class ProveCheckPass {
  public:
    ProveCheckPass(std::shared_ptr<ProveCheckCtx> ctx, const ProveCheckInput& in, hipStream_t s);
    ~ProveCheckPass();
    const std::vector<uint8_t>& finish(const uint32_t* status, const uint8_t* flags);
    bool fell_back() const { return fell_back_; }
    // the chunk's figures into the context's counters (the caller knows which statements it would have released)
    void count(size_t checked, size_t refused);
  private:
    std::shared_ptr<ProveCheckCtx> ctx_; std::unique_lock<std::mutex> lock_; hipStream_t s_; size_t n_; bool few_ = false, fell_back_ = false, finished_ = false;
    std::vector<uint8_t> win_, verdict_; std::vector<uint32_t> rnd_; uint8_t flag_ = 0;
};

}  // namespace gsc
