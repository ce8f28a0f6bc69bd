// Launchers of the few-proof verifier kernels (k_verify_few.hip): one group of 8 lanes per proof.  Types come from verify_dev.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include "verify_dev.hpp"

namespace gsc {
constexpr size_t kFewChunk = 8192;      // proofs per device pass of the few-proof path (the lines buffer holds kLineSteps lines for each)
// the Miller lines of every proof's B (skipped without ok or with A or B at infinity): kLineSteps per proof
void launch_verify_few_lines(const vfy::ProofDev* pd, size_t n, vfy::Line* out, hipStream_t s);
// launch_verify_pairing's verdicts (and fout) from the lines above
void launch_verify_few_pairing(const vfy::KeyDev& k, const vfy::ProofDev* pd, const vfy::Line* lines, uint8_t* verdict, vfy::F12* fout, size_t n, hipStream_t s);
// the miller step of the batched check (k_verify_batch.hip): f[i] for the n proofs, f[n + t] for the fixed pairs
void launch_verify_few_batch_miller(const vfy::KeyDev& k, const vfy::ProofDev* pd, const vfy::VP1* ra, const vfy::VP1* fixed, const vfy::Line* lines, size_t n, vfy::F12* f, hipStream_t s);
// the same kernel over the proofs alone: f[i] for the n proofs (the claim-wise check, k_verify_claims.hip, has fixed pairs per part)
void launch_verify_few_proof_miller(const vfy::KeyDev& k, const vfy::ProofDev* pd, const vfy::VP1* ra, const vfy::Line* lines, size_t n, vfy::F12* f, hipStream_t s);
// flag[0] = final_exp(f[0]) == 1
void launch_verify_few_final(const vfy::F12* f, uint8_t* flag, hipStream_t s);
}  // namespace gsc
