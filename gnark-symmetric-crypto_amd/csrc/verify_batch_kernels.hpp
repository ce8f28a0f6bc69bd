// Launcher of the batched Groth16 check (k_verify_batch.hip).  Types come from verify_batch_dev.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include "verify_batch_dev.hpp"

namespace gsc {
// device buffers of one chunk of n proofs (sizes for n = the chunk size)
struct BatchBufs {
    vfy::VP1* ra;          // n: rho A, affine
    uint8_t* ok;           // n: the proof passed k_verify_prep (decoding, subgroup test)
    vfy::G1X* part;        // batch_blocks(n) x kBatchSums block partials
    uint64_t* rpart;       // batch_blocks(n) x 4 column sums of rho
    vfy::VP1* fixed;       // kBatchFixed G1 points of the fixed pairs
    vfy::F12* f;           // n + kBatchFixed Miller values, product in f[0]
    uint8_t* flag;         // 1: the chunk's batch check holds
};
size_t batch_blocks(size_t n);
// rnd: n x kRandWords words (rho_i, t_i).  Writes b.ok and b.flag; proofs without ok contribute nothing.  few_lines != nullptr (room for
// n x kLineSteps lines): the Miller pass runs on the few-proof kernels (k_verify_few.hip); the final exponentiation always does.
void launch_verify_batch(const vfy::KeyDev& k, const vfy::ProofDev* pd, const uint32_t* rnd, size_t n, const BatchBufs& b, vfy::Line* few_lines, hipStream_t s);
// the proofs' part of the Miller pass alone, one thread per proof: f[i] = e(ra[i], B_i) unreduced, 1 for a proof without ok (the
// claim-wise check, k_verify_claims.hip)
void launch_verify_batch_proof_miller(const vfy::KeyDev& k, const vfy::ProofDev* pd, const vfy::VP1* ra, size_t n, vfy::F12* f, hipStream_t s);
}  // namespace gsc
