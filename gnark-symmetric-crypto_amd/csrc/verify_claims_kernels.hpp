// Launcher of the claim-wise batched check (k_verify_claims.hip).  Types come from verify_claims_dev.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include "verify_batch_kernels.hpp"
#include "verify_claims_dev.hpp"

namespace gsc {
// device buffers of one chunk of n proofs in at most n parts, beside the BatchBufs it shares with the batched check (ra, ok, f)
struct ClaimBufs {
    vfy::claims::Part* parts;   // n: the chunk's parts, in order (the caller fills the first np)
    vfy::G1X* terms;            // n x kBatchSums: every proof's own terms; a part's totals end up in its first proof's
    uint32_t* rho;              // n x 5 words: sum rho of each part
    vfy::VP1* fixed;            // n x kBatchFixed G1 points of the parts' fixed pairs
    vfy::F12* pf;               // n x kBatchFixed Miller values of the parts' fixed pairs; a part's product ends up in its first
    uint8_t* flag;              // n: 1: the part's check holds
};
// rnd: n x kRandWords words (rho_i, t_i); c.parts[0, np) tile [0, n).  Writes b.ok (per proof) and c.flag (per part); a part is accepted
// iff its flag is 1 and every one of its proofs has ok.  few_lines as in launch_verify_batch.
void launch_verify_claims(const vfy::KeyDev& k, const vfy::ProofDev* pd, const uint32_t* rnd, size_t n, size_t np, const BatchBufs& b,
                          const ClaimBufs& c, vfy::Line* few_lines, hipStream_t s);
}  // namespace gsc
