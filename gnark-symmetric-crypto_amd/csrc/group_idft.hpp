// The group transform of a powers file (k_quot_bases.hip): out[j] = (1 / n) sum_k w^(-jk) in[k], n = 2^L, w the domain's
// generator (gnark-crypto's 2^28-th root squared 28 - L times, as groth16_setup has it) — with in[k] = tau^k G the Lagrange basis L_j(tau) G,
// without anybody knowing tau.  The stage kernel is the quotient bases' (k_qb_stage<F>), over G1 or G2.  Points are the verifier's decoded
// images (verify_dev.hpp), in and out in natural order; in may hold points at infinity, out flags them.
#pragma once
#include <hip/hip_runtime.h>
#include "verify_dev.hpp"

namespace gsc {
// device memory the transform needs, free again once the stream has passed
size_t group_idft_scratch_bytes(int L, bool g2);
// 1 <= L <= 24 for the index arithmetic; n log n / 2 + n scalar multiplications with the exact group law
void launch_group_idft(const vfy::VP1* in, int L, void* scratch, vfy::VP1* out, hipStream_t s);
void launch_group_idft(const vfy::VP2* in, int L, void* scratch, vfy::VP2* out, hipStream_t s);
}  // namespace gsc
