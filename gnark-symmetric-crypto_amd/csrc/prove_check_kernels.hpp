// Launchers of the prover's self-check kernels (k_prove_check.hip).  Types come from verify_dev.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include "verify_dev.hpp"

namespace gsc {
// The prover's output buffers of one chunk of B columns, n of them real statements (engine_impl.hpp Lane): out = d_out (256 B per column),
// cpts = d_cpts (D of column i at 64 i, PoK at 64 B + 64 i; read only for a key with a commitment), status / flags = d_status / d_flags.
struct ProverOut { const uint8_t* out; const uint8_t* cpts; const uint32_t* status; const uint8_t* flags; size_t B, n; };
// pd[i] for i < n: k_verify_prep's result for the bytes column i will be serialised to; ok = 0 for a column the prover has refused already
// (solver status, an infinity flag) and for one whose points the decoder would not give back.  win: n x kWindows public-input windows.
void launch_check_prep(const vfy::KeyDev& k, const ProverOut& o, const uint8_t* win, vfy::ProofDev* pd, hipStream_t s);
// TEST HOOK (gsc_debug_prove_corrupt): changes point `which` (0 A, 1 B, 2 C, 3 D, 4 PoK) of column `index` < n.  mode 0: the same point of
// column (index + 1) mod n; mode 1: bit 0 of its y flipped.  out / cpts are written inside that column's own slot only.
void launch_prove_corrupt(uint8_t* out, uint8_t* cpts, size_t B, size_t n, uint32_t index, int which, int mode, hipStream_t s);
}  // namespace gsc
