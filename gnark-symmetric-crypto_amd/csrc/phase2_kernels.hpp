// Launchers of the key ceremony's kernels (k_phase2.hip).  Types come from verify_dev.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include "verify_batch_dev.hpp"

namespace gsc {
// out[i] = k in[i] for decoded key points (infinity stays infinity); k: eight little-endian 32-bit words in device memory, 0 < k < r, the
// same for every point.  The ladder does not branch on k's bits.
void launch_scale_points(const vfy::VP1* in, size_t n, const uint32_t* k, vfy::VP1* out, hipStream_t s);
void launch_scale_points(const vfy::VP2* in, size_t n, const uint32_t* k, vfy::VP2* out, hipStream_t s);
// out[i] = k_i in[i]: every point has a scalar of its own, word w of point i's scalar at rows[w * n + i] (eight little-endian words, below r:
// k_fr_powers' layout).  The same ladder, the same discipline.
void launch_scale_points_each(const vfy::VP1* in, size_t n, const uint32_t* rows, vfy::VP1* out, hipStream_t s);
void launch_scale_points_each(const vfy::VP2* in, size_t n, const uint32_t* rows, vfy::VP2* out, hipStream_t s);
// rows[w * n + i] = word w of m x^(first + i) mod r, canonical, for i < n; x, m: eight little-endian words each in device memory, below r
void launch_fr_powers(const uint32_t* x, const uint32_t* m, uint64_t first, size_t n, uint32_t* rows, hipStream_t s);
// decoded points -> raw big-endian canonical bytes (G1: 64 B X | Y; G2: 128 B X.A1 | X.A0 | Y.A1 | Y.A0; zeros for infinity) and infinity flags
void launch_points_be(const vfy::VP1* p, size_t n, uint8_t* out, uint8_t* inf, hipStream_t s);
void launch_points_be(const vfy::VP2* p, size_t n, uint8_t* out, uint8_t* inf, hipStream_t s);
// sums[0] = sum rho_i a[i], sums[1] = sum rho_i b[i], affine; rho: four little-endian words per point; part: 2 * phase2_rlc_blocks(n) entries
size_t phase2_rlc_blocks(size_t n);
void launch_phase2_rlc(const vfy::VP1* a, const vfy::VP1* b, const uint32_t* rho, size_t n, vfy::G1X* part, vfy::VP1* sums, hipStream_t s);
// the same over G2 (one kernel template, k_phase2_rlc<P>)
using G2X = bn254::Xyzz9<bn254::Fp2x>;
void launch_phase2_rlc(const vfy::VP2* a, const vfy::VP2* b, const uint32_t* rho, size_t n, G2X* part, vfy::VP2* sums, hipStream_t s);
}  // namespace gsc
