// Launchers of the GPU verifier's kernels (k_verify.hip).  Types come from verify_dev.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include "verify_dev.hpp"

namespace gsc {
void launch_verify_key_points(const uint8_t* g1, size_t n1, const uint8_t* g2, size_t n2, vfy::VP1* o1, vfy::VP2* o2, int8_t* st, hipStream_t s);
void launch_verify_tables(const vfy::VP1* K, const uint32_t* desc, size_t nwin, vfy::VP1* table, hipStream_t s);
void launch_verify_lines(const vfy::VP2* q, size_t n, vfy::Line* out, hipStream_t s);
void launch_verify_prep(const vfy::KeyDev& k, const uint8_t* proofs, const uint8_t* win, const uint8_t* pre, vfy::ProofDev* pd, size_t n, hipStream_t s);
void launch_verify_pairing(const vfy::KeyDev& k, const vfy::ProofDev* pd, uint8_t* verdict, vfy::F12* fout, size_t n, hipStream_t s);
void launch_verify_debug_points(const uint8_t* g1, const uint8_t* g2, vfy::ProofDev* pd, size_t n, hipStream_t s);
void launch_verify_f12_bytes(const vfy::F12* f, uint8_t* out, size_t n, hipStream_t s);
// test hook (gsc_debug_verify_g1): n VP1 / VP2 images `stride` bytes apart -> 65 / 129 bytes each, `ostride` apart: canonical big-endian
// coordinates and an infinity byte; live (optional): int32 words `lstride` apart, a point whose word is zero is left alone
void launch_verify_point_bytes(const void* src, size_t stride, bool g2, const void* live, size_t lstride, uint8_t* out, size_t ostride, size_t n, hipStream_t s);
}  // namespace gsc
