// Key ceremony, second phase: the calls behind gsc_setup_contribute / gsc_setup_verify_contribution / gsc_debug_scale_points
// (include/libprove.h).  Host rules: phase2.hpp; kernels: k_phase2.hip.  Neither needs an initialised algorithm.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace gsc {

struct Phase2Step { std::vector<uint8_t> pk, vk; uint8_t record[224]; };
// 0: out filled.  -2: a key that does not parse, a refused point, pk and vk that disagree on delta (one line on stdout).  Throws
// std::runtime_error on a device error.  seed32 != nullptr: the TEST secrets of phase2.hpp seeded_scalar (the caller gates this).
int phase2_contribute(const uint8_t* pk, size_t pk_len, const uint8_t* vk, size_t vk_len, const uint8_t* seed32, Phase2Step& out);
// 1 accepted, 0 refused (one line on stdout naming the first rule that failed).  Throws std::runtime_error on a device error.
int phase2_verify(const uint8_t* pk_prev, size_t pk_prev_len, const uint8_t* vk_prev, size_t vk_prev_len, const uint8_t* pk_next, size_t pk_next_len,
                  const uint8_t* vk_next, size_t vk_next_len, const uint8_t* record);
// TEST HOOK body: out[i] = scalar * pts[i] through k_scale_points; throws std::runtime_error (bad group, a point that does not decode, scalar >= r, device)
void phase2_debug_scale(int group, const uint8_t* pts, const uint8_t* inf, size_t n, const uint8_t* scalar_be32, uint8_t* out, uint8_t* out_inf);

}  // namespace gsc
