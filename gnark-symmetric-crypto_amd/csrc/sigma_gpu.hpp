// Key ceremony, the Pedersen sigma: the calls behind gsc_pedersen_verify / gsc_setup_contribute_sigma /
// gsc_setup_verify_sigma_contribution / gsc_setup_verify_from_srs (include/libprove.h).  Host rules: sigma.hpp; kernels: the ceremony's
// (k_phase2.hip) and the verifier's, none of its own.  None needs an initialised algorithm.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace gsc {

struct SigmaStep { std::vector<uint8_t> pk, vk; uint8_t record[224]; };
// 1 accepted, 0 refused (one line on stdout naming the rule).  Throws std::runtime_error on a device error.
int pedersen_verify(const uint8_t* pk, size_t pk_len, const uint8_t* vk, size_t vk_len);
// 0: out filled.  -2: a key that does not parse, no commitment key, a refused point, a seed that gives a zero scalar (one line on stdout).
// Throws std::runtime_error on a device error.  seed32 != nullptr: the TEST secrets of sigma.hpp seeded_scalars (the caller gates this).
int sigma_contribute(const uint8_t* pk, size_t pk_len, const uint8_t* vk, size_t vk_len, const uint8_t* seed32, SigmaStep& out);
// 1 accepted, 0 refused (one line on stdout naming the first rule that failed).  Throws std::runtime_error on a device error.
int sigma_verify(const uint8_t* pk_prev, size_t pk_prev_len, const uint8_t* vk_prev, size_t vk_prev_len, const uint8_t* pk_next, size_t pk_next_len,
                 const uint8_t* vk_next, size_t vk_next_len, const uint8_t* record);
// 1 accepted, 0 refused (one line on stdout naming the rule).  Throws SrsRefused (srs_gpu.hpp: malformed r1cs, a refused powers file,
// L < log2 n) or std::runtime_error (device).
int setup_verify_from_srs(const uint8_t* r1cs, size_t r1cs_len, const uint8_t* srs, size_t srs_len, const uint8_t* pk, size_t pk_len, const uint8_t* vk, size_t vk_len);

}  // namespace gsc
