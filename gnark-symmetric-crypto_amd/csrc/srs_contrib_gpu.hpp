// Key ceremony, first phase (srs_contrib.hpp): the calls behind gsc_srs_contribute / gsc_srs_verify_contribution /
// gsc_debug_scale_powers (include/libprove.h).  Host rules: srs.hpp, srs_contrib.hpp; kernels: the verifier's key-point decoder, k_fr_powers
// and the per-point instance of k_scale_points (k_phase2.hip); the check of the next file is srs_verify (srs_gpu.hpp).  No call needs an
// initialised algorithm; each has a stream and buffers of its own on GSC_DEVICE / the first of GSC_DEVICES.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace gsc {

// One contribution: 0 and the new file in `out`, the record (544 bytes) in `record`; -2 a refused file or a seed that gives a zero scalar (one
// line on stdout).  seed32 == nullptr: secrets and nonces from the OS CSPRNG; seed32 (TEST, the caller gates it): srs_contrib.hpp's seeded
// scalars.  Throws std::runtime_error on a device error.
int srs_contribute(const uint8_t* srs, size_t len, const uint8_t* seed32, std::vector<uint8_t>& out, uint8_t* record);
// 1 accepted, 0 refused (one line on stdout naming the first rule that failed, rules 1-5 of DESIGN.md §3.12).  prev is NOT checked in full:
// a chain is verified link by link from the bytes of gsc_srs_initial.  Throws std::runtime_error on a device error.
int srs_verify_contribution(const uint8_t* prev, size_t prev_len, const uint8_t* next, size_t next_len, const uint8_t* record);
// TEST HOOK body: out[i] = m x^(first + i) pts[i] through k_fr_powers and the per-point ladder, by the launcher a contribution uses.  Conventions
// and refusals as phase2_debug_scale.  Throws std::runtime_error (bad group / point / scalar, device).
void srs_debug_scale_powers(int group, const uint8_t* pts, const uint8_t* inf, size_t n, const uint8_t* x_be32, const uint8_t* m_be32, uint64_t first,
                            uint8_t* out, uint8_t* out_inf);

}  // namespace gsc
