// Powers file (srs.hpp): the calls behind gsc_srs_verify / gsc_debug_srs_generate (include/libprove.h).  Host rules:
// srs.hpp; kernels: the verifier's key-point decoder, k_phase2.hip's random combinations in both groups, the few-proof pairing kernels.
// Neither call needs an initialised algorithm.
#pragma once
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>
#include "setup.hpp"

namespace gsc {

// 1 accepted, 0 refused (one line on stdout naming the first rule that failed, rules 1-7 of DESIGN.md §3.11).  Throws std::runtime_error
// on a device error.  Thread-safe: a stream and buffers of its own on GSC_DEVICE / the first of GSC_DEVICES.  who / prefix: the call the
// line speaks for and what stands before the rule (gsc_srs_verify_contribution runs this check on a step's next file as its rule 5).
int srs_verify(const uint8_t* srs, size_t len, const char* who = "gsc_srs_verify", const std::string& prefix = std::string());
// Groth16 Setup from a powers file (gsc_setup_from_srs): no scalar of the file is known here; the Lagrange bases at tau (group_idft.hpp),
// the column sums A, B, K (k_srs_columns.hip) and Z are computed in the groups, on the device, and written by setup.cpp's one writer.
// seed32 == nullptr: gamma = delta = 1, the Pedersen sigma and g from the OS CSPRNG.  seed32 (TEST, the caller gates it): gamma, delta, sigma,
// g = groth16_setup's toxic(seed, ...), so that the keys equal gsc_setup's for a file made from the same seed.
// Throws SrsRefused (malformed r1cs, a file gsc_srs_verify refuses, L < log2 n) or std::runtime_error (device).
struct SrsRefused : std::runtime_error { using std::runtime_error::runtime_error; };
SetupKeys setup_from_srs(const uint8_t* r1cs, size_t r1cs_len, const uint8_t* srs, size_t len, const uint8_t* seed32);
// TEST HOOK body: the file for tau, alpha, beta = toxic(seed, "tau" | "alpha" | "beta") (setup.hpp), 1 <= L <= 20, through
// setup_generator_muls on `device`.  Throws std::runtime_error (L out of range, device).
std::vector<uint8_t> srs_debug_generate(int L, const uint8_t* seed32, int device);
// TEST HOOK body: out[j] = (1 / n) sum_k w^(-jk) pts[k] over n = 2^L raw finite points of group 0 (G1, 64 B) or 1 (G2, 128 B), natural order
// (group_idft.hpp); out_inf[j] = 1 and zeros for the point at infinity.  1 <= L <= 17.  Throws std::runtime_error (bad group / L / point, device).
void srs_debug_group_idft(int group, int L, const uint8_t* pts, uint8_t* out, uint8_t* out_inf);
// TEST HOOK body: out[w] = sum over the terms [col_start[w], col_start[w + 1]) of coeff[term_coeff] rows[term_row] through the column-sum
// kernels with their segmenting (srs_columns.hpp); rows: n_rows raw finite points; coeff_be: n_coeff scalars below r, 32 big-endian bytes
// each.  Throws std::runtime_error (bad group / point / index / coefficient, device).
void srs_debug_column_sums(int group, uint32_t n_rows, const uint8_t* rows, uint32_t n_cols, const uint32_t* col_start, const uint32_t* term_row, const uint32_t* term_coeff,
                           uint32_t n_coeff, const uint8_t* coeff_be, uint8_t* out, uint8_t* out_inf);

}  // namespace gsc
