// Host-side rules of Groth16 verification shared by libverify.so (verifier.cpp, CPU) and the GPU verifier in libprove.so
// (verify_gpu.cpp): the verifying-key layout, proof sizes and commitment counts, and the order of the public inputs
// (reference libraries/verifier/impl/verifiers.go:18-40, 50-152).  Byte checks and packing only: decoding and
// all curve arithmetic belong to the callers.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>
#include "json.hpp"

namespace gsc {
namespace verify {

constexpr size_t kSignalBytes = 144;                  // ct[64] | nonce[12] | counter[4] | pt[64]
constexpr size_t kWindows = 144;                      // public-input byte windows per statement (both circuits)
constexpr size_t kChachaInputs = 1152, kAesInputs = 141;

// A point of a key is compressed (flag bits 10 / 11, or 01 for infinity: 32 B in G1, 64 B in G2) or raw (flag bits 00: X | Y, 64 B / 128 B,
// all zero for infinity), element by element, as gnark's decoder reads what WriteTo / WriteRawTo wrote.
inline bool point_is_raw(const uint8_t* first_byte) { return (*first_byte & 0xC0) == 0; }

// gnark VerifyingKey.WriteTo / WriteRawTo layout: offsets of the points in the key bytes (each in either encoding: point_is_raw)
struct VkLayout {
    size_t alpha = 0, g1_beta = 0, beta = 0, gamma = 0, g1_delta = 0, delta = 0;   // G1 32 (raw 64) bytes, G2 64 (raw 128) bytes
    std::vector<size_t> K;                                                        // G1
    bool has_commitment = false;
    size_t ped_g = 0, ped_gsn = 0;                                                // G2, when has_commitment
};
// false (and *err set) when the key is truncated, has trailing bytes or an unsupported commitment layout
bool parse_vk_layout(const uint8_t* b, size_t n, VkLayout& out, std::string* err);

uint32_t be32(const uint8_t* p);
size_t num_public(int algorithm);                     // 1152 (ChaCha20 bits) or 141 (AES nonce bytes, counter, pt, ct bytes)
// does a key with nK points in K and this commitment flag fit the algorithm's circuit?  (libverify: every proof false if not)
bool key_fits(int algorithm, size_t nK, bool has_commitment);
size_t proof_bytes(bool has_commitment);              // 164 (+32 with a commitment)
// proof length and its commitment count (the big-endian u32 at byte 128) — the checks made before any arithmetic
bool proof_shape_ok(const uint8_t* proof, size_t len, bool has_commitment);
// public inputs in circuit order (verifiers.go): ChaCha20 1152 bits — Counter (LE word), Nonce[3] (LE words), In[16] and Out[16]
// (BE words), bit b of word w at 32 w + b; AES 141 values — Nonce[12] bytes, Counter (BE u32), Plaintext[64], Ciphertext[64]
void public_inputs(int algorithm, const uint8_t sig[kSignalBytes], std::vector<uint32_t>& out);
// the same inputs as 144 byte windows for the device tables: ChaCha20 window j = bits 8j..8j+7 (bit t -> weight 2^t);
// AES window j < 12: nonce byte j, 12..15: counter byte j-12 (little-endian, weight 2^(8(j-12))), 16..143: pt | ct byte
void public_windows(int algorithm, const uint8_t sig[kSignalBytes], uint8_t win[kWindows]);
// the base of window j: ChaCha20 — subset sums of K[1 + 8j + t], t = 0..7; AES — K[1 + input] times 2^shift
void window_base(int algorithm, size_t j, uint32_t& first_k, uint32_t& shift);

// one Verify input ({"cipher","proof","publicSignals"}; keys case-folded, bytes as base64, null or an array of 0..255): false when
// malformed.  algorithm = -1 for an unknown or missing cipher (libverify: false).
bool parse_request(const JsonValue& root, int& algorithm, std::vector<uint8_t>& proof, std::vector<uint8_t>& sig);
extern const char* const kCipherNames[3];

}  // namespace verify
}  // namespace gsc
