// Key ceremony, first phase: the host side of gsc_srs_initial / gsc_srs_contribute / gsc_srs_verify_contribution.  Pure
// host code, no HIP and no device: tests/native/srs_contrib_check.cpp builds it with g++ (also under -fsanitize=address,undefined) — the
// record is caller bytes.
//
// A contribution to a powers file (srs.hpp) multiplies the file's scalars by secrets tau', alpha', beta' in [1, r):
//   tauG1'[i] = tau'^i tauG1[i], tauG2'[i] = tau'^i tauG2[i], alphaG1'[i] = alpha' tau'^i alphaG1[i], betaG1'[i] = beta' tau'^i betaG1[i],
//   betaG2' = beta' betaG2,
// so the new file holds the powers of (tau tau', alpha alpha', beta beta').  The ceremony starts from the file of tau = alpha = beta = 1
// (initial): every element a generator, a deterministic function of L.
//
// THE RECORD IS THIS PROJECT'S OWN FORMAT, 544 bytes, like the 224-byte phase-2 record (phase2.hpp).
//   0..31    SHA-256(prev)
//   32..63   SHA-256(next)
//   then, for s = tau, alpha, beta in that order (160 bytes each, at 64, 224, 384):
//     new_s raw (64)                            next's tauG1[1] / alphaG1[0] / betaG1[0]
//     T_s = k_s base_s raw (64)                 base_s: prev's tauG1[1] / alphaG1[0] / betaG1[0]
//     z_s = k_s + c_s s' mod r, big-endian (32) a Schnorr proof of knowledge of s' with new_s = s' base_s
// c_s = the first 31 bytes, as a big-endian integer, of
//   SHA-256("gsc-phase1-v1" | one byte 0 / 1 / 2 for tau / alpha / beta | SHA-256(prev) | base_s raw | new_s raw | T_s raw).
#pragma once
#include "phase2.hpp"
#include "srs.hpp"

namespace gsc {
namespace srsc {

constexpr size_t kRecordBytes = 544, kProofBytes = 160;
constexpr int kTau = 0, kAlpha = 1, kBeta = 2;
inline const char* name_of(int s) { return s == kTau ? "tau" : s == kAlpha ? "alpha" : "beta"; }

struct Proof { uint8_t elem[64], T[64], z[32]; };      // new_s, T_s, z_s
struct Record { uint8_t h_prev[32], h_next[32]; Proof s[3]; };

inline void encode_record(const Record& r, uint8_t out[kRecordBytes]) {
    memcpy(out, r.h_prev, 32); memcpy(out + 32, r.h_next, 32);
    for (int s = 0; s < 3; s++) {
        uint8_t* o = out + 64 + kProofBytes * s;
        memcpy(o, r.s[s].elem, 64); memcpy(o + 64, r.s[s].T, 64); memcpy(o + 128, r.s[s].z, 32);
    }
}
inline Record decode_record(const uint8_t in[kRecordBytes]) {
    Record r;
    memcpy(r.h_prev, in, 32); memcpy(r.h_next, in + 32, 32);
    for (int s = 0; s < 3; s++) {
        const uint8_t* o = in + 64 + kProofBytes * s;
        memcpy(r.s[s].elem, o, 64); memcpy(r.s[s].T, o + 64, 64); memcpy(r.s[s].z, o + 128, 32);
    }
    return r;
}

// c_s as 32 big-endian bytes (byte 0 is zero: c < 2^248 < r)
inline void challenge(int s, const uint8_t h_prev[32], const uint8_t base[64], const uint8_t elem[64], const uint8_t T[64], uint8_t c_be[32]) {
    static const char tag[] = "gsc-phase1-v1";
    uint8_t msg[13 + 1 + 32 + 3 * 64], h[32];
    memcpy(msg, tag, 13); msg[13] = (uint8_t)s; memcpy(msg + 14, h_prev, 32); memcpy(msg + 46, base, 64); memcpy(msg + 110, elem, 64); memcpy(msg + 174, T, 64);
    sha256_digest(msg, sizeof msg, h);
    c_be[0] = 0; memcpy(c_be + 1, h, 31);
}

// The scalars of a seeded (TEST) contribution: secret s' = SHA-256("gsc-phase1-<s>" | seed) mod r, nonce k_s = SHA-256("gsc-phase1-k-<s>" | seed)
// mod r (phase2.hpp's seeded_scalar).  False when one of them is zero.
inline bool seeded_scalars(int s, const uint8_t seed32[32], hostf::Fr& secret, hostf::Fr& nonce) {
    const std::string a = std::string("gsc-phase1-") + name_of(s), b = std::string("gsc-phase1-k-") + name_of(s);
    const bool ok1 = phase2::seeded_scalar(a.c_str(), seed32, secret), ok2 = phase2::seeded_scalar(b.c_str(), seed32, nonce);
    return ok1 && ok2;
}

// what rule 4 asks of a record's T and z before any device work: T raw (flag bits 00) and not the all-zero encoding of infinity; z below r
inline bool T_is_raw_and_finite(const uint8_t T[64]) { return !(T[0] & 0xC0) && !phase2::all_zero(T, 64); }
inline bool z_below_r(const uint8_t z[32], hostf::Fr& out) { return hostf::Fr::from_be(z, out); }

// The ceremony's starting file for N = 2^L: every G1 element the G1 generator, every G2 element the G2 generator.  False outside 1 <= L <= 24.
inline bool initial(int L, std::vector<uint8_t>& out) {
    srs::Layout l;
    out.clear();
    if (!srs::layout_of(L, l)) return false;
    uint8_t G1[64], G2[128];
    srs::generators(G1, G2);
    std::vector<uint8_t> g1(srs::kG1Bytes * l.n_g1()), g2(srs::kG2Bytes * l.n_g2());
    for (size_t i = 0; i < l.n_g1(); i++) memcpy(g1.data() + srs::kG1Bytes * i, G1, 64);
    for (size_t i = 0; i < l.n_g2(); i++) memcpy(g2.data() + srs::kG2Bytes * i, G2, 128);
    out = srs::assemble(l, g1.data(), g2.data());
    return true;
}

}  // namespace srsc
}  // namespace gsc
