// Key ceremony: the Pedersen sigma of a commitment key, distributed: the host side of gsc_pedersen_verify /
// gsc_setup_contribute_sigma / gsc_setup_verify_sigma_contribution / gsc_setup_verify_from_srs.  Pure host code, no HIP and no device, on top
// of phase2.hpp's walk (its marks pb0 / ps0 / npb / pg / pgsn): tests/native/sigma_check.cpp builds it with g++ (also under
// -fsanitize=address,undefined) — these are parsers of caller bytes.
//
// A sigma contribution with a secret x rewrites pk's BasisExpSigma'[j] = x BasisExpSigma[j] and vk's GSigmaNeg' = x GSigmaNeg; every other
// byte of both files stays (Basis, G, delta, Z, K ...), so sigma steps and delta steps may interleave: each copies what the other rewrites.
//
// THE RECORD IS THIS PROJECT'S OWN FORMAT, 224 bytes, the phase-2 record's layout under another tag:
//   0..31    SHA-256(pk_prev)
//   32..63   SHA-256(pk_next)
//   64..127  new  = next's BasisExpSigma[j0] raw, X | Y big-endian      (j0: the lowest index whose element is finite)
//   128..191 T    = k base raw, base = prev's BasisExpSigma[j0]
//   192..223 z    = k + c x mod r, big-endian                            (a Schnorr proof of knowledge of x over base)
// c = the first 31 bytes, as a big-endian integer, of SHA-256("gsc-sigma-v1" | SHA-256(pk_prev) | base raw | new raw | T raw).  The tag
// differs from phase 2's, so a delta record never passes as a sigma record.
#pragma once
#include "phase2.hpp"

namespace gsc {
namespace sigma {

using phase2::Elem;
using phase2::Walk;
constexpr size_t kRecordBytes = 224;

// the elements a sigma step rewrites: of a pk BasisExpSigma, of a vk GSigmaNeg
inline bool sigma_g1(const Walk& w, size_t i) { return w.ped && !w.vk && i >= w.ps0 && i < w.ps0 + w.npb; }
inline bool sigma_g2(const Walk& w, size_t i) { return w.ped && w.vk && i == w.pgsn; }
// rule 2 of a sigma step
inline bool same_outside_sigma(const uint8_t* a, size_t an, const Walk& wa, const uint8_t* b, size_t bn, const Walk& wb) {
    return phase2::same_outside_of(a, an, wa, b, bn, wb, sigma_g1, sigma_g2);
}
// rule 1 of gsc_setup_verify_from_srs: a production Setup draws sigma and g afresh, so pk's BasisExpSigma and vk's G and GSigmaNeg are
// outside the comparison (a circuit without a commitment: nothing is)
inline bool same_outside_fresh(const uint8_t* a, size_t an, const Walk& wa, const uint8_t* b, size_t bn, const Walk& wb) {
    return phase2::same_outside_of(a, an, wa, b, bn, wb, sigma_g1, [](const Walk& w, size_t i) { return w.ped && w.vk && (i == w.pg || i == w.pgsn); });
}

// is this element the point at infinity?  (Of a file whose points the device has decoded: a compressed infinity with stray bits is refused there.)
inline bool is_infinity(const uint8_t* key, const Elem& e) {
    const uint8_t f = key[e.off] & 0xC0;
    return f == 0x40 || (f == 0 && phase2::all_zero(key + e.off, e.size));
}
// What rule 1 of gsc_pedersen_verify asks of a pair beyond the walks and the decoding of every point.  Empty: accepted; else the reason.
// with_infinities = false leaves out the clause on the infinities' positions (gsc_setup_verify_sigma_contribution reports it on next under
// its rule 3: given rule 1 on prev and rule 2 it is the same statement).
inline std::string pair_shape(const uint8_t* pk, const Walk& wp, const uint8_t* vk, const Walk& wv, bool with_infinities = true) {
    if (!wp.ped || !wv.ped) return "no commitment key";
    if (is_infinity(vk, wv.g2[wv.pg]) || is_infinity(vk, wv.g2[wv.pgsn])) return "G or GSigmaNeg is the point at infinity";
    if (!with_infinities) return std::string();
    bool finite = false;
    for (size_t j = 0; j < wp.npb; j++) {
        const bool ib = is_infinity(pk, wp.g1[wp.pb0 + j]), is = is_infinity(pk, wp.g1[wp.ps0 + j]);
        if (ib != is) return "Basis and BasisExpSigma have their infinities at different positions";
        finite = finite || !ib;
    }
    if (!finite) return "the commitment key has no finite element";
    return std::string();
}
// j0: the lowest index whose BasisExpSigma element is finite; npb when there is none
inline size_t first_finite(const uint8_t* pk, const Walk& wp) {
    size_t j = 0;
    while (j < wp.npb && is_infinity(pk, wp.g1[wp.ps0 + j])) j++;
    return j;
}
// rule 3's last clause
inline bool same_infinities(const uint8_t* a, const Walk& wa, const uint8_t* b, const Walk& wb) {
    if (wa.npb != wb.npb) return false;
    for (size_t j = 0; j < wa.npb; j++) if (is_infinity(a, wa.g1[wa.ps0 + j]) != is_infinity(b, wb.g1[wb.ps0 + j])) return false;
    return true;
}

// The new pk: BasisExpSigma replaced, compressed, by new_sigma (64 B raw each; inf[j] != 0: the point at infinity).
inline std::vector<uint8_t> splice_pk(const uint8_t* pk, size_t n, const Walk& w, const uint8_t* new_sigma, const uint8_t* inf) {
    std::vector<uint8_t> out; out.reserve(n);
    size_t at = 0;
    for (size_t j = 0; j < w.npb; j++) {
        const Elem& e = w.g1[w.ps0 + j];
        out.insert(out.end(), pk + at, pk + e.off); at = e.off + e.size;
        uint8_t c[32]; phase2::compress_g1(new_sigma + 64 * j, inf[j] != 0, c); out.insert(out.end(), c, c + 32);
    }
    out.insert(out.end(), pk + at, pk + n);
    return out;
}
// The new vk: GSigmaNeg replaced, compressed, by new_gsn (128 B raw, finite).
inline std::vector<uint8_t> splice_vk(const uint8_t* vk, size_t n, const Walk& w, const uint8_t* new_gsn) {
    const Elem& e = w.g2[w.pgsn];
    std::vector<uint8_t> out(vk, vk + e.off);
    uint8_t c[64]; phase2::compress_g2(new_gsn, false, c); out.insert(out.end(), c, c + 64);
    out.insert(out.end(), vk + e.off + e.size, vk + n);
    return out;
}

// ---- the record: phase 2's layout (its field `delta` holds `new`) under a tag of its own ----
using phase2::Record;
using phase2::encode_record;
using phase2::decode_record;
inline void challenge(const uint8_t h_prev[32], const uint8_t base[64], const uint8_t next[64], const uint8_t T[64], uint8_t c_be[32]) {
    phase2::challenge_tagged("gsc-sigma-v1", h_prev, base, next, T, c_be);
}
// the scalars of a seeded (TEST) contribution; false when one is zero
inline bool seeded_scalars(const uint8_t seed32[32], hostf::Fr& x, hostf::Fr& k) {
    return phase2::seeded_scalar("gsc-sigma-x", seed32, x) && phase2::seeded_scalar("gsc-sigma-k", seed32, k);
}
// -P for a raw finite G1 point; false for coordinates >= p
inline bool g1_neg_raw(const uint8_t a[64], uint8_t out[64]) {
    hostf::Fp y;
    if (phase2::all_zero(a, 64)) { memset(out, 0, 64); return true; }
    if (!hostf::Fp::from_be(a + 32, y)) return false;
    memcpy(out, a, 32); y.neg().to_be(out + 32);
    return true;
}

}  // namespace sigma
}  // namespace gsc
