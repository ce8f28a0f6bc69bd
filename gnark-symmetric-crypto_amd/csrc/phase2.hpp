// Key ceremony, second phase: the host side of gsc_setup_contribute / gsc_setup_verify_contribution.  Pure host code, no
// HIP and no device: tests/native/phase2_check.cpp builds it with g++ (also under -fsanitize=address,undefined) — these are parsers of
// caller bytes.
//
// A contribution re-randomises delta with a secret x: G1.Delta' = x G1.Delta, G2.Delta' = x G2.Delta (pk and vk), G1.Z'[k] = x^-1 G1.Z[k],
// G1.K'[i] = x^-1 G1.K[i] (pk); every other byte of both files stays.  Here: the walk that finds those elements in gnark's pk / vk layouts
// (each element compressed or raw, as formats.hpp walk_points reads them), the comparison of everything else, the
// splice that writes the new file, and the record.
//
// THE RECORD IS THIS PROJECT'S OWN FORMAT, 224 bytes.  It is NOT gnark's mpcsetup transcript and not compatible with it.
//   0..31    SHA-256(pk_prev)
//   32..63   SHA-256(pk_next)
//   64..127  G1.Delta' raw, X | Y big-endian
//   128..191 T = k G1.Delta_prev raw, big-endian
//   192..223 z = k + c x mod r, big-endian           (a Schnorr proof of knowledge of x over the base G1.Delta_prev)
// c = the first 31 bytes, as a big-endian integer, of SHA-256("gsc-phase2-v1" | SHA-256(pk_prev) | Delta_prev raw | Delta' raw | T raw).
#pragma once
#include "host_ciphers.hpp"
#include "host_field.hpp"
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace gsc {
namespace phase2 {

constexpr size_t kRecordBytes = 224;

struct Elem { size_t off = 0, size = 0; };      // one point of a key file: where it lies and how many bytes it takes
// Every point of a key file in file order, G1 and G2 apart, and which of them a contribution rewrites.
struct Walk {
    std::vector<Elem> g1, g2;
    size_t d1 = 0, d2 = 0;                      // G1.Delta in g1, G2.Delta in g2
    size_t z0 = 0, nz = 0, k0 = 0, nk = 0;      // pk: G1.Z = g1[z0, z0 + nz), G1.K = g1[k0, k0 + nk); a vk has neither (its K is gamma's, untouched)
    // the one commitment key, when the file has it (sigma.hpp).  pk: Basis = g1[pb0, pb0 + npb), BasisExpSigma =
    // g1[ps0, ps0 + npb); vk: G = g2[pg], GSigmaNeg = g2[pgsn]
    bool ped = false, vk = false;               // vk: walk_vk made this walk
    size_t pb0 = 0, ps0 = 0, npb = 0, pg = 0, pgsn = 0;
};

namespace detail {
struct Cur {
    const uint8_t* b; size_t n, i = 0; bool ok = true;
    Cur(const uint8_t* p, size_t len) : b(p), n(len) {}
    bool take(size_t k, size_t& at) { if (!ok || k > n - i) { ok = false; return false; } at = i; i += k; return true; }
    uint64_t be(size_t bytes) { size_t at; if (!take(bytes, at)) return 0; uint64_t v = 0; for (size_t j = 0; j < bytes; j++) v = (v << 8) | b[at + j]; return v; }
    bool point(size_t cb, std::vector<Elem>& out) {
        if (!ok || i >= n) { ok = false; return false; }
        const size_t sz = (b[i] & 0xC0) == 0 ? 2 * cb : cb;
        size_t at; if (!take(sz, at)) return false;
        out.push_back(Elem{at, sz}); return true;
    }
    // a u32 count, then that many points; a count the data cannot hold is refused before anything is allocated for it
    bool slice(size_t cb, std::vector<Elem>& out, size_t& count) {
        count = (size_t)be(4);
        if (!ok || count > (n - i) / cb) { ok = false; return false; }
        for (size_t k = 0; k < count; k++) if (!point(cb, out)) return false;
        return true;
    }
};
inline bool fail(std::string& err, const char* m) { err = m; return false; }
}  // namespace detail

// groth16.ProvingKey.WriteTo / WriteRawTo layout, with the refusals of formats.cpp parse_pk
inline bool walk_pk(const uint8_t* b, size_t n, Walk& w, std::string& err) {
    w = Walk(); detail::Cur c(b, n);
    const uint64_t domain = c.be(8);
    if (!c.ok || domain == 0 || (domain & (domain - 1)) || domain > (1ull << 28)) return detail::fail(err, "pk: bad domain size");
    size_t at, na, nb, nb2;
    if (!c.take(5 * 32 + 1, at)) return detail::fail(err, "pk: truncated");
    if (!c.point(32, w.g1) || !c.point(32, w.g1)) return detail::fail(err, "pk: truncated");
    w.d1 = w.g1.size();
    if (!c.point(32, w.g1)) return detail::fail(err, "pk: truncated");
    if (!c.slice(32, w.g1, na) || !c.slice(32, w.g1, nb)) return detail::fail(err, "pk: truncated");
    w.z0 = w.g1.size(); if (!c.slice(32, w.g1, w.nz)) return detail::fail(err, "pk: truncated");
    w.k0 = w.g1.size(); if (!c.slice(32, w.g1, w.nk)) return detail::fail(err, "pk: truncated");
    if (!c.point(64, w.g2)) return detail::fail(err, "pk: truncated");
    w.d2 = w.g2.size();
    if (!c.point(64, w.g2) || !c.slice(64, w.g2, nb2)) return detail::fail(err, "pk: truncated");
    const uint64_t nw = c.be(8); c.be(8); c.be(8);
    if (!c.ok || nw > (n - c.i) / 2) return detail::fail(err, "pk: truncated");
    if (!c.take((size_t)(2 * nw), at)) return detail::fail(err, "pk: truncated");
    size_t fa = 0, fb = 0;
    for (size_t i = 0; i < nw; i++) { fa += !b[at + i]; fb += !b[at + nw + i]; }
    const uint64_t nck = c.be(4);
    if (!c.ok) return detail::fail(err, "pk: truncated");
    if (nck > 1) return detail::fail(err, "pk: more than one commitment key is not supported");
    if (nck == 1) {
        size_t c0, c1;
        w.pb0 = w.g1.size(); if (!c.slice(32, w.g1, c0)) return detail::fail(err, "pk: truncated");
        w.ps0 = w.g1.size(); if (!c.slice(32, w.g1, c1)) return detail::fail(err, "pk: truncated");
        if (c0 != c1) return detail::fail(err, "pk: commitment key size mismatch");
        w.ped = true; w.npb = c0;
    }
    if (c.i != n) return detail::fail(err, "pk: trailing bytes");
    if (fa != na || fb != nb || nb != nb2 || w.nz != domain - 1) return detail::fail(err, "pk: inconsistent slice sizes");
    return true;
}

// groth16.VerifyingKey.WriteTo / WriteRawTo layout, with the refusals of verify_common.cpp parse_vk_layout
inline bool walk_vk(const uint8_t* b, size_t n, Walk& w, std::string& err) {
    w = Walk(); w.vk = true; detail::Cur c(b, n);
    size_t nk;
    if (!c.point(32, w.g1) || !c.point(32, w.g1) || !c.point(64, w.g2) || !c.point(64, w.g2)) return detail::fail(err, "vk: truncated");
    w.d1 = w.g1.size(); w.d2 = w.g2.size();
    if (!c.point(32, w.g1) || !c.point(64, w.g2)) return detail::fail(err, "vk: truncated");
    if (!c.slice(32, w.g1, nk)) return detail::fail(err, "vk: truncated inside K");
    const uint64_t outer = c.be(4);
    if (!c.ok) return detail::fail(err, "vk: truncated");
    if (outer > 1) return detail::fail(err, "vk: more than one commitment");
    for (uint64_t o = 0; o < outer; o++) { const uint64_t pc = c.be(4); if (!c.ok) return detail::fail(err, "vk: truncated"); if (pc) return detail::fail(err, "vk: public committed wires are not supported"); }
    const uint64_t nck = c.be(4);
    if (!c.ok) return detail::fail(err, "vk: truncated");
    if (nck != outer) return detail::fail(err, "vk: commitment key count");
    if (nck) {
        w.pg = w.g2.size(); w.pgsn = w.pg + 1; w.ped = true;
        if (!c.point(64, w.g2) || !c.point(64, w.g2)) return detail::fail(err, "vk: truncated");
    }
    if (c.i != n) return detail::fail(err, "vk: trailing bytes");
    return true;
}

// is g1[i] one of the elements a contribution rewrites?  (Of g2 it is g2[d2] alone.)
inline bool rewritten_g1(const Walk& w, size_t i) { return i == w.d1 || (i >= w.z0 && i < w.z0 + w.nz) || (i >= w.k0 && i < w.k0 + w.nk); }

// the points of one group as the device decoders take them: slots of 2 cb bytes, a compressed element in the first half of its slot
inline void slots(const uint8_t* b, const std::vector<Elem>& el, size_t cb, std::vector<uint8_t>& out) {
    out.assign(el.size() * 2 * cb, 0);
    for (size_t i = 0; i < el.size(); i++) memcpy(out.data() + 2 * cb * i, b + el[i].off, el[i].size);
}

// Outside the elements that a step rewrites — in1(w, i) for g1[i], in2(w, i) for g2[i] — b equals a byte for byte, with the same element
// counts and marks.  (So a key whose untouched points were re-encoded — raw for compressed or back — is refused although it holds the same
// points.)
template <class In1, class In2>
inline bool same_outside_of(const uint8_t* a, size_t an, const Walk& wa, const uint8_t* b, size_t bn, const Walk& wb, In1 in1, In2 in2) {
    if (wa.g1.size() != wb.g1.size() || wa.g2.size() != wb.g2.size() || wa.nz != wb.nz || wa.nk != wb.nk || wa.z0 != wb.z0 || wa.k0 != wb.k0 ||
        wa.d1 != wb.d1 || wa.d2 != wb.d2 || wa.ped != wb.ped || wa.vk != wb.vk || wa.pb0 != wb.pb0 || wa.ps0 != wb.ps0 || wa.npb != wb.npb || wa.pg != wb.pg ||
        wa.pgsn != wb.pgsn) return false;
    // the rewritten elements in file order cut each file into the same number of gaps; every gap must match.  Each group's elements lie in
    // file order; the two groups interleave (a pk: G1 sets, G2 sets, the commitment key's G1 sets), so the two lists are merged by offset.
    std::vector<Elem> ca, cb;
    size_t i1 = 0, i2 = 0;
    const size_t n1 = wa.g1.size(), n2 = wa.g2.size();
    while (i1 < n1 || i2 < n2) {
        const bool first = i2 >= n2 || (i1 < n1 && wa.g1[i1].off < wa.g2[i2].off);
        if (first) { if (in1(wa, i1)) { ca.push_back(wa.g1[i1]); cb.push_back(wb.g1[i1]); } i1++; }
        else { if (in2(wa, i2)) { ca.push_back(wa.g2[i2]); cb.push_back(wb.g2[i2]); } i2++; }
    }
    size_t ia = 0, ib = 0;
    for (size_t k = 0; k < ca.size(); k++) {
        if (ca[k].off < ia || cb[k].off < ib || ca[k].off - ia != cb[k].off - ib || memcmp(a + ia, b + ib, ca[k].off - ia)) return false;
        ia = ca[k].off + ca[k].size; ib = cb[k].off + cb[k].size;
    }
    return an - ia == bn - ib && !memcmp(a + ia, b + ib, an - ia);
}
// Rule 2 of a delta step: the rewritten elements are G1.Delta, Z, K and G2.Delta
inline bool same_outside(const uint8_t* a, size_t an, const Walk& wa, const uint8_t* b, size_t bn, const Walk& wb) {
    return same_outside_of(a, an, wa, b, bn, wb, rewritten_g1, [](const Walk& w, size_t i) { return i == w.d2; });
}

// (p-1)/2 big-endian: a compressed point carries the "larger y" flag iff y > (p-1)/2
inline bool be_greater_than_half_p(const uint8_t* y) {
    static const uint8_t h[32] = {0x18, 0x32, 0x27, 0x39, 0x70, 0x98, 0xd0, 0x14, 0xdc, 0x28, 0x22, 0xdb, 0x40, 0xc0, 0xac, 0x2e,
                                  0xcb, 0xc0, 0xb5, 0x48, 0xb4, 0x38, 0xe5, 0x46, 0x9e, 0x10, 0x46, 0x0b, 0x6c, 0x3e, 0x7e, 0xa3};
    return memcmp(y, h, 32) > 0;
}
inline bool all_zero(const uint8_t* p, size_t n) { uint8_t o = 0; for (size_t i = 0; i < n; i++) o |= p[i]; return o == 0; }
// gnark-crypto compressed encodings from raw big-endian coordinates (G1: X | Y; G2: X.A1 | X.A0 | Y.A1 | Y.A0)
inline void compress_g1(const uint8_t* raw, bool inf, uint8_t out[32]) {
    if (inf) { memset(out, 0, 32); out[0] = 0x40; return; }
    memcpy(out, raw, 32); out[0] |= be_greater_than_half_p(raw + 32) ? 0xC0 : 0x80;
}
inline void compress_g2(const uint8_t* raw, bool inf, uint8_t out[64]) {
    if (inf) { memset(out, 0, 64); out[0] = 0x40; return; }
    memcpy(out, raw, 64);
    const bool large = all_zero(raw + 64, 32) ? be_greater_than_half_p(raw + 96) : be_greater_than_half_p(raw + 64);
    out[0] |= large ? 0xC0 : 0x80;
}

// The new file: key with its rewritten elements replaced, compressed, by the points new_g1 (64 B raw each, in the order the walk meets the
// rewritten G1 elements: Delta, Z..., K...) / new_d2 (128 B raw); inf1[i] != 0: the point at infinity.
inline std::vector<uint8_t> splice(const uint8_t* key, size_t n, const Walk& w, const uint8_t* new_g1, const uint8_t* inf1, const uint8_t* new_d2) {
    std::vector<uint8_t> out; out.reserve(n);
    size_t at = 0, j = 0;
    for (size_t i = 0; i < w.g1.size(); i++) if (rewritten_g1(w, i)) {
        out.insert(out.end(), key + at, key + w.g1[i].off); at = w.g1[i].off + w.g1[i].size;
        uint8_t e[32]; compress_g1(new_g1 + 64 * j, inf1[j] != 0, e); out.insert(out.end(), e, e + 32); j++;
    }
    const Elem& d2 = w.g2[w.d2];
    out.insert(out.end(), key + at, key + d2.off); at = d2.off + d2.size;
    uint8_t e[64]; compress_g2(new_d2, false, e); out.insert(out.end(), e, e + 64);
    out.insert(out.end(), key + at, key + n);
    return out;
}

// ---- the record ----
struct Record { uint8_t h_prev[32], h_next[32], delta[64], T[64], z[32]; };
inline void encode_record(const Record& r, uint8_t out[kRecordBytes]) {
    memcpy(out, r.h_prev, 32); memcpy(out + 32, r.h_next, 32); memcpy(out + 64, r.delta, 64); memcpy(out + 128, r.T, 64); memcpy(out + 192, r.z, 32);
}
inline Record decode_record(const uint8_t in[kRecordBytes]) {
    Record r; memcpy(r.h_prev, in, 32); memcpy(r.h_next, in + 32, 32); memcpy(r.delta, in + 64, 64); memcpy(r.T, in + 128, 64); memcpy(r.z, in + 192, 32);
    return r;
}
// c as 32 big-endian bytes (byte 0 is zero: c < 2^248 < r): the first 31 bytes of SHA-256(tag | h_prev | base | next | T), tag at most 16 bytes
inline void challenge_tagged(const char* tag, const uint8_t h_prev[32], const uint8_t base[64], const uint8_t next[64], const uint8_t T[64], uint8_t c_be[32]) {
    uint8_t msg[16 + 32 + 3 * 64], h[32];
    size_t ln = strlen(tag); if (ln > 16) ln = 16;
    memcpy(msg, tag, ln); memcpy(msg + ln, h_prev, 32); memcpy(msg + ln + 32, base, 64); memcpy(msg + ln + 96, next, 64); memcpy(msg + ln + 160, T, 64);
    sha256_digest(msg, ln + 32 + 3 * 64, h);
    c_be[0] = 0; memcpy(c_be + 1, h, 31);
}
inline void challenge(const uint8_t h_prev[32], const uint8_t delta_prev[64], const uint8_t delta_next[64], const uint8_t T[64], uint8_t c_be[32]) {
    challenge_tagged("gsc-phase2-v1", h_prev, delta_prev, delta_next, T, c_be);
}
// a scalar of a seeded (TEST) contribution: SHA-256(label | seed32) as a big-endian integer mod r; false when that is zero
inline bool seeded_scalar(const char* label, const uint8_t seed32[32], hostf::Fr& out) {
    uint8_t msg[64], h[32]; const size_t ln = strlen(label);
    if (ln > 32) return false;
    memcpy(msg, label, ln); memcpy(msg + ln, seed32, 32);
    sha256_digest(msg, ln + 32, h);
    hostf::Fr acc = hostf::Fr::zero(); const hostf::Fr k = hostf::Fr::from_u64(256);
    for (int i = 0; i < 32; i++) acc = acc * k + hostf::Fr::from_u64(h[i]);
    explicit_bzero(msg, sizeof msg); explicit_bzero(h, sizeof h);
    out = acc;
    return !acc.is_zero();
}

// ---- the Schnorr equation's one addition: affine G1 points as raw big-endian X | Y, all-zero = infinity; false for coordinates >= p ----
inline bool g1_add_raw(const uint8_t a[64], const uint8_t b[64], uint8_t out[64]) {
    using hostf::Fp;
    const bool ia = all_zero(a, 64), ib = all_zero(b, 64);
    Fp ax, ay, bx, by;
    if ((!ia && (!Fp::from_be(a, ax) || !Fp::from_be(a + 32, ay))) || (!ib && (!Fp::from_be(b, bx) || !Fp::from_be(b + 32, by)))) return false;
    if (ia) { memcpy(out, b, 64); return true; }
    if (ib) { memcpy(out, a, 64); return true; }
    Fp lam;
    if (ax == bx) {
        if (!(ay == by) || ay.is_zero()) { memset(out, 0, 64); return true; }
        lam = (ax.sq() + ax.sq() + ax.sq()) * (ay + ay).inv();
    } else lam = (by - ay) * (bx - ax).inv();
    const Fp x3 = lam.sq() - ax - bx, y3 = lam * (ax - x3) - ay;
    x3.to_be(out); y3.to_be(out + 32);
    return true;
}

}  // namespace phase2
}  // namespace gsc
