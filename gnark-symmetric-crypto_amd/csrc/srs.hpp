// Powers file: the result of a phase-1 ceremony as gsc_srs_verify reads it.  Pure host code, no HIP and no device:
// tests/native/srs_check.cpp builds it with g++ (also under -fsanitize=address,undefined) — this is a parser of caller bytes.
//
// THE FILE IS THIS PROJECT'S OWN FORMAT, version 1.  It is NOT snarkjs' .ptau and NOT gnark's mpcsetup format: neither can be pinned
// without those tools, and a converter is not part of the library.
//
//   "gscsrs01" (8 B) | u32 big-endian L | tauG1[0 .. 2N-2] | tauG2[0 .. N-1] | alphaG1[0 .. N-1] | betaG1[0 .. N-1] | betaG2        N = 2^L
//
//   tauG1[i] = tau^i G1, tauG2[i] = tau^i G2, alphaG1[i] = alpha tau^i G1, betaG1[i] = beta tau^i G1, betaG2 = beta G2.
// Every element is raw (flag bits 00; G1: 64 B X | Y, G2: 128 B X.A1 | X.A0 | Y.A1 | Y.A0, big-endian), the raw encoding formats.cpp and
// the verifier's key-point kernel read.  No compressed element and no point at infinity is admitted.  1 <= L <= 24, and the length of
// the file is the one L gives, exactly.
//
// Here: the bounds and section offsets (walk), the elements of each group as the fixed-stride vectors the decoder kernel takes (slots), the
// generators and the one writer (assemble).  Whether the elements are points, and the powers they claim to be, is the device's part
// (srs_gpu.cpp); the ceremony that makes such a file is srs_contrib.hpp / srs_contrib_gpu.cpp.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace gsc {
namespace srs {

constexpr uint8_t kMagic[8] = {'g', 's', 'c', 's', 'r', 's', '0', '1'};
constexpr int kMinLog = 1, kMaxLog = 24;
constexpr size_t kHeaderBytes = 12, kG1Bytes = 64, kG2Bytes = 128;

// Where the sections lie.  G1 elements are numbered tauG1 | alphaG1 | betaG1 and G2 elements tauG2 | betaG2: the order of slots().
struct Layout {
    int L = 0; size_t N = 0;
    size_t off_tau1 = 0, off_tau2 = 0, off_alpha1 = 0, off_beta1 = 0, off_beta2 = 0, bytes = 0;      // byte offsets in the file
    size_t n_tau1() const { return 2 * N - 1; }
    size_t n_g1() const { return 4 * N - 1; }      // 2N-1 + N + N
    size_t n_g2() const { return N + 1; }
    size_t i_alpha1() const { return 2 * N - 1; }  // alphaG1[0] among the G1 elements
    size_t i_beta1() const { return 3 * N - 1; }   // betaG1[0]
    size_t i_beta2() const { return N; }           // betaG2 among the G2 elements
};

// the layout of a file with N = 2^L; false outside 1 <= L <= 24
inline bool layout_of(int L, Layout& o) {
    if (L < kMinLog || L > kMaxLog) return false;
    o = Layout(); o.L = L; o.N = (size_t)1 << L;
    o.off_tau1 = kHeaderBytes;
    o.off_tau2 = o.off_tau1 + kG1Bytes * (2 * o.N - 1);
    o.off_alpha1 = o.off_tau2 + kG2Bytes * o.N;
    o.off_beta1 = o.off_alpha1 + kG1Bytes * o.N;
    o.off_beta2 = o.off_beta1 + kG1Bytes * o.N;
    o.bytes = o.off_beta2 + kG2Bytes;            // L = 24: 6.4 GB, far inside size_t
    return true;
}

// "tauG1[5]" for G1 element 5, "alphaG1[0]" for element 2N-1, ...
inline std::string g1_name(const Layout& l, size_t i) {
    if (i < l.i_alpha1()) return "tauG1[" + std::to_string(i) + "]";
    if (i < l.i_beta1()) return "alphaG1[" + std::to_string(i - l.i_alpha1()) + "]";
    return "betaG1[" + std::to_string(i - l.i_beta1()) + "]";
}
inline std::string g2_name(const Layout& l, size_t i) { return i < l.i_beta2() ? "tauG2[" + std::to_string(i) + "]" : std::string("betaG2"); }
// the file offset of G1 element i / G2 element i
inline size_t g1_offset(const Layout& l, size_t i) {
    if (i < l.i_alpha1()) return l.off_tau1 + kG1Bytes * i;
    if (i < l.i_beta1()) return l.off_alpha1 + kG1Bytes * (i - l.i_alpha1());
    return l.off_beta1 + kG1Bytes * (i - l.i_beta1());
}
inline size_t g2_offset(const Layout& l, size_t i) { return i < l.i_beta2() ? l.off_tau2 + kG2Bytes * i : l.off_beta2; }

namespace detail {
inline bool fail(std::string& err, const std::string& m) { err = m; return false; }
inline bool all_zero(const uint8_t* p, size_t n) { uint8_t o = 0; for (size_t i = 0; i < n; i++) o |= p[i]; return o == 0; }
}  // namespace detail

// Magic, L, the exact length; then every element's flag bits (00: raw) and that none is the all-zero encoding of the point at infinity.
// Reads nothing beyond b[0, n).  err names what was wrong, and for an element which one.
inline bool walk(const uint8_t* b, size_t n, Layout& l, std::string& err) {
    l = Layout();
    if (!b || n < kHeaderBytes) return detail::fail(err, "srs: truncated header");
    if (memcmp(b, kMagic, 8)) return detail::fail(err, "srs: not a powers file (magic)");
    const uint32_t L = (uint32_t)b[8] << 24 | (uint32_t)b[9] << 16 | (uint32_t)b[10] << 8 | b[11];
    if (L < (uint32_t)kMinLog || L > (uint32_t)kMaxLog || !layout_of((int)L, l)) return detail::fail(err, "srs: L outside [1, 24]");
    if (n < l.bytes) return detail::fail(err, "srs: truncated (the length does not match L)");
    if (n > l.bytes) return detail::fail(err, "srs: trailing bytes (the length does not match L)");
    for (size_t i = 0; i < l.n_g1(); i++) {
        const uint8_t* e = b + g1_offset(l, i);
        if (e[0] & 0xC0) return detail::fail(err, "srs: " + g1_name(l, i) + " is not a raw element");
        if (detail::all_zero(e, kG1Bytes)) return detail::fail(err, "srs: " + g1_name(l, i) + " is the point at infinity");
    }
    for (size_t i = 0; i < l.n_g2(); i++) {
        const uint8_t* e = b + g2_offset(l, i);
        if (e[0] & 0xC0) return detail::fail(err, "srs: " + g2_name(l, i) + " is not a raw element");
        if (detail::all_zero(e, kG2Bytes)) return detail::fail(err, "srs: " + g2_name(l, i) + " is the point at infinity");
    }
    return true;
}

// the elements of a walked file as the decoder kernel takes them: g1 = tauG1 | alphaG1 | betaG1 in 64-byte slots, g2 = tauG2 | betaG2 in
// 128-byte slots
inline void slots(const uint8_t* b, const Layout& l, std::vector<uint8_t>& g1, std::vector<uint8_t>& g2) {
    g1.resize(kG1Bytes * l.n_g1()); g2.resize(kG2Bytes * l.n_g2());
    memcpy(g1.data(), b + l.off_tau1, kG1Bytes * l.n_tau1());
    memcpy(g1.data() + kG1Bytes * l.i_alpha1(), b + l.off_alpha1, kG1Bytes * l.N);
    memcpy(g1.data() + kG1Bytes * l.i_beta1(), b + l.off_beta1, kG1Bytes * l.N);
    memcpy(g2.data(), b + l.off_tau2, kG2Bytes * l.N);
    memcpy(g2.data() + kG2Bytes * l.i_beta2(), b + l.off_beta2, kG2Bytes);
}

// the generators, raw big-endian: G1 (1, 2); G2 as gnark-crypto has it
inline void generators(uint8_t g1[64], uint8_t g2[128]) {
    static const char* const hex[4] = {"198e9393920d483a7260bfb731fb5d25f1aa493335a9e71297e485b7aef312c2", "1800deef121f1e76426a00665e5c4479674322d4f75edadd46debd5cd992f6ed",
                                       "090689d0585ff075ec9e99ad690c3395bc4b313370b38ef355acdadcd122975b", "12c85ea5db8c6deb4aab71808dcb408fe3d1e7690c43d37b4ce6cc0166fa7daa"};
    memset(g1, 0, 64); g1[31] = 1; g1[63] = 2;
    for (int c = 0; c < 4; c++) for (int i = 0; i < 32; i++) {
        auto nib = [](char ch) { return ch <= '9' ? ch - '0' : ch - 'a' + 10; };
        g2[32 * c + i] = (uint8_t)(nib(hex[c][2 * i]) << 4 | nib(hex[c][2 * i + 1]));
    }
}

// the file for its elements in slots() order (the one writer: gsc_debug_srs_generate, gsc_srs_initial and gsc_srs_contribute use it)
inline std::vector<uint8_t> assemble(const Layout& l, const uint8_t* g1, const uint8_t* g2) {
    std::vector<uint8_t> f(l.bytes);
    memcpy(f.data(), kMagic, 8);
    f[8] = (uint8_t)(l.L >> 24); f[9] = (uint8_t)(l.L >> 16); f[10] = (uint8_t)(l.L >> 8); f[11] = (uint8_t)l.L;
    memcpy(f.data() + l.off_tau1, g1, kG1Bytes * l.n_tau1());
    memcpy(f.data() + l.off_alpha1, g1 + kG1Bytes * l.i_alpha1(), kG1Bytes * l.N);
    memcpy(f.data() + l.off_beta1, g1 + kG1Bytes * l.i_beta1(), kG1Bytes * l.N);
    memcpy(f.data() + l.off_tau2, g2, kG2Bytes * l.N);
    memcpy(f.data() + l.off_beta2, g2 + kG2Bytes * l.i_beta2(), kG2Bytes);
    return f;
}

}  // namespace srs
}  // namespace gsc
