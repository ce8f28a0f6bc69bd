#include "verify_common.hpp"
#include <cstdlib>
#include <cstring>

namespace gsc {
namespace verify {

uint32_t be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

bool parse_vk_layout(const uint8_t* b, size_t n, VkLayout& vk, std::string* err) {
    size_t i = 0;
    auto fail = [&](const char* m) { if (err) *err = m; return false; };
    auto take = [&](size_t k, size_t& at) { if (k > n - i) return false; at = i; i += k; return true; };
    // one point as gnark's decoder reads it: flag bits 00 in its first byte -> raw, X | Y (2 x cb bytes), anything else -> cb bytes
    auto point = [&](size_t cb, size_t& at) { if (i >= n) return false; return take(point_is_raw(b + i) ? 2 * cb : cb, at); };
    size_t at;
    if (!point(32, vk.alpha) || !point(32, vk.g1_beta) || !point(64, vk.beta) || !point(64, vk.gamma) || !point(32, vk.g1_delta) || !point(64, vk.delta)) return fail("vk: truncated");
    if (!take(4, at)) return fail("vk: truncated");
    const uint32_t nk = be32(b + at);
    if ((size_t)nk > (n - i) / 32) return fail("vk: K count exceeds the key");
    vk.K.resize(nk);
    for (auto& k : vk.K) if (!point(32, k)) return fail("vk: truncated inside K");
    if (!take(4, at)) return fail("vk: truncated");
    const uint32_t outer = be32(b + at);
    if (outer > 1) return fail("vk: more than one commitment");
    for (uint32_t o = 0; o < outer; o++) {
        if (!take(4, at)) return fail("vk: truncated");
        if (be32(b + at)) return fail("vk: public committed wires are not supported");
    }
    if (!take(4, at)) return fail("vk: truncated");
    const uint32_t nck = be32(b + at);
    if (nck != outer) return fail("vk: commitment key count");
    vk.has_commitment = nck != 0;
    if (nck && (!point(64, vk.ped_g) || !point(64, vk.ped_gsn))) return fail("vk: truncated");
    if (i != n) return fail("vk: trailing bytes");
    return true;
}

size_t num_public(int algorithm) { return algorithm == 0 ? kChachaInputs : kAesInputs; }
bool key_fits(int algorithm, size_t nK, bool has_commitment) {
    if (algorithm == 0) return !has_commitment && nK == 1 + kChachaInputs;
    return nK == 1 + kAesInputs + (has_commitment ? 1 : 0);
}
size_t proof_bytes(bool has_commitment) { return 164 + (has_commitment ? 32 : 0); }
bool proof_shape_ok(const uint8_t* proof, size_t len, bool has_commitment) {
    return len == proof_bytes(has_commitment) && be32(proof + 128) == (has_commitment ? 1u : 0u);
}

void public_inputs(int algorithm, const uint8_t sig[kSignalBytes], std::vector<uint32_t>& out) {
    const uint8_t *ct = sig, *nonce = sig + 64, *ctr = sig + 76, *pt = sig + 80;
    out.clear();
    if (algorithm == 0) {
        auto word = [](const uint8_t* p, bool be) { return be ? be32(p) : (uint32_t)p[3] << 24 | (uint32_t)p[2] << 16 | (uint32_t)p[1] << 8 | p[0]; };
        std::vector<uint32_t> words;
        words.push_back(word(ctr, false));
        for (int i = 0; i < 3; i++) words.push_back(word(nonce + 4 * i, false));
        for (int i = 0; i < 16; i++) words.push_back(word(pt + 4 * i, true));
        for (int i = 0; i < 16; i++) words.push_back(word(ct + 4 * i, true));
        for (uint32_t w : words) for (int bit = 0; bit < 32; bit++) out.push_back((w >> bit) & 1);
    } else {
        for (int i = 0; i < 12; i++) out.push_back(nonce[i]);
        out.push_back(be32(ctr));
        for (int i = 0; i < 64; i++) out.push_back(pt[i]);
        for (int i = 0; i < 64; i++) out.push_back(ct[i]);
    }
}

void public_windows(int algorithm, const uint8_t sig[kSignalBytes], uint8_t win[kWindows]) {
    std::vector<uint32_t> v;
    public_inputs(algorithm, sig, v);
    if (algorithm == 0) {
        for (size_t j = 0; j < kWindows; j++) { uint32_t b = 0; for (int t = 0; t < 8; t++) b |= v[8 * j + t] << t; win[j] = (uint8_t)b; }
    } else {
        for (size_t j = 0; j < 12; j++) win[j] = (uint8_t)v[j];
        for (size_t j = 0; j < 4; j++) win[12 + j] = (uint8_t)(v[12] >> (8 * j));
        for (size_t j = 16; j < kWindows; j++) win[j] = (uint8_t)v[j - 3];
    }
}

void window_base(int algorithm, size_t j, uint32_t& first_k, uint32_t& shift) {
    if (algorithm == 0) { first_k = (uint32_t)(1 + 8 * j); shift = 0; return; }
    if (j < 12) { first_k = (uint32_t)(1 + j); shift = 0; }
    else if (j < 16) { first_k = 1 + 12; shift = (uint32_t)(8 * (j - 12)); }
    else { first_k = (uint32_t)(1 + j - 3); shift = 0; }
}

const char* const kCipherNames[3] = {"chacha20", "aes-128-ctr", "aes-256-ctr"};

static bool bytes_field(const JsonValue& v, std::vector<uint8_t>& out) {
    if (v.kind == JsonValue::String) { size_t bad; return base64_decode(v.text, out, bad); }
    if (v.kind == JsonValue::Null) { out.clear(); return true; }
    if (v.kind != JsonValue::Array) return false;
    out.clear();
    for (auto& e : v.items) { if (e.kind != JsonValue::Number || e.text.find_first_not_of("0123456789") != std::string::npos || e.text.size() > 3 || atoi(e.text.c_str()) > 255) return false; out.push_back((uint8_t)atoi(e.text.c_str())); }
    return true;
}
static bool fold_eq(const std::string& a, const char* b) { if (a.size() != strlen(b)) return false; for (size_t i = 0; i < a.size(); i++) if ((a[i] | 32) != (b[i] | 32)) return false; return true; }

bool parse_request(const JsonValue& root, int& algorithm, std::vector<uint8_t>& proof, std::vector<uint8_t>& sig) {
    algorithm = -1;
    if (root.kind != JsonValue::Object) return false;
    std::string cipher;
    for (auto& kv : root.members) {
        if (fold_eq(kv.first, "cipher")) { if (kv.second.kind == JsonValue::String) cipher = kv.second.text; else if (kv.second.kind != JsonValue::Null) return false; }
        else if (fold_eq(kv.first, "proof")) { if (!bytes_field(kv.second, proof)) return false; }
        else if (fold_eq(kv.first, "publicSignals")) { if (!bytes_field(kv.second, sig)) return false; }
    }
    for (int k = 0; k < 3; k++) if (cipher == kCipherNames[k]) algorithm = k;
    return true;
}

}  // namespace verify
}  // namespace gsc
