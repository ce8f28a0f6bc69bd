// Host check of the key ceremony's walk, splice and record (csrc/phase2.hpp): pure host code, built with g++ from the header and
// csrc/host_ciphers.cpp (SHA-256), also under -fsanitize=address,undefined (tests/test_phase2_host.py) — these are parsers of caller bytes.
//   phase2_check <pk> <vk> [<pk with raw elements>]
// walks the files, then truncations, edited length fields and trailing bytes of both (every buffer an exact heap copy: a read past the end
// is the sanitizer's to find) and expects clean refusals; splices synthetic points in and walks the result; prints facts as name=value lines
// for the test to compare with Python's, and PHASE2-OK.
#include "phase2.hpp"
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

using namespace gsc::phase2;
typedef std::vector<uint8_t> Bytes;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)

static Bytes slurp(const char* path) { std::ifstream f(path, std::ios::binary); return Bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>()); }
static void hex(const char* name, const uint8_t* p, size_t n) { printf("%s=", name); for (size_t i = 0; i < n; i++) printf("%02x", p[i]); printf("\n"); }

// the walk over an exact heap copy of b[0, n)
static bool walk(bool is_pk, const uint8_t* b, size_t n, Walk& w, std::string& err) {
    std::unique_ptr<uint8_t[]> heap(new uint8_t[n ? n : 1]);
    if (n) memcpy(heap.get(), b, n);
    return is_pk ? walk_pk(heap.get(), n, w, err) : walk_vk(heap.get(), n, w, err);
}
static bool elems_inside(const Walk& w, size_t n) {
    for (const std::vector<Elem>* v : {&w.g1, &w.g2}) for (const Elem& e : *v) if (e.off > n || e.size > n - e.off) return false;
    return true;
}

static void malformed(bool is_pk, const Bytes& key, const std::vector<size_t>& count_fields, size_t wires_field) {
    const char* tag = is_pk ? "pk" : "vk";
    Walk w; std::string err;
    // truncations: every length near the ends, a stride through the middle (every length of a small file)
    size_t cuts = 0, refused = 0;
    const size_t n = key.size(), step = n > 100000 ? 4099 : 1;
    for (size_t len = 0; len < n; len += (len < 600 || len + 600 >= n) ? 1 : step) {
        cuts++;
        err.clear();
        if (!walk(is_pk, key.data(), len, w, err) && err.compare(0, 4, std::string(tag) + ": ") == 0) refused++;
    }
    CHECK(cuts == refused);
    printf("%s.truncations=%zu\n", tag, cuts);
    // trailing bytes
    for (size_t extra : {1, 32, 64}) { Bytes t = key; t.resize(n + extra, 0); CHECK(!walk(is_pk, t.data(), t.size(), w, err) ); }
    // every count field: one more, one less, zero, far too large
    size_t edits = 0;
    for (size_t at : count_fields) {
        const uint32_t v = (uint32_t)key[at] << 24 | (uint32_t)key[at + 1] << 16 | (uint32_t)key[at + 2] << 8 | key[at + 3];
        for (uint32_t nv : {v + 1, v - 1, 0u, 0x7FFFFFFFu, 0xFFFFFFFFu, v + 0x01000000u}) {
            if (nv == v) continue;
            Bytes t = key; for (int i = 0; i < 4; i++) t[at + i] = (uint8_t)(nv >> (24 - 8 * i));
            err.clear();
            const bool ok = walk(is_pk, t.data(), t.size(), w, err);
            // an edit may by chance leave a file that still walks (a vk's K count cannot: the bytes are all used); what it must never do is
            // read outside the buffer or report elements that lie outside it
            if (ok) CHECK(elems_inside(w, t.size())); else CHECK(!err.empty());
            if (!is_pk || at != wires_field) CHECK(!ok);
            edits++;
        }
    }
    printf("%s.count_edits=%zu\n", tag, edits);
}

int main(int argc, char** argv) {
    if (argc < 3) { printf("usage: phase2_check <pk> <vk> [<pk with raw elements>]\n"); return 2; }
    const Bytes pk = slurp(argv[1]), vk = slurp(argv[2]);
    Walk wp, wv; std::string err;
    if (!walk_pk(pk.data(), pk.size(), wp, err) || !walk_vk(vk.data(), vk.size(), wv, err)) { printf("REFUSED %s\n", err.c_str()); return 3; }
    printf("pk.g1=%zu\npk.g2=%zu\npk.Z=%zu\npk.K=%zu\nvk.g1=%zu\nvk.g2=%zu\n", wp.g1.size(), wp.g2.size(), wp.nz, wp.nk, wv.g1.size(), wv.g2.size());
    printf("pk.delta1=%zu\npk.delta2=%zu\nvk.delta1=%zu\nvk.delta2=%zu\npk.Z0=%zu\npk.K0=%zu\n", wp.g1[wp.d1].off, wp.g2[wp.d2].off, wv.g1[wv.d1].off, wv.g2[wv.d2].off,
           wp.g1[wp.z0].off, wp.g1[wp.k0].off);
    CHECK(wv.nz == 0 && wv.nk == 0 && wp.k0 == wp.z0 + wp.nz);

    // the count fields of a pk: in front of A, B, Z, K, G2.B; the wire count (a u64: its low word); the commitment key count
    std::vector<size_t> pf;
    const size_t nA = wp.z0 - 3 - (wp.g2.size() - 2);      // g1 = alpha, beta, delta | A | B (as many as G2.B) | Z | K | ...
    pf.push_back(wp.g1[3].off - 4); pf.push_back(wp.g1[3 + nA].off - 4); pf.push_back(wp.g1[wp.z0].off - 4); pf.push_back(wp.g1[wp.k0].off - 4);
    pf.push_back(wp.g2[2].off - 4);
    const Elem& lastB = wp.g2.back();
    const size_t wires = lastB.off + lastB.size + 4;
    pf.push_back(wires);
    malformed(true, pk, pf, wires);
    malformed(false, vk, {wv.g1[3].off - 4, vk.size() - 8, vk.size() - 4}, 0);

    // splice: synthetic points (the compressor copies X and looks at Y only to set the flag), then the result walks with the same counts
    const size_t n1 = 1 + wp.nz + wp.nk;
    Bytes g1(64 * n1), inf(n1, 0), d2(128);
    for (size_t i = 0; i < g1.size(); i++) g1[i] = (uint8_t)(i * 131 + 7);
    for (size_t i = 0; i < n1; i++) { g1[64 * i] &= 0x1F; g1[64 * i + 32] = (i & 1) ? 0x2F : 0x01; }      // x below 2^253; y above / below (p-1)/2 alternately
    for (size_t i = 0; i < 128; i++) d2[i] = (uint8_t)(i + 1);
    d2[0] &= 0x1F; d2[64] = 0x2F;
    inf[2] = 1;
    const Bytes pk2 = splice(pk.data(), pk.size(), wp, g1.data(), inf.data(), d2.data()), vk2 = splice(vk.data(), vk.size(), wv, g1.data(), inf.data(), d2.data());
    Walk wp2, wv2;
    CHECK(walk(true, pk2.data(), pk2.size(), wp2, err) && walk(false, vk2.data(), vk2.size(), wv2, err));
    CHECK(pk2.size() == pk.size() && vk2.size() == vk.size());      // the golden files are compressed throughout
    CHECK(same_outside(pk.data(), pk.size(), wp, pk2.data(), pk2.size(), wp2) && same_outside(vk.data(), vk.size(), wv, vk2.data(), vk2.size(), wv2));
    {
        const uint8_t* e = pk2.data() + wp2.g1[wp2.d1].off;
        CHECK(e[0] == (0x80 | g1[0]) && !memcmp(e + 1, g1.data() + 1, 31));                                   // Delta': y small
        e = pk2.data() + wp2.g1[wp2.z0].off; CHECK(e[0] == (0xC0 | g1[64]) && !memcmp(e + 1, g1.data() + 65, 31));     // Z'[0]: y large
        e = pk2.data() + wp2.g1[wp2.z0 + 1].off; CHECK(e[0] == 0x40 && all_zero(e + 1, 31));                   // Z'[1]: infinity
        e = pk2.data() + wp2.g1[wp2.k0 + wp2.nk - 1].off; CHECK(!memcmp(e + 1, g1.data() + 64 * (n1 - 1) + 1, 31));   // the last K
        e = pk2.data() + wp2.g2[wp2.d2].off; CHECK(e[0] == (0xC0 | d2[0]) && !memcmp(e + 1, d2.data() + 1, 63));
        e = vk2.data() + wv2.g1[wv2.d1].off; CHECK(e[0] == (0x80 | g1[0]) && !memcmp(e + 1, g1.data() + 1, 31));
        e = vk2.data() + wv2.g2[wv2.d2].off; CHECK(e[0] == (0xC0 | d2[0]) && !memcmp(e + 1, d2.data() + 1, 63));
    }
    // rule 2 sees every byte outside delta, Z and K and none inside
    for (size_t at : {(size_t)0, (size_t)9, wp.g1[0].off + 5, wp.g1[3].off + 31, wp.g1[wp.z0].off - 1, wp.g2[0].off, wp.g2[2].off + 63, pk.size() - 1}) {
        Bytes t = pk2; t[at] ^= 1; Walk wt;
        if (walk(true, t.data(), t.size(), wt, err)) CHECK(!same_outside(pk.data(), pk.size(), wp, t.data(), t.size(), wt));
    }
    for (size_t at : {wp.g1[wp.d1].off + 31, wp.g1[wp.z0].off + 31, wp.g1[wp.k0 + wp.nk - 1].off + 31, wp.g2[wp.d2].off + 63}) {
        Bytes t = pk2; t[at] ^= 1; Walk wt;
        CHECK(walk(true, t.data(), t.size(), wt, err) && same_outside(pk.data(), pk.size(), wp, t.data(), t.size(), wt));
    }
    CHECK(!same_outside(pk.data(), pk.size(), wp, vk.data(), vk.size(), wv));
    if (argc > 3) {      // the same key with some elements raw: it walks, rule 2 refuses it against the compressed file, the splice writes compressed
        const Bytes mixed = slurp(argv[3]); Walk wm;
        CHECK(walk(true, mixed.data(), mixed.size(), wm, err));
        CHECK(wm.g1.size() == wp.g1.size() && wm.nz == wp.nz && wm.nk == wp.nk && mixed.size() > pk.size());
        CHECK(!same_outside(pk.data(), pk.size(), wp, mixed.data(), mixed.size(), wm));
        const Bytes m2 = splice(mixed.data(), mixed.size(), wm, g1.data(), inf.data(), d2.data()); Walk wm2;
        CHECK(walk(true, m2.data(), m2.size(), wm2, err) && same_outside(mixed.data(), mixed.size(), wm, m2.data(), m2.size(), wm2));
        size_t raw_left = 0; for (size_t i = 0; i < wm2.g1.size(); i++) if (rewritten_g1(wm2, i) && wm2.g1[i].size != 32) raw_left++;
        CHECK(raw_left == 0 && wm2.g2[wm2.d2].size == 64);
        Bytes s1; slots(mixed.data(), wm.g1, 32, s1);
        CHECK(s1.size() == 64 * wm.g1.size());
        printf("mixed.bytes=%zu\nmixed.spliced=%zu\n", mixed.size(), m2.size());
    }

    // the record, its challenge, the seeded scalars, the Schnorr equation's addition
    Record r;
    for (int i = 0; i < 32; i++) { r.h_prev[i] = (uint8_t)i; r.h_next[i] = (uint8_t)(32 + i); r.z[i] = (uint8_t)(200 + i); }
    for (int i = 0; i < 64; i++) { r.delta[i] = (uint8_t)(64 + i); r.T[i] = (uint8_t)(128 + i); }
    uint8_t rec[kRecordBytes], c[32];
    encode_record(r, rec);
    for (size_t i = 0; i < kRecordBytes; i++) CHECK(rec[i] == (uint8_t)(i < 192 ? i : 200 + (i - 192)));
    const Record back = decode_record(rec);
    CHECK(!memcmp(&back, &r, sizeof r));
    uint8_t dprev[64]; for (int i = 0; i < 64; i++) dprev[i] = (uint8_t)(255 - i);
    challenge(r.h_prev, dprev, r.delta, r.T, c);
    hex("challenge", c, 32);
    uint8_t seed[32]; for (int i = 0; i < 32; i++) seed[i] = (uint8_t)(3 * i + 1);
    gsc::hostf::Fr x; uint8_t xb[32];
    CHECK(seeded_scalar("gsc-phase2-x", seed, x)); x.to_be(xb); hex("seeded.x", xb, 32);
    CHECK(seeded_scalar("gsc-phase2-k", seed, x)); x.to_be(xb); hex("seeded.k", xb, 32);
    uint8_t G[64] = {0}, G2[64], G3[64], N[64], O[64] = {0}, out[64];
    G[31] = 1; G[63] = 2;
    CHECK(g1_add_raw(G, G, G2)); hex("G+G", G2, 64);
    CHECK(g1_add_raw(G, G2, G3)); hex("G+2G", G3, 64);
    CHECK(g1_add_raw(G2, G, out) && !memcmp(out, G3, 64));
    memcpy(N, G, 64); { gsc::hostf::Fp y; gsc::hostf::Fp::from_be(G + 32, y); y.neg().to_be(N + 32); }
    CHECK(g1_add_raw(G, N, out) && all_zero(out, 64));
    CHECK(g1_add_raw(G, O, out) && !memcmp(out, G, 64) && g1_add_raw(O, G3, out) && !memcmp(out, G3, 64));
    memset(out, 0xFF, 64); CHECK(!g1_add_raw(out, G, G2));      // coordinates not below p

    if (failures) { printf("%d check(s) failed\n", failures); return 1; }
    printf("PHASE2-OK\n");
    return 0;
}
