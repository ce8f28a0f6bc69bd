// Host check of the first phase's record, challenge, seeded scalars and starting file (csrc/srs_contrib.hpp): pure host code, built with g++
// from the header and csrc/host_ciphers.cpp (SHA-256), also under -fsanitize=address,undefined (tests/test_srs_contrib_host.py) — the record
// is caller bytes.
//   srs_contrib_check <out dir>
// encodes and decodes a record (every buffer an exact heap copy: a read past the end is the sanitizer's to find), prints the three challenges and
// the seeded scalars as name=value lines for the test to compare with Python's, checks what rule 4 asks of z and T before any device work,
// writes initial(L) for L = 1, 2, 3 into <out dir>/initial.<L>, and prints SRSC-OK.
#include "srs_contrib.hpp"
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

using namespace gsc::srsc;
typedef std::vector<uint8_t> Bytes;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)

static void hex(const std::string& name, const uint8_t* p, size_t n) { printf("%s=", name.c_str()); for (size_t i = 0; i < n; i++) printf("%02x", p[i]); printf("\n"); }

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: srs_contrib_check <out dir>\n"); return 2; }
    static_assert(kRecordBytes == 544 && kRecordBytes == 64 + 3 * kProofBytes, "the record's size");

    // the record: byte i of the encoding is i (mod 256) when the fields are filled in layout order
    Record r;
    {
        size_t at = 0;
        auto fill = [&](uint8_t* p, size_t n) { for (size_t i = 0; i < n; i++) p[i] = (uint8_t)(at++); };
        fill(r.h_prev, 32); fill(r.h_next, 32);
        for (int s = 0; s < 3; s++) { fill(r.s[s].elem, 64); fill(r.s[s].T, 64); fill(r.s[s].z, 32); }
        CHECK(at == kRecordBytes);
    }
    std::unique_ptr<uint8_t[]> rec(new uint8_t[kRecordBytes]);
    encode_record(r, rec.get());
    for (size_t i = 0; i < kRecordBytes; i++) CHECK(rec[i] == (uint8_t)i);
    const Record back = decode_record(rec.get());
    CHECK(!memcmp(back.h_prev, r.h_prev, 32) && !memcmp(back.h_next, r.h_next, 32));
    for (int s = 0; s < 3; s++) CHECK(!memcmp(back.s[s].elem, r.s[s].elem, 64) && !memcmp(back.s[s].T, r.s[s].T, 64) && !memcmp(back.s[s].z, r.s[s].z, 32));
    std::unique_ptr<uint8_t[]> rec2(new uint8_t[kRecordBytes]);
    encode_record(back, rec2.get());
    CHECK(!memcmp(rec.get(), rec2.get(), kRecordBytes));
    CHECK(std::string(name_of(kTau)) == "tau" && std::string(name_of(kAlpha)) == "alpha" && std::string(name_of(kBeta)) == "beta");

    // the challenges of the three proofs over that record's fields and a base of bytes 255 - i
    uint8_t base[64], c[32];
    for (int i = 0; i < 64; i++) base[i] = (uint8_t)(255 - i);
    for (int s = 0; s < 3; s++) {
        challenge(s, r.h_prev, base, r.s[s].elem, r.s[s].T, c);
        CHECK(c[0] == 0);
        hex(std::string("challenge.") + name_of(s), c, 32);
    }

    // the seeded scalars
    uint8_t seed[32]; for (int i = 0; i < 32; i++) seed[i] = (uint8_t)(3 * i + 1);
    for (int s = 0; s < 3; s++) {
        gsc::hostf::Fr x, k; uint8_t b[32];
        CHECK(seeded_scalars(s, seed, x, k));
        x.to_be(b); hex(std::string("seeded.") + name_of(s), b, 32);
        k.to_be(b); hex(std::string("seeded.k.") + name_of(s), b, 32);
    }

    // z: below r or refused.  r - 1 and 0 pass, r, r + 1 and 2^256 - 1 do not
    static const uint8_t r_be[32] = {0x30, 0x64, 0x4e, 0x72, 0xe1, 0x31, 0xa0, 0x29, 0xb8, 0x50, 0x45, 0xb6, 0x81, 0x81, 0x58, 0x5d,
                                     0x28, 0x33, 0xe8, 0x48, 0x79, 0xb9, 0x70, 0x91, 0x43, 0xe1, 0xf5, 0x93, 0xf0, 0x00, 0x00, 0x01};
    {
        gsc::hostf::Fr z; uint8_t v[32], b[32];
        memcpy(v, r_be, 32); CHECK(!z_below_r(v, z));
        v[31] = 0x02; CHECK(!z_below_r(v, z));
        v[31] = 0x00; CHECK(z_below_r(v, z)); z.to_be(b); CHECK(!memcmp(b, v, 32));
        memset(v, 0xFF, 32); CHECK(!z_below_r(v, z));
        memset(v, 0, 32); CHECK(z_below_r(v, z) && z.is_zero());
    }
    // T: raw and finite or refused
    {
        std::unique_ptr<uint8_t[]> T(new uint8_t[64]);
        memset(T.get(), 0, 64); CHECK(!T_is_raw_and_finite(T.get()));                       // all zero: the point at infinity
        T[63] = 2; T[31] = 1; CHECK(T_is_raw_and_finite(T.get()));                          // the generator
        for (uint8_t flag : {0x40, 0x80, 0xC0}) { T[0] = flag; CHECK(!T_is_raw_and_finite(T.get())); }      // compressed / infinity flag bits
        T[0] = 0x3F; CHECK(T_is_raw_and_finite(T.get()));                                   // whether it is a point is the device's part
        memset(T.get(), 0, 64); T[63] = 1; CHECK(T_is_raw_and_finite(T.get()));
    }

    // the starting file
    for (int L : {0, -1, 25, 1 << 20}) { Bytes f(3, 7); CHECK(!initial(L, f) && f.empty()); }
    for (int L = 1; L <= 3; L++) {
        Bytes f;
        CHECK(initial(L, f));
        gsc::srs::Layout l; std::string err;
        CHECK(gsc::srs::walk(f.data(), f.size(), l, err) && l.L == L && f.size() == l.bytes);
        std::ofstream o(std::string(argv[1]) + "/initial." + std::to_string(L), std::ios::binary);
        o.write((const char*)f.data(), (std::streamsize)f.size());
        printf("initial.%d=%zu\n", L, f.size());
    }

    if (failures) { printf("%d check(s) failed\n", failures); return 1; }
    printf("SRSC-OK\n");
    return 0;
}
