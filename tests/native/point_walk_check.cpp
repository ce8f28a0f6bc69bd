// Host check of the key-point walk (csrc/formats.hpp walk_points, parse_pk): pure host code, built with g++ from csrc/formats.cpp, also
// under -fsanitize=address,undefined (tests/test_point_walk_host.py) — these are parsers of caller bytes.
//   point_walk_check self              synthetic slices; prints WALK-OK
//   point_walk_check pk <in> <out>     parse_pk(<in>); every point set dumped to <out> as
//                                      u32 name length | name | u64 points | u64 x bytes | x | u64 y bytes | y   (little-endian)
//                                      a refused key: "REFUSED <message>" on stdout, exit status 3
#include "formats.hpp"
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <stdexcept>
#include <string>
#include <vector>

using gsc::walk_points;
typedef std::vector<uint8_t> Bytes;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)

// element k of a synthetic slice: every byte tells its element and position, the flag bits say the form
static Bytes element(size_t cb, size_t k, bool raw) {
    Bytes e(raw ? 2 * cb : cb);
    for (size_t i = 0; i < e.size(); i++) e[i] = (uint8_t)(17 * k + 3 * i + 1);
    e[0] = (uint8_t)((e[0] & 0x3F) | (raw ? 0x00 : (k & 1 ? 0xC0 : 0x80)));
    return e;
}
static std::string refused(const uint8_t* p, size_t len, size_t count, size_t cb) {
    Bytes x, y;
    try { walk_points(p, len, count, cb, x, y, "t"); } catch (const std::runtime_error& e) { return e.what(); }
    return "";
}

// pattern: 0 all compressed, 1 all raw, 2 alternating from compressed, 3 alternating from raw, 4 raw at the last index only
static void one_slice(size_t cb, size_t n, int pattern) {
    std::vector<bool> raw(n);
    for (size_t k = 0; k < n; k++) raw[k] = pattern == 1 || (pattern == 2 && (k & 1)) || (pattern == 3 && !(k & 1)) || (pattern == 4 && k + 1 == n);
    bool any = false; for (size_t k = 0; k < n; k++) any = any || raw[k];
    Bytes buf; std::vector<Bytes> el;
    for (size_t k = 0; k < n; k++) { el.push_back(element(cb, k, raw[k])); buf.insert(buf.end(), el[k].begin(), el[k].end()); }
    // an exact heap copy: a read past the end is the sanitizer's to find
    uint8_t* heap = new uint8_t[buf.size() ? buf.size() : 1]; if (!buf.empty()) memcpy(heap, buf.data(), buf.size());
    Bytes x(3, 9), y(5, 9);
    const size_t used = walk_points(heap, buf.size(), n, cb, x, y, "t");
    CHECK(used == buf.size());
    CHECK(x.size() == n * cb);
    CHECK(any ? y.size() == n * cb : y.empty());
    for (size_t k = 0; k < n; k++) {
        CHECK(!memcmp(x.data() + k * cb, el[k].data(), cb));
        if (any) {
            Bytes want(cb, 0); if (raw[k]) want.assign(el[k].begin() + cb, el[k].end());
            CHECK(!memcmp(y.data() + k * cb, want.data(), cb));
        }
    }
    // the same bytes with something behind them: the walk stops after n elements
    Bytes more(buf); more.push_back(0xAA); more.push_back(0x00);
    CHECK(walk_points(more.data(), more.size(), n, cb, x, y, "t") == buf.size());
    // every proper prefix ends before or inside an element (n > 0): refused, message in the caller's style
    for (size_t cut = 0; cut < buf.size(); cut++) {
        uint8_t* h2 = new uint8_t[cut ? cut : 1]; if (cut) memcpy(h2, buf.data(), cut);
        const std::string msg = refused(h2, cut, n, cb);
        CHECK(!msg.empty() && msg.compare(0, 3, "t: ") == 0);
        delete[] h2;
    }
    // a count the bytes cannot hold
    CHECK(!refused(heap, buf.size(), n + 1, cb).empty());
    CHECK(!refused(heap, buf.size(), buf.size() / cb + 1, cb).empty());
    CHECK(!refused(heap, buf.size(), (size_t)0xFFFFFFFFu, cb).empty());
    delete[] heap;
}

static int self_test() {
    for (size_t cb : {(size_t)32, (size_t)64})
        for (size_t n : {(size_t)0, (size_t)1, (size_t)2, (size_t)5})
            for (int pattern = 0; pattern < 5; pattern++) one_slice(cb, n, pattern);
    {   // truncation in the middle of a raw element, by name: 2 compressed, then a raw one cut after its X
        Bytes buf; for (size_t k = 0; k < 3; k++) { Bytes e = element(32, k, k == 2); buf.insert(buf.end(), e.begin(), e.end()); }
        buf.resize(2 * 32 + 32 + 7);
        const std::string msg = refused(buf.data(), buf.size(), 3, 32);
        CHECK(msg.find("inside point 2") != std::string::npos);
    }
    {   // parse_pk itself: nothing but a header
        Bytes tiny(8 + 5 * 32 + 1, 0); tiny[7] = 8;
        bool threw = false;
        try { gsc::parse_pk(tiny.data(), tiny.size()); } catch (const std::runtime_error& e) { threw = std::string(e.what()).compare(0, 4, "pk: ") == 0; }
        CHECK(threw);
    }
    if (failures) return 1;
    printf("WALK-OK\n");
    return 0;
}

static void put(std::ofstream& f, uint64_t v, int n) { for (int i = 0; i < n; i++) f.put((char)(v >> (8 * i))); }

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "self")) return self_test();
    if (argc == 4 && !strcmp(argv[1], "pk")) {
        std::ifstream in(argv[2], std::ios::binary);
        if (!in) { printf("cannot read %s\n", argv[2]); return 2; }
        const Bytes file((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        uint8_t* heap = new uint8_t[file.size() ? file.size() : 1]; if (!file.empty()) memcpy(heap, file.data(), file.size());
        try {
            const gsc::PkFile pk = gsc::parse_pk(heap, file.size());
            std::ofstream out(argv[3], std::ios::binary);
            struct Set { const char* name; size_t cb; const Bytes* x; const Bytes* y; };
            const Set sets[] = {{"g1.alpha", 32, &pk.g1_alpha, &pk.g1_alpha_y}, {"g1.beta", 32, &pk.g1_beta, &pk.g1_beta_y}, {"g1.delta", 32, &pk.g1_delta, &pk.g1_delta_y},
                                {"g1.A", 32, &pk.g1_A, &pk.g1_A_y}, {"g1.B", 32, &pk.g1_B, &pk.g1_B_y}, {"g1.Z", 32, &pk.g1_Z, &pk.g1_Z_y}, {"g1.K", 32, &pk.g1_K, &pk.g1_K_y},
                                {"g2.beta", 64, &pk.g2_beta, &pk.g2_beta_y}, {"g2.delta", 64, &pk.g2_delta, &pk.g2_delta_y}, {"g2.B", 64, &pk.g2_B, &pk.g2_B_y},
                                {"ped.basis", 32, &pk.ped_basis, &pk.ped_basis_y}, {"ped.sigma", 32, &pk.ped_basis_sigma, &pk.ped_basis_sigma_y}};
            for (const Set& s : sets) {
                put(out, strlen(s.name), 4); out.write(s.name, (std::streamsize)strlen(s.name));
                put(out, s.x->size() / s.cb, 8);
                put(out, s.x->size(), 8); out.write((const char*)s.x->data(), (std::streamsize)s.x->size());
                put(out, s.y->size(), 8); out.write((const char*)s.y->data(), (std::streamsize)s.y->size());
            }
            printf("PARSED domain %llu wires %llu\n", (unsigned long long)pk.domain_n, (unsigned long long)pk.n_wires);
        } catch (const std::runtime_error& e) { printf("REFUSED %s\n", e.what()); delete[] heap; return 3; }
        delete[] heap;
        return 0;
    }
    printf("usage: point_walk_check self | pk <in> <out>\n");
    return 2;
}
