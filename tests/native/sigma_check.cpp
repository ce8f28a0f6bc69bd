// Host check of the sigma ceremony's host side (csrc/sigma.hpp on csrc/phase2.hpp): pure host code, built with g++ from the headers and
// csrc/host_ciphers.cpp (SHA-256), also under -fsanitize=address,undefined (tests/test_sigma_host.py) — these are parsers of caller bytes.
//   sigma_check <small pk> <small vk> <pk> <vk> <pk without commitment> <vk without commitment> [<small pk, some elements raw> <small vk, raw>]
// The small pair (tests/sigmamodel.py) gets every truncation and every edited count of its commitment-key tail (every buffer an exact heap
// copy: a read past the end is the sanitizer's to find); the walk's marks of all pairs are printed as name=value lines for the test to
// compare with Python's; the splice, rule 2's comparison (against a restatement of phase 2's own, as it was before it took a predicate), the
// record, the challenge and the seeded scalars; then SIGMA-OK.
#include "sigma.hpp"
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

using namespace gsc::phase2;
namespace S = gsc::sigma;
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

// phase 2's rule 2 as it stood before same_outside_of: the reference of the generalised comparison on phase 2's element set
static bool reference_same_outside(const uint8_t* a, size_t an, const Walk& wa, const uint8_t* b, size_t bn, const Walk& wb) {
    if (wa.g1.size() != wb.g1.size() || wa.g2.size() != wb.g2.size() || wa.nz != wb.nz || wa.nk != wb.nk || wa.z0 != wb.z0 || wa.k0 != wb.k0 ||
        wa.d1 != wb.d1 || wa.d2 != wb.d2) return false;
    std::vector<Elem> ca, cb;
    for (size_t i = 0; i < wa.g1.size(); i++) if (rewritten_g1(wa, i)) { ca.push_back(wa.g1[i]); cb.push_back(wb.g1[i]); }
    ca.push_back(wa.g2[wa.d2]); cb.push_back(wb.g2[wb.d2]);
    size_t ia = 0, ib = 0;
    for (size_t k = 0; k < ca.size(); k++) {
        if (ca[k].off < ia || cb[k].off < ib || ca[k].off - ia != cb[k].off - ib || memcmp(a + ia, b + ib, ca[k].off - ia)) return false;
        ia = ca[k].off + ca[k].size; ib = cb[k].off + cb[k].size;
    }
    return an - ia == bn - ib && !memcmp(a + ia, b + ib, an - ia);
}

static void marks(const char* tag, const Walk& wp, const Walk& wv) {
    printf("%s.pk.ped=%d\n%s.vk.ped=%d\n", tag, (int)wp.ped, tag, (int)wv.ped);
    if (wp.ped) {
        printf("%s.pk.n=%zu\n", tag, wp.npb);
        if (wp.npb) printf("%s.pk.basis0=%zu\n%s.pk.sigma0=%zu\n%s.pk.basis_last=%zu\n%s.pk.sigma_last=%zu\n", tag, wp.g1[wp.pb0].off, tag, wp.g1[wp.ps0].off,
                           tag, wp.g1[wp.pb0 + wp.npb - 1].off, tag, wp.g1[wp.ps0 + wp.npb - 1].off);
        CHECK(wp.ps0 == wp.pb0 + wp.npb && wp.ps0 + wp.npb == wp.g1.size() && !wp.vk);
    }
    if (wv.ped) {
        printf("%s.vk.g=%zu\n%s.vk.gsn=%zu\n", tag, wv.g2[wv.pg].off, tag, wv.g2[wv.pgsn].off);
        CHECK(wv.pgsn == wv.pg + 1 && wv.pgsn + 1 == wv.g2.size() && wv.vk);
    }
}

// every truncation of key from `from` on, and every edit of the count fields: clean refusals
static void malformed(bool is_pk, const Bytes& key, size_t from, const std::vector<size_t>& count_fields) {
    const char* tag = is_pk ? "pk" : "vk";
    Walk w; std::string err;
    size_t cuts = 0, refused = 0;
    for (size_t len = from; len < key.size(); len++) {
        cuts++; err.clear();
        if (!walk(is_pk, key.data(), len, w, err) && err.compare(0, 4, std::string(tag) + ": ") == 0) refused++;
    }
    CHECK(cuts == refused);
    printf("%s.truncations=%zu\n", tag, cuts);
    for (size_t extra : {1, 32, 64}) { Bytes t = key; t.resize(key.size() + extra, 0); CHECK(!walk(is_pk, t.data(), t.size(), w, err)); }
    size_t edits = 0;
    for (size_t at : count_fields) {
        const uint32_t v = (uint32_t)key[at] << 24 | (uint32_t)key[at + 1] << 16 | (uint32_t)key[at + 2] << 8 | key[at + 3];
        for (uint32_t nv : {v + 1, v - 1, 0u, 2u, 0x7FFFFFFFu, 0xFFFFFFFFu, v + 0x01000000u}) {
            if (nv == v) continue;
            Bytes t = key; for (int i = 0; i < 4; i++) t[at + i] = (uint8_t)(nv >> (24 - 8 * i));
            err.clear();
            const bool ok = walk(is_pk, t.data(), t.size(), w, err);
            if (ok) CHECK(elems_inside(w, t.size())); else CHECK(!err.empty());
            CHECK(!ok);
            edits++;
        }
    }
    printf("%s.count_edits=%zu\n", tag, edits);
}

int main(int argc, char** argv) {
    if (argc < 7) { printf("usage: sigma_check <small pk> <small vk> <pk> <vk> <pk without commitment> <vk without commitment> [<small pk raw> <small vk raw>]\n"); return 2; }
    const Bytes pk = slurp(argv[1]), vk = slurp(argv[2]);
    Walk wp, wv; std::string err;
    if (!walk_pk(pk.data(), pk.size(), wp, err) || !walk_vk(vk.data(), vk.size(), wv, err)) { printf("REFUSED %s\n", err.c_str()); return 3; }
    marks("small", wp, wv);
    printf("small.pk.g1=%zu\nsmall.pk.g2=%zu\nsmall.vk.g1=%zu\nsmall.vk.g2=%zu\n", wp.g1.size(), wp.g2.size(), wv.g1.size(), wv.g2.size());
    CHECK(wp.ped && wv.ped && wp.npb > 0);
    CHECK(S::pair_shape(pk.data(), wp, vk.data(), wv).empty());
    printf("small.j0=%zu\n", S::first_finite(pk.data(), wp));
    size_t infs = 0; for (size_t j = 0; j < wp.npb; j++) infs += S::is_infinity(pk.data(), wp.g1[wp.ps0 + j]);
    printf("small.infinities=%zu\n", infs);
    {
        const Bytes bpk = slurp(argv[3]), bvk = slurp(argv[4]), npk = slurp(argv[5]), nvk = slurp(argv[6]);
        Walk a, b;
        CHECK(walk_pk(bpk.data(), bpk.size(), a, err) && walk_vk(bvk.data(), bvk.size(), b, err));
        marks("big", a, b);
        CHECK(S::pair_shape(bpk.data(), a, bvk.data(), b).empty());
        CHECK(walk_pk(npk.data(), npk.size(), a, err) && walk_vk(nvk.data(), nvk.size(), b, err));
        marks("none", a, b);
        CHECK(S::pair_shape(npk.data(), a, nvk.data(), b) == "no commitment key");
        // a pair without a commitment: nothing is outside the comparison
        CHECK(S::same_outside_fresh(npk.data(), npk.size(), a, npk.data(), npk.size(), a) && S::same_outside_sigma(nvk.data(), nvk.size(), b, nvk.data(), nvk.size(), b));
        Bytes t = npk; t[t.size() - 40] ^= 1; Walk c;
        if (walk_pk(t.data(), t.size(), c, err)) CHECK(!S::same_outside_fresh(npk.data(), npk.size(), a, t.data(), t.size(), c));
    }

    // the commitment-key tail: pk from the key count on (u32 nck | u32 n | Basis | u32 n | BasisExpSigma), vk from the outer count on
    const size_t pk_tail = wp.g1[wp.pb0].off - 8, vk_tail = wv.g2[wv.pg].off - 12;
    malformed(true, pk, pk_tail, {pk_tail, pk_tail + 4, wp.g1[wp.ps0].off - 4});
    malformed(false, vk, vk_tail, {vk_tail, vk_tail + 4, vk_tail + 8});

    // splice: synthetic points (the compressor copies X and looks at Y only to set the flag), then the result walks with the same marks
    const size_t n = wp.npb;
    Bytes g1(64 * n), inf(n, 0), gsn(128);
    for (size_t i = 0; i < g1.size(); i++) g1[i] = (uint8_t)(i * 131 + 7);
    for (size_t i = 0; i < n; i++) { g1[64 * i] &= 0x1F; g1[64 * i + 32] = (i & 1) ? 0x2F : 0x01; inf[i] = S::is_infinity(pk.data(), wp.g1[wp.ps0 + i]); }
    for (size_t i = 0; i < 128; i++) gsn[i] = (uint8_t)(i + 1);
    gsn[0] &= 0x1F; gsn[64] = 0x2F;
    const Bytes pk2 = S::splice_pk(pk.data(), pk.size(), wp, g1.data(), inf.data()), vk2 = S::splice_vk(vk.data(), vk.size(), wv, gsn.data());
    Walk wp2, wv2;
    CHECK(walk(true, pk2.data(), pk2.size(), wp2, err) && walk(false, vk2.data(), vk2.size(), wv2, err));
    CHECK(pk2.size() == pk.size() && vk2.size() == vk.size());      // the small pair is compressed throughout
    CHECK(S::same_outside_sigma(pk.data(), pk.size(), wp, pk2.data(), pk2.size(), wp2) && S::same_outside_sigma(vk.data(), vk.size(), wv, vk2.data(), vk2.size(), wv2));
    CHECK(S::same_infinities(pk.data(), wp, pk2.data(), wp2));
    CHECK(!same_outside(pk.data(), pk.size(), wp, pk2.data(), pk2.size(), wp2));      // a sigma step is no delta step ...
    for (size_t j = 0; j < n; j++) {
        const uint8_t* e = pk2.data() + wp2.g1[wp2.ps0 + j].off;
        if (inf[j]) CHECK(e[0] == 0x40 && all_zero(e + 1, 31));
        else CHECK(e[0] == (((j & 1) ? 0xC0 : 0x80) | g1[64 * j]) && !memcmp(e + 1, g1.data() + 64 * j + 1, 31));
    }
    { const uint8_t* e = vk2.data() + wv2.g2[wv2.pgsn].off; CHECK(e[0] == (0xC0 | gsn[0]) && !memcmp(e + 1, gsn.data() + 1, 63)); }
    // rule 2 sees every byte outside BasisExpSigma / GSigmaNeg and none inside
    for (size_t at : {(size_t)0, (size_t)9, wp.g1[0].off + 5, wp.g1[wp.d1].off + 31, wp.g1[wp.z0].off + 1, wp.g2[wp.d2].off + 63, wp.g1[wp.pb0].off + 31,
                      wp.g1[wp.pb0 + n - 1].off + 31, wp.g1[wp.ps0].off - 1}) {
        Bytes t = pk2; t[at] ^= 1; Walk wt;
        if (walk(true, t.data(), t.size(), wt, err)) CHECK(!S::same_outside_sigma(pk.data(), pk.size(), wp, t.data(), t.size(), wt));
    }
    for (size_t at : {wp.g1[wp.ps0].off + 31, wp.g1[wp.ps0 + n - 1].off + 31}) {
        Bytes t = pk2; t[at] ^= 1; Walk wt;
        CHECK(walk(true, t.data(), t.size(), wt, err) && S::same_outside_sigma(pk.data(), pk.size(), wp, t.data(), t.size(), wt));
    }
    for (size_t at : {(size_t)3, wv.g2[wv.d2].off + 63, wv.g2[wv.pg].off + 63, wv.g2[wv.pg].off - 1}) {
        Bytes t = vk2; t[at] ^= 1; Walk wt;
        if (walk(false, t.data(), t.size(), wt, err)) CHECK(!S::same_outside_sigma(vk.data(), vk.size(), wv, t.data(), t.size(), wt));
    }
    {
        Bytes t = vk2; t[wv.g2[wv.pgsn].off + 63] ^= 1; Walk wt;
        CHECK(walk(false, t.data(), t.size(), wt, err) && S::same_outside_sigma(vk.data(), vk.size(), wv, t.data(), t.size(), wt));
        t = vk2; t[wv.g2[wv.pg].off + 63] ^= 1;
        CHECK(walk(false, t.data(), t.size(), wt, err) && S::same_outside_fresh(vk.data(), vk.size(), wv, t.data(), t.size(), wt));      // ... and G is fresh in a Setup
        CHECK(S::same_outside_fresh(pk.data(), pk.size(), wp, pk2.data(), pk2.size(), wp2));
    }
    CHECK(!S::same_outside_sigma(pk.data(), pk.size(), wp, vk.data(), vk.size(), wv));

    // the generalised comparison on phase 2's element set against phase 2's own, over a delta-step-like file and single flipped bytes
    {
        const size_t n1 = 1 + wp.nz + wp.nk;
        Bytes d1(64 * n1), di(n1, 0), d2(128);
        for (size_t i = 0; i < d1.size(); i++) d1[i] = (uint8_t)(i * 29 + 3);
        for (size_t i = 0; i < n1; i++) { d1[64 * i] &= 0x1F; d1[64 * i + 32] = 0x01; }
        for (size_t i = 0; i < 128; i++) d2[i] = (uint8_t)(2 * i + 1);
        d2[0] &= 0x1F;
        const Bytes pk3 = splice(pk.data(), pk.size(), wp, d1.data(), di.data(), d2.data()), vk3 = splice(vk.data(), vk.size(), wv, d1.data(), di.data(), d2.data());
        Walk wp3, wv3;
        CHECK(walk(true, pk3.data(), pk3.size(), wp3, err) && walk(false, vk3.data(), vk3.size(), wv3, err));
        CHECK(same_outside(pk.data(), pk.size(), wp, pk3.data(), pk3.size(), wp3) && same_outside(vk.data(), vk.size(), wv, vk3.data(), vk3.size(), wv3));
        CHECK(!S::same_outside_sigma(pk.data(), pk.size(), wp, pk3.data(), pk3.size(), wp3));      // a delta step is no sigma step
        size_t agree = 0, refused = 0;
        for (size_t at = 0; at < pk3.size(); at += 7) {
            Bytes t = pk3; t[at] ^= 0x10; Walk wt;
            if (!walk(true, t.data(), t.size(), wt, err)) continue;
            const bool got = same_outside(pk.data(), pk.size(), wp, t.data(), t.size(), wt), want = reference_same_outside(pk.data(), pk.size(), wp, t.data(), t.size(), wt);
            CHECK(got == want); agree++; refused += !got;
        }
        for (size_t at = 0; at < vk3.size(); at++) {
            Bytes t = vk3; t[at] ^= 0x10; Walk wt;
            if (!walk(false, t.data(), t.size(), wt, err)) continue;
            const bool got = same_outside(vk.data(), vk.size(), wv, t.data(), t.size(), wt), want = reference_same_outside(vk.data(), vk.size(), wv, t.data(), t.size(), wt);
            CHECK(got == want); agree++; refused += !got;
        }
        CHECK(refused > 0 && refused < agree);
        printf("same_outside.compared=%zu\n", agree);
    }

    if (argc > 8) {      // the same pair with some elements raw: it walks, rule 2 refuses it against the compressed pair, the splice writes compressed
        const Bytes mpk = slurp(argv[7]), mvk = slurp(argv[8]); Walk wm, wn;
        CHECK(walk(true, mpk.data(), mpk.size(), wm, err) && walk(false, mvk.data(), mvk.size(), wn, err));
        CHECK(wm.npb == wp.npb && mpk.size() > pk.size() && mvk.size() > vk.size());
        CHECK(!S::same_outside_sigma(pk.data(), pk.size(), wp, mpk.data(), mpk.size(), wm));      // an untouched element is raw too
        CHECK(!S::same_outside_sigma(vk.data(), vk.size(), wv, mvk.data(), mvk.size(), wn));
        CHECK(S::same_infinities(pk.data(), wp, mpk.data(), wm) && S::first_finite(mpk.data(), wm) == S::first_finite(pk.data(), wp));
        const Bytes m2 = S::splice_pk(mpk.data(), mpk.size(), wm, g1.data(), inf.data()), v2 = S::splice_vk(mvk.data(), mvk.size(), wn, gsn.data());
        Walk wm2, wn2;
        CHECK(walk(true, m2.data(), m2.size(), wm2, err) && S::same_outside_sigma(mpk.data(), mpk.size(), wm, m2.data(), m2.size(), wm2));
        CHECK(walk(false, v2.data(), v2.size(), wn2, err) && S::same_outside_sigma(mvk.data(), mvk.size(), wn, v2.data(), v2.size(), wn2));
        size_t raw_left = 0; for (size_t j = 0; j < wm2.npb; j++) if (wm2.g1[wm2.ps0 + j].size != 32) raw_left++;
        CHECK(raw_left == 0 && wn2.g2[wn2.pgsn].size == 64);
        printf("mixed.pk.bytes=%zu\nmixed.pk.spliced=%zu\nmixed.vk.bytes=%zu\nmixed.vk.spliced=%zu\n", mpk.size(), m2.size(), mvk.size(), v2.size());
    }

    // the record, its challenge, the seeded scalars, the negation
    S::Record r;
    for (int i = 0; i < 32; i++) { r.h_prev[i] = (uint8_t)i; r.h_next[i] = (uint8_t)(32 + i); r.z[i] = (uint8_t)(200 + i); }
    for (int i = 0; i < 64; i++) { r.delta[i] = (uint8_t)(64 + i); r.T[i] = (uint8_t)(128 + i); }
    uint8_t rec[S::kRecordBytes], c[32], c2[32];
    S::encode_record(r, rec);
    for (size_t i = 0; i < S::kRecordBytes; i++) CHECK(rec[i] == (uint8_t)(i < 192 ? i : 200 + (i - 192)));
    const S::Record back = S::decode_record(rec);
    CHECK(!memcmp(&back, &r, sizeof r));
    uint8_t base[64]; for (int i = 0; i < 64; i++) base[i] = (uint8_t)(255 - i);
    S::challenge(r.h_prev, base, r.delta, r.T, c);
    hex("challenge", c, 32);
    challenge(r.h_prev, base, r.delta, r.T, c2);
    hex("challenge.phase2", c2, 32);
    CHECK(memcmp(c, c2, 32));
    uint8_t seed[32]; for (int i = 0; i < 32; i++) seed[i] = (uint8_t)(5 * i + 2);
    gsc::hostf::Fr x, k; uint8_t b[32];
    CHECK(S::seeded_scalars(seed, x, k));
    x.to_be(b); hex("seeded.x", b, 32); k.to_be(b); hex("seeded.k", b, 32);
    uint8_t G[64] = {0}, N[64], O[64] = {0}, out[64];
    G[31] = 1; G[63] = 2;
    CHECK(S::g1_neg_raw(G, N) && g1_add_raw(G, N, out) && all_zero(out, 64));
    hex("-G", N, 64);
    CHECK(S::g1_neg_raw(O, out) && all_zero(out, 64));
    memset(out, 0xFF, 64); CHECK(!S::g1_neg_raw(out, N));      // a coordinate not below p

    if (failures) { printf("%d check(s) failed\n", failures); return 1; }
    printf("SIGMA-OK\n");
    return 0;
}
