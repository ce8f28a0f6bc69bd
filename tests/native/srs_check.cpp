// Stand-alone check of the powers file's host walker (csrc/srs.hpp), driven by tests/test_srs_host.py; built plainly and under
// AddressSanitizer + UBSan.  Every buffer handed to walk() is a heap block of exactly the length it is told, so a read past the end is caught.
//   srs_check <valid file> [<r1cs file>]
// With an r1cs: the term lists by wire (csrc/srs_columns.hpp build_matrices) against a second, independent walk over the instruction list,
// the coefficient table and the cut of the columns into segments.
// prints key=value tokens and SRS-OK; exit 3 with "REFUSED <reason>" when the valid file is refused, 1 on a failed expectation.
#include "srs.hpp"
#include "srs_columns.hpp"
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>

using namespace gsc;

static std::vector<uint8_t> read_file(const char* p) {
    std::ifstream f(p, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
// walk() on an exact-size copy of b[0, n)
static bool walk_copy(const uint8_t* b, size_t n, srs::Layout& l, std::string& err) {
    uint8_t* c = (uint8_t*)malloc(n ? n : 1);
    if (n) memcpy(c, b, n);
    const bool ok = srs::walk(c, n, l, err);
    free(c);
    return ok;
}
static void hex(const char* name, const std::vector<uint8_t>& v) {
    printf("%s=", name);
    for (uint8_t x : v) printf("%02x", x);
    printf("\n");
}
static std::string token(std::string s) { for (char& c : s) if (c == ' ') c = '_'; return s; }
#define EXPECT(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main(int argc, char** argv) {
    if (argc != 2 && argc != 3) return 2;
    const std::vector<uint8_t> f = read_file(argv[1]);
    srs::Layout l; std::string err;
    if (!walk_copy(f.data(), f.size(), l, err)) { printf("REFUSED %s\n", err.c_str()); return 3; }
    printf("L=%d N=%zu bytes=%zu tau1=%zu tau2=%zu alpha1=%zu beta1=%zu beta2=%zu g1=%zu g2=%zu\n", l.L, l.N, l.bytes, l.off_tau1, l.off_tau2, l.off_alpha1,
           l.off_beta1, l.off_beta2, l.n_g1(), l.n_g2());
    EXPECT(l.bytes == f.size());
    // the slots, and the way back
    std::vector<uint8_t> g1, g2;
    srs::slots(f.data(), l, g1, g2);
    EXPECT(g1.size() == 64 * l.n_g1() && g2.size() == 128 * l.n_g2());
    hex("g1slots", g1); hex("g2slots", g2);
    EXPECT(srs::assemble(l, g1.data(), g2.data()) == f);
    for (size_t i = 0; i < l.n_g1(); i++) EXPECT(!memcmp(f.data() + srs::g1_offset(l, i), g1.data() + 64 * i, 64));
    for (size_t i = 0; i < l.n_g2(); i++) EXPECT(!memcmp(f.data() + srs::g2_offset(l, i), g2.data() + 128 * i, 128));
    printf("name.first=%s name.alpha0=%s name.betalast=%s name.g2last=%s\n", srs::g1_name(l, 0).c_str(), srs::g1_name(l, l.i_alpha1()).c_str(),
           srs::g1_name(l, l.n_g1() - 1).c_str(), srs::g2_name(l, l.n_g2() - 1).c_str());

    // every truncation, the empty file included
    size_t refused = 0;
    srs::Layout t;
    for (size_t n = 0; n < f.size(); n++) { EXPECT(!walk_copy(f.data(), n, t, err)); EXPECT(err.find(n < 12 ? "truncated header" : "truncated") != std::string::npos); refused++; }
    printf("truncations=%zu\n", refused);
    EXPECT(!srs::walk(nullptr, 0, t, err));
    // trailing bytes
    { std::vector<uint8_t> b = f; b.push_back(0); EXPECT(!walk_copy(b.data(), b.size(), t, err)); printf("trailing=%s\n", token(err).c_str()); }
    // a wrong magic (every byte of it in turn)
    for (int i = 0; i < 8; i++) { std::vector<uint8_t> b = f; b[i] ^= 1; EXPECT(!walk_copy(b.data(), b.size(), t, err)); EXPECT(err.find("magic") != std::string::npos); }
    printf("magic=%s\n", token(err).c_str());
    // L edited against the length; L = 0, L = 25, high bytes of the field
    auto with_L = [&](uint32_t L) { std::vector<uint8_t> b = f; b[8] = (uint8_t)(L >> 24); b[9] = (uint8_t)(L >> 16); b[10] = (uint8_t)(L >> 8); b[11] = (uint8_t)L; return b; };
    for (uint32_t L : {(uint32_t)l.L - 1, (uint32_t)l.L + 1, 24u}) {
        if (L < 1 || L == (uint32_t)l.L) continue;
        std::vector<uint8_t> b = with_L(L); EXPECT(!walk_copy(b.data(), b.size(), t, err)); EXPECT(err.find("length does not match L") != std::string::npos);
    }
    printf("L.edited=%s\n", token(err).c_str());
    for (uint32_t L : {0u, 25u, 0x01000000u | (uint32_t)l.L, 0xFFFFFFFFu, 0x80000002u}) {
        std::vector<uint8_t> b = with_L(L); EXPECT(!walk_copy(b.data(), b.size(), t, err)); EXPECT(err.find("L outside") != std::string::npos);
    }
    printf("L.range=%s\n", token(err).c_str());
    // an element with flag bits (compressed, compressed infinity) and an all-zero element, in every section
    const size_t g1_at[] = {0, l.n_tau1() - 1, l.i_alpha1(), l.i_beta1() - 1, l.i_beta1(), l.n_g1() - 1};
    for (size_t i : g1_at) for (uint8_t flag : {0x80, 0xC0, 0x40}) {
        std::vector<uint8_t> b = f; b[srs::g1_offset(l, i)] |= flag;
        EXPECT(!walk_copy(b.data(), b.size(), t, err)); EXPECT(err == "srs: " + srs::g1_name(l, i) + " is not a raw element");
    }
    for (size_t i : g1_at) {
        std::vector<uint8_t> b = f; memset(b.data() + srs::g1_offset(l, i), 0, 64);
        EXPECT(!walk_copy(b.data(), b.size(), t, err)); EXPECT(err == "srs: " + srs::g1_name(l, i) + " is the point at infinity");
    }
    printf("g1.zero=%s\n", token(err).c_str());
    for (size_t i : {(size_t)0, l.N - 1, l.N}) {
        std::vector<uint8_t> b = f; b[srs::g2_offset(l, i)] |= 0x80;
        EXPECT(!walk_copy(b.data(), b.size(), t, err)); EXPECT(err == "srs: " + srs::g2_name(l, i) + " is not a raw element");
        b = f; memset(b.data() + srs::g2_offset(l, i), 0, 128);
        EXPECT(!walk_copy(b.data(), b.size(), t, err)); EXPECT(err == "srs: " + srs::g2_name(l, i) + " is the point at infinity");
    }
    printf("g2.zero=%s\n", token(err).c_str());
    // the sizes L gives
    for (int L = -1; L <= 26; L++) {
        srs::Layout q; const bool ok = srs::layout_of(L, q);
        EXPECT(ok == (L >= 1 && L <= 24));
        if (ok) EXPECT(q.bytes == 12 + 64 * q.n_g1() + 128 * q.n_g2() && q.n_g1() == 4 * q.N - 1 && q.off_beta2 + 128 == q.bytes);
        if (L == 24) printf("bytes24=%zu\n", q.bytes);
    }
    if (argc == 3) {
        const std::vector<uint8_t> rb = read_file(argv[2]);
        const R1csFile cs = parse_r1cs(rb.data(), rb.size());
        srs::Matrix M[3];
        srs::build_matrices(cs, M);
        const size_t nw = cs.n_wires();
        // the second walk: per wire and matrix, the number of terms and the sums of (coefficient id + 1) * (row + 1) and of row
        std::vector<uint64_t> cnt[3], mix[3], rows[3];
        for (int s = 0; s < 3; s++) { cnt[s].assign(nw, 0); mix[s].assign(nw, 0); rows[s].assign(nw, 0); }
        for (size_t ii = 0; ii < cs.n_instr(); ii++) {
            if (cs.bp_kind[cs.blueprint[ii]] != BP_R1C) continue;
            const uint32_t* cd = cs.calldata.data() + cs.instr_start[ii];
            size_t at = 4;
            for (int s = 0; s < 3; s++) for (uint32_t k = 0; k < cd[1 + s]; k++, at += 2) {
                const uint32_t w = cd[at + 1] == WIRE_CONST ? 0 : cd[at + 1];
                cnt[s][w]++; mix[s][w] += (uint64_t)(cd[at] + 1) * (cs.constraint_off[ii] + 1); rows[s][w] += cs.constraint_off[ii];
            }
        }
        size_t total = 0;
        const char* names[3] = {"L", "R", "O"};
        for (int s = 0; s < 3; s++) {
            EXPECT(M[s].col_start.size() == nw + 1 && M[s].col_start[0] == 0 && M[s].col_start[nw] == M[s].n_terms() && M[s].coeff.size() == M[s].row.size());
            for (size_t w = 0; w < nw; w++) {
                uint64_t c = 0, mx = 0, rw = 0;
                for (uint32_t t = M[s].col_start[w]; t < M[s].col_start[w + 1]; t++) { c++; mx += (uint64_t)(M[s].coeff[t] + 1) * (M[s].row[t] + 1); rw += M[s].row[t]; EXPECT(M[s].row[t] < cs.n_constraints && M[s].coeff[t] < cs.n_coeff()); }
                EXPECT(c == cnt[s][w] && mx == mix[s][w] && rw == rows[s][w]);
            }
            srs::Segments sg;
            EXPECT(srs::cut_columns(M[s].col_start.data(), nw, M[s].n_terms(), sg));
            size_t covered = 0;
            for (size_t k = 0; k < sg.begin.size(); k++) { EXPECT(sg.end[k] > sg.begin[k] && sg.end[k] - sg.begin[k] <= srs::kColSegTerms); covered += sg.end[k] - sg.begin[k]; }
            EXPECT(covered == M[s].n_terms() && sg.col_seg[nw] == sg.begin.size());
            printf("%s.terms=%zu %s.columns=%zu %s.longest=%zu %s.segments=%zu %s.wire0=%u\n", names[s], M[s].n_terms(), names[s], nw, names[s], M[s].longest(), names[s], sg.begin.size(), names[s], M[s].col_start[1]);
            total += M[s].n_terms();
        }
        // what the solver computes beyond the constraints: the linear expressions that feed the hints (cd: size, hint id, inputs, then per input
        // a count and that many (coefficient, wire) pairs).  They are no rows of the matrices, so no Setup walks them.
        size_t hint_terms = 0;
        for (size_t ii = 0; ii < cs.n_instr(); ii++) {
            if (cs.bp_kind[cs.blueprint[ii]] != BP_HINT) continue;
            const uint32_t* cd = cs.calldata.data() + cs.instr_start[ii]; const uint32_t* end = cs.calldata.data() + cs.instr_start[ii + 1];
            const uint32_t* p = cd + 3;
            for (uint32_t k = 0; k < cd[2] && p < end; k++) { hint_terms += p[0]; p += 1 + 2 * (size_t)p[0]; }
        }
        printf("terms.total=%zu hint.terms=%zu coefficients=%zu\n", total, hint_terms, cs.n_coeff());
        // bad offsets are refused, not walked
        srs::Segments sg; const uint32_t bad1[3] = {0, 5, 3}, bad2[3] = {1, 2, 3}, bad3[3] = {0, 2, 4};
        EXPECT(!srs::cut_columns(bad1, 2, 3, sg) && !srs::cut_columns(bad2, 2, 3, sg) && !srs::cut_columns(bad3, 2, 3, sg));
        // the coefficient table: 0, 1, r - 1, 2, r - 2, (two zeros), a 34-bit value, then r itself (refused)
        uint8_t be[9][32]; memset(be, 0, sizeof be);
        auto r_minus = [&](uint8_t* o, uint32_t k) { uint32_t m[8], kk[8] = {k, 0, 0, 0, 0, 0, 0, 0}; srs::detail::sub8(srs::kR, kk, m); for (int i = 0; i < 8; i++) for (int b = 0; b < 4; b++) o[4 * (7 - i) + b] = (uint8_t)(m[i] >> (24 - 8 * b)); };
        be[1][31] = 1; r_minus(be[2], 1); be[3][31] = 2; r_minus(be[4], 2); be[7][27] = 3; be[7][31] = 9; r_minus(be[8], 0);
        srs::CoeffTable ct;
        EXPECT(srs::prepare_coeffs(&be[0][0], 8, ct));
        printf("meta=%x,%x,%x,%x,%x,%x\n", ct.meta[0], ct.meta[1], ct.meta[2], ct.meta[3], ct.meta[4], ct.meta[7]);
        EXPECT(ct.mag[8 * 2] == 1 && ct.mag[8 * 4] == 2 && ct.mag[8 * 7] == 9 && ct.mag[8 * 7 + 1] == 3);
        EXPECT(!srs::prepare_coeffs(&be[0][0], 9, ct));
    }
    printf("SRS-OK\n");
    return 0;
}
