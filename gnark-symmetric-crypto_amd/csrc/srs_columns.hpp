// Column sums over a sparse matrix "in the exponent" (k_srs_columns.hip): the host side.  Pure host code, no HIP:
// tests/native/srs_check.cpp builds it with g++ (also under -fsanitize=address,undefined).
//
// A matrix is given by columns: column w holds the terms [col_start[w], col_start[w + 1]), each a (row, coefficient id) pair; the device
// computes out[w] = sum c P[row] over the column's terms for a vector P of group elements.  Here: the coefficients as the kernel wants them
// (sign and magnitude, so that -1 and r - small cost what 1 and small cost), and the cut of long columns into segments of at most
// kColSegTerms terms, each summed by one wave before a second kernel adds a column's segments up.  Coefficients are public (they are the
// circuit's), so nothing here or in the kernel is constant-time.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <vector>
#include "formats.hpp"

namespace gsc {
namespace srs {

constexpr uint32_t kColLanes = 64;          // one wave per segment, lanes striding over its terms
constexpr uint32_t kColSegTerms = 256;      // terms per segment: at most four per lane
constexpr uint32_t kColsPerBlock = 64;      // the second kernel: one thread per column

// r, little-endian 32-bit words
constexpr uint32_t kR[8] = {0xf0000001u, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};

// coefficient id -> magnitude (8 little-endian words) and meta = bits of the magnitude | negative << 16; c = 0 has 0 bits (the term is skipped)
struct CoeffTable { std::vector<uint32_t> mag, meta; };

namespace detail {
inline int cmp8(const uint32_t* a, const uint32_t* b) { for (int i = 7; i >= 0; i--) if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1; return 0; }
inline void sub8(const uint32_t* a, const uint32_t* b, uint32_t* o) { uint64_t br = 0; for (int i = 0; i < 8; i++) { const uint64_t t = (uint64_t)a[i] - b[i] - br; o[i] = (uint32_t)t; br = (t >> 32) & 1; } }
inline int bits8(const uint32_t* a) { for (int i = 255; i >= 0; i--) if ((a[i >> 5] >> (i & 31)) & 1u) return i + 1; return 0; }
}  // namespace detail

// be: n coefficients of 32 big-endian bytes; false when one is not below r
inline bool prepare_coeffs(const uint8_t* be, size_t n, CoeffTable& t) {
    t.mag.assign(8 * n, 0); t.meta.assign(n, 0);
    for (size_t k = 0; k < n; k++) {
        uint32_t c[8], m[8];
        for (int i = 0; i < 8; i++) { const uint8_t* p = be + 32 * k + 4 * (7 - i); c[i] = (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }
        if (detail::cmp8(c, kR) >= 0) return false;
        detail::sub8(kR, c, m);                                           // r - c
        const bool neg = detail::bits8(c) != 0 && detail::cmp8(m, c) < 0;      // the shorter of c and r - c
        memcpy(&t.mag[8 * k], neg ? m : c, 32);
        t.meta[k] = (uint32_t)detail::bits8(&t.mag[8 * k]) | (neg ? 1u << 16 : 0u);
    }
    return true;
}

// segment s covers the terms [begin[s], end[s]) of one column; column w owns the segments [col_seg[w], col_seg[w + 1]) (none: an empty column)
struct Segments { std::vector<uint32_t> begin, end, col_seg; };

// false when col_start (n_cols + 1 entries) does not start at 0, decreases, or does not end at n_terms
inline bool cut_columns(const uint32_t* col_start, size_t n_cols, size_t n_terms, Segments& s) {
    s.begin.clear(); s.end.clear(); s.col_seg.assign(n_cols + 1, 0);
    if (col_start[0] != 0 || col_start[n_cols] != n_terms) return false;
    for (size_t w = 0; w < n_cols; w++) {
        const uint32_t a = col_start[w], b = col_start[w + 1];
        if (b < a || b > n_terms) return false;
        for (uint32_t at = a; at < b; at += kColSegTerms) { s.begin.push_back(at); s.end.push_back(b - at > kColSegTerms ? at + kColSegTerms : b); }
        s.col_seg[w + 1] = (uint32_t)s.begin.size();
    }
    return true;
}

// One R1CS matrix by wire: column w = the terms (constraint row, coefficient id) of wire w, in instruction order.
struct Matrix {
    std::vector<uint32_t> col_start, row, coeff;
    size_t n_terms() const { return row.size(); }
    size_t longest() const { size_t m = 0; for (size_t w = 0; w + 1 < col_start.size(); w++) if (col_start[w + 1] - col_start[w] > m) m = col_start[w + 1] - col_start[w]; return m; }
};
// The three matrices L, R, O from the walk over the instruction list that groth16_setup does: the same terms, a constant term goes to wire
// 0 (the ONE wire), the same range checks (std::runtime_error).  m: the constraint count the rows must stay below.
inline void build_matrices(const R1csFile& cs, Matrix out[3]) {
    const size_t m = cs.n_constraints, nw = cs.n_wires(), nc = cs.n_coeff();
    for (int pass = 0; pass < 2; pass++) {
        if (pass == 1) for (int side = 0; side < 3; side++) {
            Matrix& M = out[side];
            uint32_t run = 0;
            for (size_t w = 0; w <= nw; w++) { const uint32_t c = w < nw ? M.col_start[w] : 0; M.col_start[w] = run; run += c; }
            M.row.assign(run, 0); M.coeff.assign(run, 0);
        } else for (int side = 0; side < 3; side++) { out[side].col_start.assign(nw + 1, 0); out[side].row.clear(); out[side].coeff.clear(); }
        std::vector<uint32_t> fill[3];
        if (pass == 1) for (int side = 0; side < 3; side++) fill[side].assign(out[side].col_start.begin(), out[side].col_start.end() - 1);
        for (size_t ii = 0; ii < cs.n_instr(); ii++) {
            if (cs.bp_kind[cs.blueprint[ii]] != BP_R1C) continue;
            const uint32_t* cd = cs.calldata.data() + cs.instr_start[ii];
            const uint32_t cnt[3] = {cd[1], cd[2], cd[3]}; const uint32_t* t = cd + 4;
            if (cs.constraint_off[ii] >= m) throw std::runtime_error("setup: constraint offset out of range");
            for (int side = 0; side < 3; side++) for (uint32_t k = 0; k < cnt[side]; k++, t += 2) {
                if (t[0] >= nc) throw std::runtime_error("setup: coefficient id out of range");
                const uint32_t wid = t[1] == WIRE_CONST ? 0 : t[1];
                if (wid >= nw) throw std::runtime_error("setup: wire id out of range");
                if (pass == 0) out[side].col_start[wid]++;
                else { const uint32_t at = fill[side][wid]++; out[side].row[at] = cs.constraint_off[ii]; out[side].coeff[at] = t[0]; }
            }
        }
    }
}

}  // namespace srs
}  // namespace gsc
