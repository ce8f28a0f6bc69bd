// Per-thread Groth16 verification over BN254 for the GPU verifier (k_verify.hip): strict point decoding, the G2 subgroup test,
// the public-input sum from byte-window tables, an Fp6/Fp12 tower on the radix-2^29 field of bn254_fp29.hpp, the optimal-ate
// Miller loop (inversion-free for the proof's own pair, precomputed lines for the key's fixed G2 points) and the final
// exponentiation by an x-power chain.  Every function is plain per-thread code: the same source compiles for the host (g++ with
// the HIP headers), which is how tests/native/verify_dev_check.cpp checks it against libverify without a GPU.
//
// The Fp12 operations, the Miller steps and the exponentiations are out-of-line functions: each is compiled once (inlining them
// all makes one kernel of a million instructions); their operands pass through the stack.
//
// Value discipline: every Fp / Fp2 value handed to a product is tight (limbs 0..7 in [0, 2^29)) with |value| < 5p; products and
// red() return |value| < 2.01p, so sums of two such values may be multiplied directly and longer sums go through red() first.
// Two operations hand parts of their operand on untouched, which keep the operand's bound: the even coefficients of conj12 and
// coefficient 0 of frob12_2 (whose other coefficients are scale2's unreduced products, in (-p, 2p)).
#pragma once
#include "bn254_fp29.hpp"
#include "sha256_dev.hpp"

namespace gsc {
namespace vfy {
using bn254::fe;
using bn254::fe9;
using bn254::fe9x2;
using F = bn254::Fp29;
using F2 = bn254::Fp2x;
using e1 = fe9;
using e2 = fe9x2;

// ---- memory images (plain limbs, no packing: these buffers never leave the verifier) ----
struct VP1 { fe9 x, y; int32_t inf; };          // affine G1, inf != 0: point at infinity
struct VP2 { fe9x2 x, y; int32_t inf; };        // affine G2
struct Line { fe9x2 a, b, c; };                 // l(P) = a yP + b xP w + c w^3

constexpr int kLoopSteps = 64;                                        // bits 63..0 of 6x+2 below its top bit
DEVFN constexpr uint64_t loop_bits() { return 0x9d797039be763ba8ull; }  // 6x + 2 = 2^64 + this, x = 4965661367192848881
constexpr int kLineSteps = 64 + 36 + 2;                                 // doublings + additions of the loop (popcount 36) + 2 Frobenius adds
constexpr uint64_t kX = 4965661367192848881ull;                        // BN254 x (positive)
constexpr int kWindows = 144;                                         // public-input byte windows (ChaCha: 1152 bits; AES: 12 + 4 + 128 bytes)
constexpr int kCommitWindows = 32;                                    // bytes of the commitment challenge

// ---- Fp ----
DEVFN e1 cst(const int32_t (&v)[9]) { e1 r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = v[i];
    return r; }
// tight value with |value| < 2.01p: subtract q p, q from the top limb (|limb 8| of p is 3171406)
DEVFN e1 red(const e1& a) {
    const e1 x = F::norm(a);
    const int32_t q = x.l[8] / 3171406;
    e1 r; int64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) { const int64_t t = (int64_t)x.l[i] - (int64_t)q * F::P(i) + c; r.l[i] = (int32_t)(t & F::MASK); c = t >> 29; }
    r.l[8] = (int32_t)((int64_t)x.l[8] - (int64_t)q * F::P(8) + c);
    return r;
}
// ka a + kb b for small integers (9 + u multiplications), then red()
DEVFN e1 lin(const e1& a, int ka, const e1& b, int kb) {
    e1 r; int64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) { const int64_t t = (int64_t)ka * a.l[i] + (int64_t)kb * b.l[i] + c; r.l[i] = (int32_t)(t & F::MASK); c = t >> 29; }
    r.l[8] = (int32_t)((int64_t)ka * a.l[8] + (int64_t)kb * b.l[8] + c);
    return red(r);
}
DEVFN e1 add1(const e1& a, const e1& b) { return red(F::add(a, b)); }
DEVFN e1 sub1(const e1& a, const e1& b) { return red(F::sub(a, b)); }
DEVFN e1 neg1(const e1& a) { return red(F::neg(a)); }
DEVFN e1 mul1(const e1& a, const e1& b) { return F::mul(a, b); }
DEVFN e1 sqr1(const e1& a) { return F::sqr(a); }
DEVFN bool eq1(const e1& a, const e1& b) { return F::is_zero(F::sub(a, b)); }
DEVFN bool zero1(const e1& a) { return F::is_zero(a); }
// a^e for a fixed 256-bit exponent (8 little-endian words)
DEVNOINL e1 pow1(const e1& a, const uint32_t (&e)[8]) {
    e1 acc = F::one();
    for (int i = 255; i >= 0; i--) {
        acc = F::sqr(acc);
        if ((e[i >> 5] >> (i & 31)) & 1) acc = F::mul(acc, a);
    }
    return acc;
}
DEVFN e1 inv1(const e1& a) {      // Fermat; 0 -> 0
    const uint32_t e[8] = {0xd87cfd45u, 0x3c208c16u, 0x6871ca8du, 0x97816a91u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};
    return pow1(a, e);
}
// square root candidate a^((p+1)/4) (p = 3 mod 4); the caller checks it
DEVFN e1 sqrt_cand(const e1& a) {
    const uint32_t e[8] = {0xb61f3f52u, 0x4f082305u, 0x5a1c72a3u, 0x65e05aa4u, 0xa0605617u, 0x6e14116du, 0xb84c680au, 0x0c19139cu};
    return pow1(a, e);
}
DEVFN bool sqrt1(const e1& a, e1& out) { const e1 s = sqrt_cand(a); if (!eq1(F::sqr(s), a)) return false; out = s; return true; }

// ---- Fp2 ----
DEVFN e2 mk2(const e1& a, const e1& b) { return e2{a, b}; }
DEVFN e2 red2(const e2& a) { return e2{red(a.a0), red(a.a1)}; }
DEVFN e2 add2(const e2& a, const e2& b) { return red2(F2::add(a, b)); }
DEVFN e2 sub2(const e2& a, const e2& b) { return red2(F2::sub(a, b)); }
DEVFN e2 neg2(const e2& a) { return red2(F2::neg(a)); }
DEVFN e2 mul2(const e2& a, const e2& b) { return red2(F2::mul(a, b)); }
DEVFN e2 sqr2(const e2& a) { return red2(F2::sqr(a)); }
DEVFN e2 scale2(const e2& a, const e1& k) { return e2{F::mul(a.a0, k), F::mul(a.a1, k)}; }
DEVFN e2 conj2(const e2& a) { return e2{red(a.a0), neg1(a.a1)}; }      // both halves reduced: an operand that was a lazy sum does not stay one
DEVFN e2 conj2p(const e2& a) { return e2{a.a0, neg1(a.a1)}; }           // for the operand of a product: the real half goes in as it came
DEVFN e2 mulxi(const e2& a) { return e2{lin(a.a0, 9, a.a1, -1), lin(a.a0, 1, a.a1, 9)}; }     // (9 + u) a
DEVFN e2 small2(const e2& a, int k) { return e2{lin(a.a0, k, a.a1, 0), lin(a.a1, k, a.a0, 0)}; }
DEVFN bool zero2(const e2& a) { return zero1(a.a0) && zero1(a.a1); }
DEVFN bool eq2(const e2& a, const e2& b) { return eq1(a.a0, b.a0) && eq1(a.a1, b.a1); }
DEVFN e2 inv2(const e2& a) {
    const e1 n = inv1(red(F::add(F::sqr(a.a0), F::sqr(a.a1))));
    return e2{F::mul(a.a0, n), neg1(F::mul(a.a1, n))};
}
DEVFN bool lex_large1(const e1& a) { return F::lex_large(red(a)); }
DEVFN bool lex_large2(const e2& a) { return zero1(a.a1) ? lex_large1(a.a0) : lex_large1(a.a1); }

// constants in the 2^261 Montgomery domain
DEVFN e2 twist_b() { constexpr int32_t a[9] = {189306456, 13619797, 266050167, 47090167, 3383508, 443974981, 116276700, 275414465, 1651051}, b[9] = {463465696, 132959441, 275378631, 215966963, 22334433, 231877312, 116106472, 422158901, 2635577}; return e2{cst(a), cst(b)}; }
DEVFN e2 frob_g2() { constexpr int32_t a[9] = {77959568, 116720857, 200831163, 387972444, 449106301, 79574741, 198110247, 444835091, 2396851}, b[9] = {286535409, 187804871, 492312764, 403373079, 442701694, 360078139, 294614062, 104485018, 1269326}; return e2{cst(a), cst(b)}; }   // xi^((p-1)/3)
DEVFN e2 frob_g3() { constexpr int32_t a[9] = {455018104, 57932550, 320278461, 408777911, 37819167, 383878197, 519288526, 32534274, 1918653}, b[9] = {430327765, 436072363, 496131354, 220163167, 145517765, 530932250, 323946238, 161949718, 1410845}; return e2{cst(a), cst(b)}; }   // xi^((p-1)/2)
// w^(i p) = frob1(i) w^i with gamma = xi^((p-1)/6), frob1(i) = gamma^i (i = 1..5)
DEVFN e2 frob1(int i) {
    constexpr int32_t v[5][2][9] = {
        {{168567705, 446838140, 21606957, 76005147, 193575774, 320063457, 492961205, 101471925, 3016032}, {466013235, 394132337, 371054763, 25204381, 93145077, 448361909, 29518381, 483951129, 39811}},
        {{77959568, 116720857, 200831163, 387972444, 449106301, 79574741, 198110247, 444835091, 2396851}, {286535409, 187804871, 492312764, 403373079, 442701694, 360078139, 294614062, 104485018, 1269326}},
        {{455018104, 57932550, 320278461, 408777911, 37819167, 383878197, 519288526, 32534274, 1918653}, {430327765, 436072363, 496131354, 220163167, 145517765, 530932250, 323946238, 161949718, 1410845}},
        {{276953182, 328873349, 306900296, 55370336, 434202341, 186067288, 221116544, 233072759, 1472337}, {258042488, 93586473, 404468614, 107881851, 15098452, 202552781, 251052073, 472003299, 457208}},
        {{122035596, 70559408, 351843991, 185247759, 294359775, 74527549, 415682662, 131659696, 1090544}, {515197319, 148204830, 209777112, 355922816, 112506023, 137088316, 422875504, 397322748, 530422}}};
    return e2{cst(v[i - 1][0]), cst(v[i - 1][1])};
}
// w^(i p^2) = frob2(i) w^i, frob2(i) = N(gamma)^i in Fp
DEVFN e1 frob2c(int i) {
    constexpr int32_t v[5][9] = {
        {239698866, 192365459, 64358326, 265999499, 489041563, 23351122, 297356679, 439555315, 2382159},
        {416069521, 391846970, 193189602, 244240497, 310558434, 69340804, 535036287, 352865610, 1478937},
        {50344230, 216545630, 69235323, 25763511, 182610367, 93913074, 248616249, 154230411, 2268184},
        {171145621, 361569571, 412916632, 318393925, 408922844, 24572269, 250450874, 338235712, 789246},
        {531645878, 162088059, 284085356, 340152927, 50535061, 515453500, 12771265, 424925417, 1692468}};
    return cst(v[i - 1]);
}
DEVFN e1 half1() { constexpr int32_t v[9] = {385672372, 177226759, 174221841, 303076213, 269788312, 269402311, 155063972, 163804910, 2037314}; return cst(v); }
DEVFN e1 three1() { constexpr int32_t v[9] = {7758947, 475297290, 150377082, 65277005, 535449387, 398901866, 360702999, 260069113, 2709666}; return cst(v); }

// Fp2 square root by the norm method, the same case split as libverify's fp2_sqrt (the result is checked, so any root will do:
// the caller picks the sign)
DEVNOINL bool sqrt2(const e2& a, e2& out) {
    e2 x;
    if (zero1(a.a1)) {
        e1 s;
        if (sqrt1(a.a0, s)) x = e2{s, F::zero()};
        else { if (!sqrt1(neg1(a.a0), s)) return false; x = e2{F::zero(), s}; }
    } else {
        e1 s, x0;
        if (!sqrt1(red(F::add(F::sqr(a.a0), F::sqr(a.a1))), s)) return false;
        if (!sqrt1(F::mul(add1(a.a0, s), half1()), x0) && !sqrt1(F::mul(sub1(a.a0, s), half1()), x0)) return false;
        x = e2{x0, F::mul(a.a1, inv1(add1(x0, x0)))};
    }
    if (!eq2(sqr2(x), a)) return false;
    out = x; return true;
}

// ---- gnark-crypto compressed points, as strict as libverify's g1_decode / g2_decode ----
// canonical value as eight little-endian 32-bit words -> Montgomery limbs; false when >= p
DEVFN bool fp_from_words(const fe& w, e1& out) {
    constexpr uint32_t P[8] = {0xd87cfd47u, 0x3c208c16u, 0x6871ca8du, 0x97816a91u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};
    bool lt = false, decided = false;
    for (int i = 7; i >= 0; i--) if (!decided && w.l[i] != P[i]) { lt = w.l[i] < P[i]; decided = true; }
    if (!lt) return false;
    out = F::to_mont(F::unpack(w));
    return true;
}
// big-endian 32 bytes (top two bits cleared when `mask`) -> canonical limbs; false when >= p
DEVFN bool fp_from_be(const uint8_t* b, bool mask, e1& out) {
    fe w;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint8_t* q = b + 28 - 4 * i;
        uint32_t b0 = q[0];
        if (mask && i == 7) b0 &= 0x3F;
        w.l[i] = (b0 << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | q[3];
    }
    return fp_from_words(w, out);
}
// the limbs fp_from_words gives for the value of a: a decoded point is then the same words whichever encoding it came in (a square root's
// limbs are one of several images of its value)
DEVFN e1 canon1(const e1& a) { return F::to_mont(F::unpack(F::pack(F::from_mont(a)))); }
// 0: finite point, 1: infinity, -1: rejected
DEVFN int decode_g1(const uint8_t* b, VP1& p) {
    const uint8_t flag = b[0] & 0xC0;
    p.x = F::zero(); p.y = F::zero(); p.inf = 1;
    if (flag == 0x40) {      // infinity only when every other bit is zero
        uint32_t o = b[0] & 0x3F;
        for (int i = 1; i < 32; i++) o |= b[i];
        return o ? -1 : 1;
    }
    if (flag == 0) return -1;
    e1 x, y;
    if (!fp_from_be(b, true, x)) return -1;
    if (!sqrt1(red(F::add(F::mul(F::sqr(x), x), three1())), y)) return -1;
    if ((flag == 0xC0) != lex_large1(y)) y = neg1(y);
    p.x = x; p.y = canon1(y); p.inf = 0;
    return 0;
}
DEVFN int decode_g2_curve(const uint8_t* b, VP2& p) {      // without the subgroup test
    const uint8_t flag = b[0] & 0xC0;
    p.x = F2::zero(); p.y = F2::zero(); p.inf = 1;
    if (flag == 0x40) {
        uint32_t o = b[0] & 0x3F;
        for (int i = 1; i < 64; i++) o |= b[i];
        return o ? -1 : 1;
    }
    if (flag == 0) return -1;
    e2 x, y;
    if (!fp_from_be(b, true, x.a1) || !fp_from_be(b + 32, false, x.a0)) return -1;
    if (!sqrt2(add2(mul2(sqr2(x), x), twist_b()), y)) return -1;
    if ((flag == 0xC0) != lex_large2(y)) y = neg2(y);
    p.x = x; p.y = e2{canon1(y.a0), canon1(y.a1)}; p.inf = 0;
    return 0;
}
// [r] Q == O: the plain test libverify uses (double-and-add over the bits of r, exact XYZZ formulas)
DEVNOINL bool g2_in_subgroup(const VP2& q) {
    if (q.inf) return true;
    using G = bn254::G2x;
    constexpr uint32_t R[8] = {0xf0000001u, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};
    const bn254::Aff9<F2> qa{q.x, q.y};
    bn254::Xyzz9<F2> acc = G::from_aff(qa);
    for (int i = 252; i >= 0; i--) {      // r < 2^254, bit 253 set
        acc = G::dbl(acc);
        if ((R[i >> 5] >> (i & 31)) & 1) acc = G::madd<true>(acc, qa);
    }
    return acc.inf || F2::is_zero(acc.zz);
}
DEVFN int decode_g2(const uint8_t* b, VP2& p) {
    const int s = decode_g2_curve(b, p);
    if (s == 0 && !g2_in_subgroup(p)) return -1;
    return s;
}

// ---- points of a KEY: compressed as above, or raw (flag bits 00: X | Y as WriteRawTo writes them), as strict as libverify's g1_decode_key /
// g2_decode_key.  b is a slot of 64 (G1) / 128 (G2) bytes: a compressed element sits in its first half.  Raw: canonical coordinates, the
// curve equation exactly, no square root; all-zero bytes are the point at infinity.  Proofs never come this way. ----
DEVFN int decode_g1_key(const uint8_t* b, VP1& p) {
    if ((b[0] & 0xC0) != 0) return decode_g1(b, p);
    p.x = F::zero(); p.y = F::zero(); p.inf = 1;
    uint32_t o = 0;
    for (int i = 0; i < 64; i++) o |= b[i];
    if (!o) return 1;
    e1 x, y;
    if (!fp_from_be(b, false, x) || !fp_from_be(b + 32, false, y)) return -1;
    if (!eq1(F::sqr(y), red(F::add(F::mul(F::sqr(x), x), three1())))) return -1;
    p.x = x; p.y = y; p.inf = 0;
    return 0;
}
DEVFN int decode_g2_key(const uint8_t* b, VP2& p) {      // with the subgroup test
    if ((b[0] & 0xC0) != 0) return decode_g2(b, p);
    p.x = F2::zero(); p.y = F2::zero(); p.inf = 1;
    uint32_t o = 0;
    for (int i = 0; i < 128; i++) o |= b[i];
    if (!o) return 1;
    e2 x, y;
    if (!fp_from_be(b, false, x.a1) || !fp_from_be(b + 32, false, x.a0) || !fp_from_be(b + 64, false, y.a1) || !fp_from_be(b + 96, false, y.a0)) return -1;
    if (!eq2(sqr2(y), add2(mul2(sqr2(x), x), twist_b()))) return -1;
    p.x = x; p.y = y; p.inf = 0;
    return g2_in_subgroup(p) ? 0 : -1;
}

// ---- G1 sums (exact XYZZ) ----
using G1X = bn254::Xyzz9<bn254::Fp29f>;
DEVFN G1X g1_inf() { return bn254::G1x::infinity(); }
DEVFN G1X g1_madd(const G1X& acc, const VP1& q) {
    if (q.inf) return acc;
    return bn254::G1x::madd<true>(acc, bn254::Aff9<bn254::Fp29f>{q.x, q.y});
}
DEVFN VP1 g1_affine(const G1X& p) {
    VP1 r;
    if (p.inf || F::is_zero(p.zz)) { r.x = F::zero(); r.y = F::zero(); r.inf = 1; return r; }
    const auto a = bn254::G1x::to_aff(p);
    r.x = red(a.x); r.y = red(a.y); r.inf = 0;
    return r;
}
// the same for G2 (the key ceremony's results: k_phase2.hip, k_quot_bases.hip's transform of a powers file, k_srs_columns.hip)
DEVFN VP2 g2_affine(const bn254::Xyzz9<bn254::Fp2x>& p) {
    VP2 r;
    if (p.inf || F2::is_zero(p.zz)) { r.x = F2::zero(); r.y = F2::zero(); r.inf = 1; return r; }
    const auto a = bn254::G2x::to_aff(p);
    r.x = red2(a.x); r.y = red2(a.y); r.inf = 0;
    return r;
}
// v 2^shift Q for one table entry (v < 256)
DEVFN VP1 g1_small_mul(const VP1& q, uint32_t v, int shift) {
    if (q.inf || v == 0) { VP1 r; r.x = F::zero(); r.y = F::zero(); r.inf = 1; return r; }
    G1X b = bn254::G1x::from_aff(bn254::Aff9<bn254::Fp29f>{q.x, q.y});
    for (int i = 0; i < shift; i++) b = bn254::G1x::dbl(b);
    const VP1 ba = g1_affine(b);
    G1X acc = g1_inf();
    for (int i = 7; i >= 0; i--) { acc = bn254::G1x::dbl(acc); if ((v >> i) & 1) acc = g1_madd(acc, ba); }
    return g1_affine(acc);
}

// ---- Fp12 = Fp2[w] / (w^6 - xi), xi = 9 + u (the tower libverify uses); Fp6 = Fp2[v] / (v^3 - xi), v = w^2 ----
struct F12 { e2 c[6]; };
DEVFN F12 one12() { F12 r;
#pragma unroll
    for (int i = 0; i < 6; i++) r.c[i] = F2::zero();
    r.c[0] = F2::one(); return r; }
DEVFN e2 acc2(const e2& s, const e2& t) { return F2::norm(F2::add(s, t)); }      // running sums of reduced products stay < 2^31 per limb
// (the loops of the three Fp12 products below stay rolled: the optimizer declines to unroll bodies this large)
DEVNOINL F12 mul12(const F12& a, const F12& b) {
    F12 r;
    for (int k = 0; k < 6; k++) {
        e2 lo = mul2(a.c[0], b.c[k]);
        for (int i = 1; i <= k; i++) lo = acc2(lo, mul2(a.c[i], b.c[k - i]));
        if (k < 5) {
            e2 hi = mul2(a.c[k + 1], b.c[5]);
            for (int i = k + 2; i < 6; i++) hi = acc2(hi, mul2(a.c[i], b.c[k + 6 - i]));
            lo = F2::add(red2(lo), mulxi(red2(hi)));
        }
        r.c[k] = red2(lo);
    }
    return r;
}
DEVNOINL F12 sqr12(const F12& a) {
    e2 d[6];
    for (int i = 0; i < 6; i++) d[i] = small2(a.c[i], 2);
    F12 r;
    for (int k = 0; k < 6; k++) {
        // t_k = sum_{i+j=k} a_i a_j, t_{k+6} likewise; cross products once against the doubled operand
        e2 lo = F2::zero(), hi = F2::zero();
        bool lo_set = false, hi_set = false;
        for (int i = 0; 2 * i <= k; i++) {
            const int j = k - i;
            const e2 m = (i == j) ? sqr2(a.c[i]) : mul2(d[i], a.c[j]);
            lo = lo_set ? acc2(lo, m) : m; lo_set = true;
        }
        for (int i = k + 1; 2 * i <= k + 6; i++) {
            const int j = k + 6 - i;
            if (j > 5) continue;
            const e2 m = (i == j) ? sqr2(a.c[i]) : mul2(d[j], a.c[i]);
            hi = hi_set ? acc2(hi, m) : m; hi_set = true;
        }
        if (hi_set) lo = F2::add(red2(lo), mulxi(red2(hi)));
        r.c[k] = red2(lo);
    }
    return r;
}
// f * (c0 + c1 w + c3 w^3)
DEVNOINL F12 mul_line(const F12& f, const e2& c0, const e2& c1, const e2& c3) {
    // ext[j + 3] = f_j, ext[j] = xi f_(j+3): the coefficient of w^(k-1) is ext[k+2], that of w^(k-3) is ext[k].  (Selecting the operands
    // with nested conditionals over references instead gave wrong products in the gfx950 build while the host build was right.)
    e2 ext[9];
    for (int j = 0; j < 3; j++) ext[j] = mulxi(f.c[j + 3]);
    for (int j = 0; j < 6; j++) ext[j + 3] = f.c[j];
    F12 r;
    for (int k = 0; k < 6; k++) r.c[k] = red2(acc2(acc2(mul2(ext[k + 3], c0), mul2(ext[k + 2], c1)), mul2(ext[k], c3)));
    return r;
}
DEVFN F12 conj12(const F12& a) { F12 r = a; r.c[1] = neg2(a.c[1]); r.c[3] = neg2(a.c[3]); r.c[5] = neg2(a.c[5]); return r; }      // x^(p^6)
DEVNOINL F12 frob12(const F12& a) {      // x^p
    F12 r; r.c[0] = conj2(a.c[0]);
#pragma unroll
    for (int i = 1; i < 6; i++) r.c[i] = mul2(conj2p(a.c[i]), frob1(i));
    return r;
}
DEVFN F12 frob12_2(const F12& a) {    // x^(p^2)
    F12 r; r.c[0] = a.c[0];
#pragma unroll
    for (int i = 1; i < 6; i++) r.c[i] = scale2(a.c[i], frob2c(i));
    return r;
}
struct F6 { e2 a, b, c; };
DEVFN F6 mul6(const F6& x, const F6& y) {
    return F6{add2(mul2(x.a, y.a), mulxi(add2(mul2(x.b, y.c), mul2(x.c, y.b)))),
              add2(add2(mul2(x.a, y.b), mul2(x.b, y.a)), mulxi(mul2(x.c, y.c))),
              add2(add2(mul2(x.a, y.c), mul2(x.b, y.b)), mul2(x.c, y.a))};
}
DEVFN F6 inv6(const F6& x) {
    const e2 t0 = sub2(sqr2(x.a), mulxi(mul2(x.b, x.c))), t1 = sub2(mulxi(sqr2(x.c)), mul2(x.a, x.b)), t2 = sub2(sqr2(x.b), mul2(x.a, x.c));
    const e2 n = inv2(add2(mul2(x.a, t0), mulxi(add2(mul2(x.c, t1), mul2(x.b, t2)))));
    return F6{mul2(t0, n), mul2(t1, n), mul2(t2, n)};
}
DEVNOINL F12 inv12(const F12& x) {      // x = A + w B, 1/x = (A - w B) / (A^2 - v B^2)
    const F6 A{x.c[0], x.c[2], x.c[4]}, B{x.c[1], x.c[3], x.c[5]};
    const F6 A2 = mul6(A, A), B2 = mul6(B, B);
    const F6 n = inv6(F6{sub2(A2.a, mulxi(B2.c)), sub2(A2.b, B2.a), sub2(A2.c, B2.b)});
    const F6 ra = mul6(A, n), rb = mul6(B, n);
    F12 r; r.c[0] = ra.a; r.c[2] = ra.b; r.c[4] = ra.c; r.c[1] = neg2(rb.a); r.c[3] = neg2(rb.b); r.c[5] = neg2(rb.c);
    return r;
}
DEVFN bool is_one12(const F12& a) {
    bool ok = eq1(a.c[0].a0, F::one()) && zero1(a.c[0].a1);
#pragma unroll
    for (int i = 1; i < 6; i++) ok = ok && zero2(a.c[i]);
    return ok;
}
DEVNOINL F12 pow_x(const F12& a) {      // a^x, x = 0x44E992B44A6909F1 (63 bits)
    F12 acc = a;
    for (int i = 61; i >= 0; i--) {
        acc = sqr12(acc);
        if ((kX >> i) & 1) acc = mul12(acc, a);
    }
    return acc;
}
// f^((p^12 - 1) / r): easy part (p^6 - 1)(p^2 + 1), hard part (p^4 - p^2 + 1) / r = l0 + l1 p + l2 p^2 + p^3 with l2 = 6x^2 + 1,
// l1 = -36x^3 - 18x^2 - 12x + 1, l0 = -36x^3 - 30x^2 - 18x - 2 (Scott et al., "On the final exponentiation for calculating pairings
// on ordinary elliptic curves", 2009): three exponentiations by x and a fixed chain; inverses are conjugates in the cyclotomic
// subgroup.  The exponent is exactly the reduced pairing's (m = 1).
DEVNOINL F12 final_exp(const F12& f) {
    const F12 e1v = mul12(conj12(f), inv12(f));
    const F12 g = mul12(frob12_2(e1v), e1v);
    F12 fx = g, fx2 = g, fx3 = g, cur = g;
    for (int k = 0; k < 3; k++) {      // one copy of pow_x, three passes
        cur = pow_x(cur);
        if (k == 0) fx = cur; else if (k == 1) fx2 = cur; else fx3 = cur;
    }
    const F12 fp2 = frob12_2(g);
    const F12 y0 = mul12(mul12(frob12(g), fp2), frob12(fp2));
    const F12 y1 = conj12(g);
    const F12 y2 = frob12_2(fx2);
    const F12 y3 = conj12(frob12(fx));
    const F12 y4 = conj12(mul12(fx, frob12(fx2)));
    const F12 y5 = conj12(fx2);
    const F12 y6 = conj12(mul12(fx3, frob12(fx3)));
    F12 t0 = mul12(mul12(sqr12(y6), y4), y5);
    F12 t1 = mul12(mul12(y3, y5), t0);
    t0 = mul12(t0, y2);
    t1 = sqr12(mul12(sqr12(t1), t0));
    t0 = mul12(t1, y1);
    t1 = mul12(t1, y0);
    return mul12(sqr12(t0), t1);
}

// ---- Miller loop ----
// T in Jacobian coordinates (x = X/Z^2, y = Y/Z^3).  Each step returns its line scaled by an Fp2 factor (Z-powers, 2Y, H), which
// the final exponentiation removes: doubling l = 2YZ^3 yP - 3X^2Z^2 xP w + (3X^3 - 2Y^2) w^3, addition of affine Q
// l = ZH yP - R xP w + (R xQ - yQ ZH) w^3.
struct G2J { e2 X, Y, Z; };
DEVNOINL Line dbl_step(G2J& T) {
    const e2 XX = sqr2(T.X), YY = sqr2(T.Y), ZZ = sqr2(T.Z);
    Line l;
    l.a = mul2(small2(T.Y, 2), mul2(T.Z, ZZ));
    l.b = neg2(mul2(small2(XX, 3), ZZ));
    l.c = sub2(mul2(small2(XX, 3), T.X), small2(YY, 2));
    // dbl-2009-l
    const e2 C = sqr2(YY);
    const e2 D = small2(sub2(sub2(sqr2(add2(T.X, YY)), XX), C), 2);
    const e2 E = small2(XX, 3), Fv = sqr2(E);
    const e2 X3 = sub2(Fv, small2(D, 2));
    const e2 Y3 = sub2(mul2(E, sub2(D, X3)), small2(C, 8));
    const e2 Z3 = small2(mul2(T.Y, T.Z), 2);
    T = G2J{X3, Y3, Z3};
    return l;
}
DEVNOINL Line add_step(G2J& T, const e2& qx, const e2& qy) {
    const e2 ZZ = sqr2(T.Z), U2 = mul2(qx, ZZ), S2 = mul2(qy, mul2(T.Z, ZZ));
    const e2 H = sub2(U2, T.X), R = sub2(S2, T.Y), ZH = mul2(T.Z, H);
    Line l;
    l.a = ZH;
    l.b = neg2(R);
    l.c = sub2(mul2(R, qx), mul2(qy, ZH));
    const e2 HH = sqr2(H), HHH = mul2(H, HH), V = mul2(T.X, HH);
    const e2 X3 = sub2(sub2(sqr2(R), HHH), small2(V, 2));
    const e2 Y3 = sub2(mul2(R, sub2(V, X3)), mul2(T.Y, HHH));
    T = G2J{X3, Y3, ZH};
    return l;
}
// pi(Q) and -pi^2(Q) on the twist (libverify's q1 / q2)
DEVFN void frob_points(const VP2& q, e2& q1x, e2& q1y, e2& q2x, e2& q2y) {
    q1x = mul2(conj2p(q.x), frob_g2()); q1y = mul2(conj2p(q.y), frob_g3());
    q2x = mul2(conj2p(q1x), frob_g2()); q2y = neg2(mul2(conj2p(q1y), frob_g3()));
}
// the kLineSteps lines of the Miller loop for one G2 point (the fixed points of a key; also how the loop itself walks)
DEVFN void lines_of(const VP2& q, Line* out) {
    G2J T{q.x, q.y, F2::one()};
    int s = 0;
    for (int i = kLoopSteps - 1; i >= 0; i--) {
        out[s++] = dbl_step(T);
        if ((loop_bits() >> i) & 1) out[s++] = add_step(T, q.x, q.y);
    }
    e2 q1x, q1y, q2x, q2y; frob_points(q, q1x, q1y, q2x, q2y);
    out[s++] = add_step(T, q1x, q1y);
    out[s++] = add_step(T, q2x, q2y);
}
DEVFN F12 apply_line(const F12& f, const Line& l, const VP1& p) {
    return mul_line(f, scale2(l.a, p.y), scale2(l.b, p.x), l.c);
}
// prod_k e(P_k, Q_k) before the final exponentiation.  var: the proof's own pair (lines computed on the fly, skipped when either
// point is infinity); fixed[k]: kLineSteps precomputed lines each, skipped when fixed_inf[k] or P_k is infinity.
template <int NFIXED>
DEVFN F12 miller(const VP1& vp, const VP2& vq, bool use_var, const VP1 (&fp)[NFIXED], const Line* const (&lines)[NFIXED], const bool (&fixed_inf)[NFIXED]) {
    const bool var = use_var && !vp.inf && !vq.inf;
    bool fon[NFIXED];
#pragma unroll
    for (int k = 0; k < NFIXED; k++) fon[k] = !fixed_inf[k] && !fp[k].inf;
    F12 f = one12();
    G2J T{vq.x, vq.y, F2::one()};
    int s = 0;
    for (int i = kLoopSteps - 1; i >= -2; i--) {
        // i >= 0: doubling step of bit i (then its addition when set); i = -1, -2: the two Frobenius additions
        const int nsub = (i >= 0) ? (1 + (int)((loop_bits() >> i) & 1)) : 1;
        if (i >= 0) f = sqr12(f);
        for (int sub = 0; sub < nsub; sub++, s++) {
            if (var) {
                Line l;
                if (i >= 0 && sub == 0) l = dbl_step(T);
                else if (i >= 0) l = add_step(T, vq.x, vq.y);
                else {
                    e2 q1x, q1y, q2x, q2y; frob_points(vq, q1x, q1y, q2x, q2y);
                    l = (i == -1) ? add_step(T, q1x, q1y) : add_step(T, q2x, q2y);
                }
                f = apply_line(f, l, vp);
            }
            for (int k = 0; k < NFIXED; k++) if (fon[k]) f = apply_line(f, lines[k][s], fp[k]);
        }
    }
    return f;
}

// ---- public inputs ----
// L = K0 + sum_w table[w][win[w]] (+ the AES commitment terms, added by the caller)
DEVFN G1X lsum(const VP1& k0, const VP1* table, const uint8_t* win, int nwin) {
    G1X acc = g1_inf();
    acc = g1_madd(acc, k0);
    for (int w = 0; w < nwin; w++) acc = g1_madd(acc, table[256 * w + win[w]]);
    return acc;
}
// hash_to_field(D) mod r as 32 little-endian bytes (D = infinity hashes the all-zero message with 0x40 in front, as libverify)
DEVFN void commitment_challenge(const VP1& d, uint8_t out[32]) {
    uint32_t msg[16], h[12];
    if (d.inf) { for (int i = 0; i < 16; i++) msg[i] = 0; msg[0] = 0x40000000u; }
    else {
        const fe x = F::pack(F::from_mont(d.x)), y = F::pack(F::from_mont(d.y));
        for (int i = 0; i < 8; i++) { msg[7 - i] = x.l[i]; msg[15 - i] = y.l[i]; }
    }
    gsc::xmd::commitment_xmd(msg, h);
    using R = bn254::Fr29;
    fe9 acc = R::zero();
    const fe9 w32 = R::mul(R::from_u32(65536), R::from_u32(65536));
    for (int i = 0; i < 12; i++) acc = R::norm(R::add(R::mul(acc, w32), R::from_u32(h[i])));
    const fe c = R::pack(R::from_mont(acc));
    for (int i = 0; i < 8; i++) for (int j = 0; j < 4; j++) out[4 * i + j] = (uint8_t)(c.l[i] >> (8 * j));
}


// one entry of a window table: ChaCha20 — subset sum of K[first + t] over the bits t of v; AES — v 2^shift K[first]
DEVFN VP1 table_entry(bool subset, const VP1* K, uint32_t first, uint32_t shift, uint32_t v) {
    if (!subset) return g1_small_mul(K[first], v, (int)shift);
    G1X acc = g1_inf();
    for (int t = 0; t < 8; t++) if ((v >> t) & 1) acc = g1_madd(acc, K[first + t]);
    return g1_affine(acc);
}

// ---- one proof ----
// what the key contributes on the device; the pointers are device memory (host memory in the native check)
struct KeyDev {
    VP1 k0, alpha;
    const VP1* table;            // kWindows x 256 public-input entries
    const VP1* ctable;           // kCommitWindows x 256 multiples of the commitment base (AES)
    const Line* lines[5];        // beta, gamma, delta, ped_g, ped_gsn: kLineSteps each
    int32_t qinf[5];             // that G2 point is infinity
    int32_t has_commitment, fits;
};
struct ProofDev { VP1 A, C, L, D, pok; VP2 B; int32_t ok; };
constexpr int kProofSlot = 196;
// What follows the decode of a proof's points, whichever form they came in (prep_one, prep_affine_one): L = K0 + sum of window entries
// (+ c K[npub+1] + D with the challenge c of the decoded D)
DEVFN void prep_finish(const KeyDev& k, const uint8_t* win, ProofDev& out) {
    G1X acc = lsum(k.k0, k.table, win, kWindows);
    if (k.has_commitment) {
        uint8_t c[32];
        commitment_challenge(out.D, c);
        for (int j = 0; j < kCommitWindows; j++) acc = g1_madd(acc, k.ctable[256 * j + c[j]]);
        acc = g1_madd(acc, out.D);
    }
    out.L = g1_affine(acc);
    out.ok = 1;
}
// strict decoding of A, B (with the subgroup test), C (and D, PoK), then prep_finish
DEVFN void prep_one(const KeyDev& k, const uint8_t* proof, const uint8_t* win, ProofDev& out) {
    out.ok = 0;
    if (!k.fits) return;
    if (decode_g1(proof, out.A) < 0 || decode_g2(proof + 32, out.B) < 0 || decode_g1(proof + 96, out.C) < 0) return;
    // the proof of knowledge follows the commitments; libverify decodes it (and refuses a bad encoding) even without a commitment
    if (decode_g1(proof + (k.has_commitment ? 164 : 132), out.pok) < 0) return;
    if (k.has_commitment && decode_g1(proof + 132, out.D) < 0) return;
    prep_finish(k, win, out);
}
// ---- the prover's own output, before it is compressed (k_prove_check.hip) ----
// A finite affine point as the prover leaves it: canonical coordinates (< p) that satisfy the curve equation exactly, no square root.  Such a
// point is what decode_g1 / decode_g2_curve return for its compressed encoding (the encoding keeps x and the sign of y, and the curve has one
// y of that sign for x), and a point off the curve is not: its encoding decodes to another point or to none.  So accepting these points is
// accepting the bytes serialisation will write.
DEVFN bool affine_g1(const fe& xw, const fe& yw, VP1& p) {
    p.x = F::zero(); p.y = F::zero(); p.inf = 1;
    e1 x, y;
    if (!fp_from_words(xw, x) || !fp_from_words(yw, y)) return false;
    if (!eq1(F::sqr(y), red(F::add(F::mul(F::sqr(x), x), three1())))) return false;
    p.x = x; p.y = y; p.inf = 0;
    return true;
}
DEVFN bool affine_g2_curve(const fe& x0, const fe& x1, const fe& y0, const fe& y1, VP2& p) {      // without the subgroup test
    p.x = F2::zero(); p.y = F2::zero(); p.inf = 1;
    e2 x, y;
    if (!fp_from_words(x0, x.a0) || !fp_from_words(x1, x.a1) || !fp_from_words(y0, y.a0) || !fp_from_words(y1, y.a1)) return false;
    if (!eq2(sqr2(y), add2(mul2(sqr2(x), x), twist_b()))) return false;
    p.x = x; p.y = y; p.inf = 0;
    return true;
}
DEVFN fe words_le(const uint8_t* b) { fe w;      // eight little-endian words (the layout of Lane::d_out)
#pragma unroll
    for (int i = 0; i < 8; i++) w.l[i] = (uint32_t)b[4 * i] | ((uint32_t)b[4 * i + 1] << 8) | ((uint32_t)b[4 * i + 2] << 16) | ((uint32_t)b[4 * i + 3] << 24);
    return w; }
DEVFN fe words_be(const uint8_t* b) { fe w;      // 32 big-endian bytes (the layout points_to_affine_be leaves)
#pragma unroll
    for (int i = 0; i < 8; i++) { const uint8_t* q = b + 28 - 4 * i; w.l[i] = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | q[3]; }
    return w; }
// prep_one's twin on the prover's buffers.  abc: 256 bytes, eight canonical little-endian words per coordinate: A.x A.y | B.x.a0 B.x.a1 B.y.a0
// B.y.a1 | C.x C.y.  d_be, pok_be: X | Y as 64 big-endian bytes each (read only for a key with a commitment; without one the proof of
// knowledge is the point at infinity, as the proof bytes say).  The caller has excluded the statements whose infinity flags are set.
DEVFN void prep_affine_one(const KeyDev& k, const uint8_t* abc, const uint8_t* d_be, const uint8_t* pok_be, const uint8_t* win, ProofDev& out) {
    out.ok = 0;
    if (!k.fits) return;
    if (!affine_g1(words_le(abc), words_le(abc + 32), out.A)) return;
    if (!affine_g2_curve(words_le(abc + 64), words_le(abc + 96), words_le(abc + 128), words_le(abc + 160), out.B) || !g2_in_subgroup(out.B)) return;
    if (!affine_g1(words_le(abc + 192), words_le(abc + 224), out.C)) return;
    if (k.has_commitment) {
        if (!affine_g1(words_be(pok_be), words_be(pok_be + 32), out.pok) || !affine_g1(words_be(d_be), words_be(d_be + 32), out.D)) return;
    } else { out.pok.x = F::zero(); out.pok.y = F::zero(); out.pok.inf = 1; }
    prep_finish(k, win, out);
}
DEVFN VP1 neg_p(const VP1& p) { VP1 r = p; r.y = neg1(p.y); return r; }
// pass 0 (keys with a commitment): e(D, ped_gsn) e(PoK, ped_g) == 1; pass 1: e(A, B) e(-alpha, beta) e(-L, gamma) e(-C, delta) == 1.
// One copy of the Miller loop and of the final exponentiation serves both.  f_out (optional): pass 1's reduced value.
DEVFN bool pair_one(const KeyDev& k, const ProofDev& p, F12* f_out) {
    bool ok = p.ok && k.fits;
    for (int pass = k.has_commitment ? 0 : 1; pass < 2 && ok; pass++) {
        VP1 fp[3]; const Line* ln[3]; bool finf[3];
        if (pass == 0) {
            fp[0] = p.D; ln[0] = k.lines[4]; finf[0] = k.qinf[4];
            fp[1] = p.pok; ln[1] = k.lines[3]; finf[1] = k.qinf[3];
            fp[2] = p.D; ln[2] = k.lines[0]; finf[2] = true;
        } else {
            fp[0] = neg_p(k.alpha); ln[0] = k.lines[0]; finf[0] = k.qinf[0];
            fp[1] = neg_p(p.L); ln[1] = k.lines[1]; finf[1] = k.qinf[1];
            fp[2] = neg_p(p.C); ln[2] = k.lines[2]; finf[2] = k.qinf[2];
        }
        const F12 f = final_exp(miller<3>(p.A, p.B, pass == 1, fp, ln, finf));
        if (pass == 1 && f_out) *f_out = f;
        ok = is_one12(f);
    }
    return ok;
}


}  // namespace vfy
}  // namespace gsc
