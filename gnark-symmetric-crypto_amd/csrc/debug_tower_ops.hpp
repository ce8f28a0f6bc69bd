// TEST HOOKS: one element of gsc_debug_tower_ops (include/libprove.h): the verifier's Fp / Fp2 helpers, its Fp12 tower, the Miller
// steps and the final exponentiation, one operation at a time on RAW limbs (9 x int32 per Fp value, 2^261 Montgomery domain, used
// exactly as given).  tower_op is the serial per-thread code of verify_dev.hpp (path 0); tower_group_op is the lane-sliced code of
// verify_few_dev.hpp on a group G (path 1: WaveGroup in the hook kernel of k_debug_tower.hip, HostGroup in tests/native/tower_check.cpp,
// which builds the same functions for the host so that the case tables and references of tests/devref.py are proven on a CPU before
// the device code is judged by them).  No production kernel includes this.
#pragma once
#include "verify_few_dev.hpp"

namespace gsc {
namespace vfy {
namespace dbg {

enum {
    T_RED = 0, T_LIN, T_ADD2, T_SUB2, T_NEG2, T_CONJ2, T_MUL2, T_SQR2, T_SCALE2, T_MULXI, T_SMALL2, T_INV1, T_INV2, T_SQRT1, T_SQRT2, T_LEX_LARGE2,
    T_MUL12, T_SQR12, T_MUL_LINE, T_CONJ12, T_FROB12, T_FROB12_2, T_INV12, T_POW_X, T_FINAL_EXP, T_IS_ONE12,
    T_DBL_STEP, T_ADD_STEP, T_FROB_POINTS, T_LINES_OF, T_OPS
};
constexpr int kW1 = 9, kW2 = 18, kW12 = 108, kWLine = 54;      // int32 words of an Fp, Fp2, Fp12 value and of a line
constexpr int kWGroup = few::kGroup * kW2;                     // path 1 returns every lane's slice, the two pad lanes included
static_assert(sizeof(Line) == 4 * kWLine && sizeof(e2) == 4 * kW2, "lines and Fp2 values are plain limbs");

constexpr bool tower_has(int path, int op) { return path == 0 ? (op >= 0 && op < T_OPS) : path == 1 ? (op >= T_MUL12 && op <= T_IS_ONE12) : false; }
// words one element reads:  lin a, b, ka, kb;  scale2 a, k;  small2 a, k;  mul_line f, c0, c1, c3;  dbl_step X, Y, Z;  add_step X, Y, Z, xQ, yQ;
// frob_points / lines_of xQ, yQ
constexpr int tower_in_words(int op) {
    switch (op) {
        case T_RED: case T_INV1: case T_SQRT1: return kW1;
        case T_LIN: return 2 * kW1 + 2;
        case T_ADD2: case T_SUB2: case T_MUL2: case T_FROB_POINTS: case T_LINES_OF: return 2 * kW2;
        case T_SCALE2: return kW2 + kW1;
        case T_SMALL2: return kW2 + 1;
        case T_MUL12: return 2 * kW12;
        case T_MUL_LINE: return kW12 + 3 * kW2;
        case T_DBL_STEP: return 3 * kW2;
        case T_ADD_STEP: return 5 * kW2;
        default: return op >= T_MUL12 ? kW12 : kW2;
    }
}
// words one element writes:  the steps T' (X, Y, Z) and the line (a, b, c);  frob_points x1, y1, x2, y2;  lines_of kLineSteps lines
constexpr int tower_out_words(int path, int op) {
    switch (op) {
        case T_RED: case T_LIN: case T_INV1: case T_SQRT1: return kW1;
        case T_LEX_LARGE2: case T_IS_ONE12: return 0;
        case T_DBL_STEP: case T_ADD_STEP: return 3 * kW2 + kWLine;
        case T_FROB_POINTS: return 4 * kW2;
        case T_LINES_OF: return kLineSteps * kWLine;
        default: return op >= T_MUL12 ? (path == 1 ? kWGroup : kW12) : kW2;
    }
}

DEVFN e1 ld1(const int32_t* p) { e1 r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = p[i];
    return r; }
DEVFN e2 ld2(const int32_t* p) { return e2{ld1(p), ld1(p + kW1)}; }
DEVFN void st1(int32_t* p, const e1& a) {
#pragma unroll
    for (int i = 0; i < 9; i++) p[i] = a.l[i]; }
DEVFN void st2(int32_t* p, const e2& a) { st1(p, a.a0); st1(p + kW1, a.a1); }
DEVFN F12 ld12(const int32_t* p) { F12 r; for (int i = 0; i < 6; i++) r.c[i] = ld2(p + kW2 * i); return r; }
DEVFN void st12(int32_t* p, const F12& a) { for (int i = 0; i < 6; i++) st2(p + kW2 * i, a.c[i]); }
DEVFN void st_step(int32_t* p, const G2J& T, const Line& l) {
    st2(p, T.X); st2(p + kW2, T.Y); st2(p + 2 * kW2, T.Z); st2(p + 3 * kW2, l.a); st2(p + 4 * kW2, l.b); st2(p + 5 * kW2, l.c);
}

// path 0: the flag of sqrt1 / sqrt2 (a root was found; zeros are written when not), lex_large2 and is_one12, 0 for every other op
DEVFN uint32_t tower_op(int op, const int32_t* in, int32_t* out) {
    switch (op) {
        case T_RED: st1(out, red(ld1(in))); return 0;
        case T_LIN: st1(out, lin(ld1(in), in[2 * kW1], ld1(in + kW1), in[2 * kW1 + 1])); return 0;
        case T_ADD2: st2(out, add2(ld2(in), ld2(in + kW2))); return 0;
        case T_SUB2: st2(out, sub2(ld2(in), ld2(in + kW2))); return 0;
        case T_NEG2: st2(out, neg2(ld2(in))); return 0;
        case T_CONJ2: st2(out, conj2(ld2(in))); return 0;
        case T_MUL2: st2(out, mul2(ld2(in), ld2(in + kW2))); return 0;
        case T_SQR2: st2(out, sqr2(ld2(in))); return 0;
        case T_SCALE2: st2(out, scale2(ld2(in), ld1(in + kW2))); return 0;
        case T_MULXI: st2(out, mulxi(ld2(in))); return 0;
        case T_SMALL2: st2(out, small2(ld2(in), in[kW2])); return 0;
        case T_INV1: st1(out, inv1(ld1(in))); return 0;
        case T_INV2: st2(out, inv2(ld2(in))); return 0;
        case T_SQRT1: { e1 r = F::zero(); const bool ok = sqrt1(ld1(in), r); st1(out, r); return ok; }
        case T_SQRT2: { e2 r = F2::zero(); const bool ok = sqrt2(ld2(in), r); st2(out, r); return ok; }
        case T_LEX_LARGE2: return lex_large2(ld2(in));
        case T_MUL12: st12(out, mul12(ld12(in), ld12(in + kW12))); return 0;
        case T_SQR12: st12(out, sqr12(ld12(in))); return 0;
        case T_MUL_LINE: st12(out, mul_line(ld12(in), ld2(in + kW12), ld2(in + kW12 + kW2), ld2(in + kW12 + 2 * kW2))); return 0;
        case T_CONJ12: st12(out, conj12(ld12(in))); return 0;
        case T_FROB12: st12(out, frob12(ld12(in))); return 0;
        case T_FROB12_2: st12(out, frob12_2(ld12(in))); return 0;
        case T_INV12: st12(out, inv12(ld12(in))); return 0;
        case T_POW_X: st12(out, pow_x(ld12(in))); return 0;
        case T_FINAL_EXP: st12(out, final_exp(ld12(in))); return 0;
        case T_IS_ONE12: return is_one12(ld12(in));
        case T_DBL_STEP: { G2J T{ld2(in), ld2(in + kW2), ld2(in + 2 * kW2)}; const Line l = dbl_step(T); st_step(out, T, l); return 0; }
        case T_ADD_STEP: { G2J T{ld2(in), ld2(in + kW2), ld2(in + 2 * kW2)}; const Line l = add_step(T, ld2(in + 3 * kW2), ld2(in + 4 * kW2)); st_step(out, T, l); return 0; }
        case T_FROB_POINTS: {
            VP2 q; q.x = ld2(in); q.y = ld2(in + kW2); q.inf = 0;
            e2 r[4]; frob_points(q, r[0], r[1], r[2], r[3]);
            for (int i = 0; i < 4; i++) st2(out + kW2 * i, r[i]);
            return 0;
        }
        case T_LINES_OF: { VP2 q; q.x = ld2(in); q.y = ld2(in + kW2); q.inf = 0; lines_of(q, reinterpret_cast<Line*>(out)); return 0; }
        default: return 0;
    }
}

// path 1: `in` is the group's element, or nullptr for a group without one, which computes on the identity (and on zero line
// coefficients) as the production kernels do.  Returns the value (every lane its slice) and is_one12's flag.
template <class G> DEVFN typename G::V tower_group_op(const G& g, int op, const int32_t* in, bool& flag) {
    using V = typename G::V;
    const V a = g.each([&](int k) { return in ? ld2(in + kW2 * k) : (k == 0 ? F2::one() : F2::zero()); });
    flag = false;
    switch (op) {
        case T_MUL12: { const V b = g.each([&](int k) { return in ? ld2(in + kW12 + kW2 * k) : (k == 0 ? F2::one() : F2::zero()); }); return few::mul12(g, a, b); }
        case T_SQR12: return few::sqr12(g, a);
        case T_MUL_LINE: {
            e2 c[3];
            for (int j = 0; j < 3; j++) c[j] = in ? ld2(in + kW12 + kW2 * j) : F2::zero();
            return few::mul_line(g, a, c[0], c[1], c[2]);
        }
        case T_CONJ12: return few::conj12(g, a);
        case T_FROB12: return few::frob12(g, a);
        case T_FROB12_2: return few::frob12_2(g, a);
        case T_INV12: return few::inv12(g, a);
        case T_POW_X: return few::pow_x(g, a);
        case T_FINAL_EXP: return few::final_exp(g, a);
        default: flag = few::is_one12(g, a); return a;
    }
}

}  // namespace dbg
}  // namespace vfy
}  // namespace gsc
