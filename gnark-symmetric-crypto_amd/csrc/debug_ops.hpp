// TEST HOOKS: one element of gsc_debug_limb_ops / gsc_debug_curve_ops (include/libprove.h).  The hook kernels of k_init.hip call these
// per thread; tests/native builds the same functions for the host, where the products of bn254_fp29.hpp are plain C, so that the case
// tables and the references of the tests are proven on a CPU before the device code is judged by them; and the element function that returns the sums of the
// hooks gsc_debug_msm / gsc_debug_assemble (device builds only).  No production kernel includes this.
#pragma once
#include "bn254_fp29.hpp"

namespace bn254 {
namespace dbg {

// ---- raw limbs in, raw limbs out: the operands are used exactly as given (no to_mont, no freeze, no pack) ----
enum { LIMB_MUL = 0, LIMB_SQR = 1, LIMB_FMMS = 2, LIMB_NORM = 3, LIMB_FREEZE = 4, LIMB_FREEZE_NEAR = 5, LIMB_OPS = 6 };

template <class F>
DEVFN fe9 limb_op(int op, const fe9& a, const fe9& b, const fe9& c, const fe9& d) {
    switch (op) {
        case LIMB_MUL: return F::mul(a, b);
        case LIMB_SQR: return F::sqr(a);
        case LIMB_FMMS: return F::fmms(a, b, c, d);
        case LIMB_NORM: return F::norm(a);
        case LIMB_FREEZE: return F::freeze(a);
        default: return F::freeze_near(a);
    }
}

// ---- the XYZZ group law of Curve9<F> on canonical affine inputs ----
// The operands are built (Montgomery form, the scale) with the plain-C products of Field29 / Fp2x, never with the products under test.
template <class F> struct CurveIO;
template <> struct CurveIO<Fp29f> {
    using B = Fp29;
    DEVFN static fe9 in(const fe* p) { return Fp29::to_mont(Fp29::unpack(p[0])); }
    DEVFN static void out(fe* p, const fe9& a) { p[0] = Fp29::pack(Fp29::from_mont(a)); }
    DEVFN static void out_zero(fe* p) { p[0] = Fp29::pack(Fp29::zero()); }
};
template <> struct CurveIO<Fp2x> {
    using B = Fp2x;
    DEVFN static fe9x2 in(const fe* p) { return fe9x2{Fp29::to_mont(Fp29::unpack(p[0])), Fp29::to_mont(Fp29::unpack(p[1]))}; }
    DEVFN static void out(fe* p, const fe9x2& a) { p[0] = Fp29::pack(Fp29::from_mont(a.a0)); p[1] = Fp29::pack(Fp29::from_mont(a.a1)); }
    DEVFN static void out_zero(fe* p) { p[0] = p[1] = Fp29::pack(Fp29::zero()); }
};

enum { CURVE_DBL = 0, CURVE_MADD_EXACT = 1, CURVE_MADD_FAST = 2, CURVE_ADD = 3, CURVE_TO_AFF = 4, CURVE_PARTIAL_SUMS = 5, CURVE_OPS = 6 };
enum { CURVE_FLAG_INF = 1, CURVE_FLAG_ZZ0_FIRST = 2, CURVE_FLAG_ZZ0_LAST = 4 };

template <class F> DEVFN Aff9<F> curve_aff(const fe* pt) { return Aff9<F>{CurveIO<F>::in(pt), CurveIO<F>::in(pt + F::WORDS)}; }
// (x, y) -> (x l^2, y l^3, l^2, l^3): the same point with ZZ != 1
template <class F> DEVFN Xyzz9<F> curve_xyzz(const fe* pt, bool inf, const fe* lam) {
    using B = typename CurveIO<F>::B;
    if (inf) return Curve9<F>::infinity();
    const Aff9<F> a = curve_aff<F>(pt);
    const typename F::E l = CurveIO<F>::in(lam), l2 = B::sqr(l), l3 = B::mul(l2, l);
    return Xyzz9<F>{B::mul(a.x, l2), B::mul(a.y, l3), l2, l3, false};
}

// pts: k canonical affine points (2 * F::WORDS values each), inf: their infinity flags, lam: the scales of points 0 and 1 where those
// enter as XYZZ operands (F::WORDS values each, non-zero).  out: the canonical affine result (zeros when there is none).  Returns flags.
//   DBL          k = 1   dbl(X0)
//   MADD_EXACT   k >= 2  acc = X0; acc = madd<true>(acc, P_j), j = 1..k-1
//   MADD_FAST    k >= 2  the same with madd<false>; ZZ0_FIRST: ZZ == 0 mod p after the first addition, ZZ0_LAST: after the last one
//                        (no affine result then)
//   ADD          k = 2   add(X0, X1)
//   TO_AFF       k = 1   to_aff(X0)
//   PARTIAL_SUMS k >= 1  four accumulators from infinity, P_j into accumulator j mod 4 with madd<true>, then add(add(s0, s1), add(s2, s3))
// Points that enter as AFFINE operands cannot be infinity (the caller checks that).
template <class F>
DEVFN uint32_t curve_op(int op, size_t k, const fe* pts, const uint8_t* inf, const fe* lam, fe* out) {
    using C = Curve9<F>;
    constexpr int W = F::WORDS;
    uint32_t flags = 0;
    Xyzz9<F> r = op == CURVE_PARTIAL_SUMS ? C::infinity() : curve_xyzz<F>(pts, inf[0] != 0, lam);
    switch (op) {
        case CURVE_DBL: r = C::dbl(r); break;
        case CURVE_MADD_EXACT:
            for (size_t j = 1; j < k; j++) r = C::template madd<true>(r, curve_aff<F>(pts + 2 * W * j));
            break;
        case CURVE_MADD_FAST:
            for (size_t j = 1; j < k; j++) {
                r = C::template madd<false>(r, curve_aff<F>(pts + 2 * W * j));
                if (j == 1 && F::is_zero(r.zz)) flags |= CURVE_FLAG_ZZ0_FIRST;
            }
            if (F::is_zero(r.zz)) flags |= CURVE_FLAG_ZZ0_LAST;
            break;
        case CURVE_ADD: r = C::add(r, curve_xyzz<F>(pts + 2 * W, inf[1] != 0, lam + W)); break;
        case CURVE_PARTIAL_SUMS: {
            Xyzz9<F> s[4] = {r, r, r, r};
            for (size_t j = 0; j < k; j++) s[j & 3] = C::template madd<true>(s[j & 3], curve_aff<F>(pts + 2 * W * j));
            r = C::add(C::add(s[0], s[1]), C::add(s[2], s[3]));
            break;
        }
        default: break;      // TO_AFF
    }
    if (r.inf) flags |= CURVE_FLAG_INF;
    if (r.inf || (flags & CURVE_FLAG_ZZ0_LAST)) { CurveIO<F>::out_zero(out); CurveIO<F>::out_zero(out + W); return flags; }
    const Aff9<F> a = C::to_aff(r);
    CurveIO<F>::out(out, a.x); CurveIO<F>::out(out + W, a.y);
    return flags;
}

#ifdef __HIPCC__
// The results of the hooks gsc_debug_msm and gsc_debug_assemble, one element: out[i] = the XYZZ sum sums[i] as canonical little-endian coordinates
// (G1 x, y; G2 x.a0, x.a1, y.a0, y.a1); inf[i] = 1 and zeros for the point at infinity
template <class F>
DEVFN void sum_out(const fe* sums, size_t i, fe* out, uint8_t* inf) {
    using C = Curve9<F>;
    const Xyzz9<F> v = C::load_xyzz(sums + i * (4 * F::WORDS));
    fe* o = out + i * (2 * F::WORDS);
    if (v.inf) { inf[i] = 1; for (int q = 0; q < 2 * F::WORDS; q++) store_fe(o + q, fe{}); return; }
    inf[i] = 0;
    const Aff9<F> a = C::to_aff(v);
    if constexpr (F::WORDS == 1) { store_fe(o, Fp29::pack(Fp29::from_mont(a.x))); store_fe(o + 1, Fp29::pack(Fp29::from_mont(a.y))); }
    else {
        store_fe(o, Fp29::pack(Fp29::from_mont(a.x.a0))); store_fe(o + 1, Fp29::pack(Fp29::from_mont(a.x.a1)));
        store_fe(o + 2, Fp29::pack(Fp29::from_mont(a.y.a0))); store_fe(o + 3, Fp29::pack(Fp29::from_mont(a.y.a1)));
    }
}
#endif

}  // namespace dbg
}  // namespace bn254
