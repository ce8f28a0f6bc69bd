// Building blocks shared by the MSM kernels (k_msm_win.hip, k_msm.hip) and by the transform kernel that writes MSM digits itself
// (k_ntt.hip): ONE definition each of the signed-digit step, the octet slot, the table gather, the wave sum, the escape and the slice
// geometry.  The design note of the MSM is the header of k_msm_win.hip.
#pragma once
#include "kernels.hpp"
#include "bn254_fp29.hpp"

namespace gsc {
using namespace bn254;

// The device fields behind a group's point types: F for the radix-2^29 arithmetic, Old for the 8 x 32-bit images in memory
template <class PointT> struct GroupOf;
template <> struct GroupOf<G1Aff> { using F = Fp29f; using Old = Fp; };
template <> struct GroupOf<G2Aff> { using F = Fp2x; using Old = Fp2; };
template <> struct GroupOf<G1Xyzz> : GroupOf<G1Aff> {};
template <> struct GroupOf<G2Xyzz> : GroupOf<G2Aff> {};

// |s| <= (r-1)/2 after sign normalisation; returns true when the point must be negated
DEVFN bool sign_normalise(fe& s) {
    bool gt = false, decided = false;
#pragma unroll
    for (int i = 7; i >= 0; i--) {
        const uint32_t lo = FrParams::mod(i) - (i == 0 ? 1u : 0u);
        const uint32_t hi = i < 7 ? FrParams::mod(i + 1) : 0u;
        const uint32_t h = (lo >> 1) | (hi << 31);
        if (!decided && s.l[i] != h) { gt = s.l[i] > h; decided = true; }
    }
    if (gt) {
        uint64_t br = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) { uint64_t d = (uint64_t)FrParams::mod(i) - s.l[i] - br; s.l[i] = (uint32_t)d; br = (d >> 32) & 1; }
    }
    return gt;
}

// One window of the signed c-bit recoding, s = sum_j e_j 2^(c j) with e_j in [-D, D-1], D = 2^(c-1): takes the low c bits of s plus the
// carry of the window below, shifts s down by c and returns the digit; carry_bit (0 or 1) goes in and comes out.  negated: s is the
// magnitude of a scalar whose point is negated — the returned digit is negated and the split threshold moves by one, so that it lies
// in [-D, D-1] all the same.  Callers that keep several carries packed in one register pass the bit in and out.
DEVFN int32_t signed_digit_step(fe& s, uint32_t c, uint32_t& carry_bit, bool negated) {
    const uint32_t cmask = (1u << c) - 1, D = 1u << (c - 1);
    const uint32_t raw = (s.l[0] & cmask) + carry_bit;
#pragma unroll
    for (int q = 0; q < 7; q++) {
#if defined(__HIP_DEVICE_COMPILE__)
        s.l[q] = __builtin_amdgcn_alignbit(s.l[q + 1], s.l[q], c);
#else
        s.l[q] = (uint32_t)((((uint64_t)s.l[q + 1] << 32) | s.l[q]) >> c);
#endif
    }
    s.l[7] >>= c;
    int32_t d = (int32_t)raw;
    if (raw >= D + (negated ? 1u : 0u)) { d -= (int32_t)(1u << c); carry_bit = 1; } else carry_bit = 0;
    if (negated) d = -d;
    return d;
}

// slot i (wave-uniform) of an octet: eight int16 in one 16-byte word, or (WIDE) eight int32 in two
template <bool WIDE> DEVFN int32_t octet_slot(const uint4& w0, const uint4& w1, uint32_t i) {
    if (WIDE) {
        const uint4& w = (i & 4) ? w1 : w0;
        return (int32_t)((i & 2) ? ((i & 1) ? w.w : w.z) : ((i & 1) ? w.y : w.x));
    }
    const uint64_t lo = (uint64_t)w0.x | ((uint64_t)w0.y << 32), hi = (uint64_t)w0.z | ((uint64_t)w0.w << 32);
    return (int32_t)(int16_t)(uint16_t)(((i & 4) ? hi : lo) >> (16 * (i & 3)));
}

// ---- table entries -----------------------------------------------------------------------------------------------------------------
template <class F> struct RawAff { fe w[2 * F::WORDS]; };
template <class F> DEVFN RawAff<F> load_raw(const fe* p) {
    RawAff<F> r;
#pragma unroll
    for (int i = 0; i < 2 * F::WORDS; i++) r.w[i] = load_fe(p + i);
    return r;
}
DEVFN Aff9<Fp29f> unpack_aff(const RawAff<Fp29f>& r, bool negate) {
    Aff9<Fp29f> e{Fp29::unpack(r.w[0]), Fp29::unpack(r.w[1])};
    if (negate) e.y = Fp29::neg(e.y);                      // signed-tight: fine as a product operand
    return e;
}
DEVFN Aff9<Fp2x> unpack_aff(const RawAff<Fp2x>& r, bool negate) {
    Aff9<Fp2x> e{fe9x2{Fp29::unpack(r.w[0]), Fp29::unpack(r.w[1])}, fe9x2{Fp29::unpack(r.w[2]), Fp29::unpack(r.w[3])}};
    if (negate) e.y = Fp2x::neg(e.y);
    return e;
}

// A flat value d that its row cannot serve (beyond the row's length, or MSM_FLAT_ESCAPE: the scalar scalars[rows[k] * batch + p] did
// not fit 15 bits and is read again here) multiplied out by double-and-add from the row's first entry: scalar * P_k.
template <class F>
DEVFN Xyzz9<F> mul_out(int32_t d, const fe* first_entry, const fe* scalars, const uint32_t* rows, size_t k, size_t batch, size_t p) {
    using C = Curve9<F>;
    fe sc = fe{}; bool sneg = d < 0;
    if (d == MSM_FLAT_ESCAPE) { sc = Fr::from_mont(load_fe(scalars + (size_t)rows[k] * batch + p)); sneg = sign_normalise(sc); }
    else sc.l[0] = (uint32_t)(d < 0 ? -d : d);
    const Aff9<F> P1 = unpack_aff(load_raw<F>(first_entry), sneg);
    Xyzz9<F> Q = C::infinity();
    for (int b = 253; b >= 0; b--) {
        if (!Q.inf) Q = C::dbl(Q);
        uint32_t word = sc.l[0];
#pragma unroll
        for (int q = 1; q < 8; q++) word = (b >> 5) == q ? sc.l[q] : word;
        if ((word >> (b & 31)) & 1u) Q = C::template madd<true>(Q, P1);
    }
    return Q;
}

// ---- slice geometry ----------------------------------------------------------------------------------------------------------------
// XCD-aware order: workgroups go round-robin over the 8 XCDs by linear id L and each XCD has its own L2.  Every wave of a slice
// (per_slice of them) gathers from the same table rows, so a slice is placed on ONE XCD (consecutive ids there).
struct SliceRem { size_t slice, rem; };
DEVFN SliceRem xcd_slice(size_t L, size_t nslices, size_t per_slice) {
    const size_t S8 = nslices & ~(size_t)7;
    if (L < S8 * per_slice) { const size_t xcd = L & 7, i = L >> 3; return SliceRem{(i / per_slice) * 8 + xcd, i % per_slice}; }
    return SliceRem{L / per_slice, L % per_slice};
}
// bases [k0, k1) of a slice of `per`
struct BaseRange { size_t k0, k1; };
DEVFN BaseRange slice_bounds(size_t slice, size_t per, size_t nbases) {
    const size_t k0 = slice * per < nbases ? slice * per : nbases;
    return BaseRange{k0, k0 + per < nbases ? k0 + per : nbases};
}

// ---- the sum of a point over the 64 lanes of a wave: a __shfl_xor butterfly of six exact additions; every lane gets the sum ----------
#if defined(__HIPCC__)
DEVFN fe9 shfl_xor_e(const fe9& v, int m) {
    fe9 r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = __shfl_xor(v.l[i], m);
    return r;
}
DEVFN fe9x2 shfl_xor_e(const fe9x2& v, int m) { return fe9x2{shfl_xor_e(v.a0, m), shfl_xor_e(v.a1, m)}; }
template <class F> DEVFN Xyzz9<F> wave_sum(Xyzz9<F> acc) {
    for (int m = 32; m >= 1; m >>= 1) {
        Xyzz9<F> o;
        o.x = shfl_xor_e(acc.x, m); o.y = shfl_xor_e(acc.y, m); o.zz = shfl_xor_e(acc.zz, m); o.zzz = shfl_xor_e(acc.zzz, m);
        o.inf = __shfl_xor((int)acc.inf, m) != 0;
        acc = Curve9<F>::add(acc, o);
    }
    return acc;
}
#endif

}  // namespace gsc
