// Lane-sliced Fp12 arithmetic for the few-proof verifier kernels (k_verify_few.hip): a group of kGroup = 8 consecutive lanes of one
// wave verifies one proof.  Lanes 0..5 of the group hold the coefficients c[0..5] of every Fp12 value (one Fp2 each); lanes 6 and 7
// ride along on zero.  An operation publishes its operands in the group's exchange slots, then lane k evaluates the formula of its
// own output coefficient k from verify_dev.hpp: the six iterations of the serial outer loops run side by side, and no lane ever
// holds a whole Fp12 (inv12, once per proof, is the exception: lane 0 gathers the value and runs the serial function).
//
// The group is a type G handed to every function:
//   G::V                      what one value is: the lane's Fp2 slice on the device, all kGroup slices on the host
//   g.open() / g.close()      before the first and after the last put of an exchange (barriers on the device)
//   g.put(s, a)               publish a in exchange slot s (every lane its own slice)
//   g.view(s)                 the kGroup slices of slot s, indexed by lane
//   g.each(fn)                the value whose slice k is fn(k); g.own(a, k) is slice k of a inside fn
//   g.all(fn)                 fn(k) holds on every slice lane
//   g.pick(c, a, b)           c ? a : b for a group-uniform c
//   g.lane0(fn)               run fn once per group (after close(): it may read views and write slot 0)
// WaveGroup (device) keeps the slots in LDS; HostGroup walks the lanes in a loop, which is how tests/native/verify_few_check.cpp
// checks every operation against the serial code without a GPU.  Nothing in here returns early in front of an exchange: a group
// without a proof computes on the identity.
//
// Value discipline as in verify_dev.hpp: slices are reduced (|value| < 2.01p) between operations.
#pragma once
#include "verify_dev.hpp"

namespace gsc {
namespace vfy {
namespace few {

constexpr int kGroup = 8;          // lanes per proof
constexpr int kSlices = 6;         // of which hold a coefficient
constexpr int kSlots = 2;          // exchange slots per group (two operands)
constexpr int kGroupsPerWave = 64 / kGroup;

DEVFN e1 sel1(bool c, const e1& a, const e1& b) { e1 r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = c ? a.l[i] : b.l[i];
    return r; }
DEVFN e2 sel2(bool c, const e2& a, const e2& b) { return e2{sel1(c, a.a0, b.a0), sel1(c, a.a1, b.a1)}; }

// ---- the groups ----
struct HostGroup {
    struct V { e2 v[kGroup]; };
    e2* slots;                        // kSlots x kGroup
    void open() const {}
    void close() const {}
    void put(int s, const V& a) const { for (int k = 0; k < kGroup; k++) slots[kGroup * s + k] = a.v[k]; }
    const e2* view(int s) const { return slots + kGroup * s; }
    e2* wview(int s) const { return slots + kGroup * s; }
    static const e2& own(const V& a, int k) { return a.v[k]; }
    template <class Fn> V each(Fn fn) const { V r; for (int k = 0; k < kGroup; k++) r.v[k] = k < kSlices ? fn(k) : F2::zero(); return r; }
    template <class Fn> bool all(Fn fn) const { bool ok = true; for (int k = 0; k < kSlices; k++) ok = fn(k) && ok; return ok; }
    template <class Fn> void lanes(Fn fn) const { for (int k = 0; k < kSlices; k++) fn(k); }
    template <class Fn> void lane0(Fn fn) const { fn(); }
    static V pick(bool c, const V& a, const V& b) { return c ? a : b; }
};

#ifdef __HIPCC__
// one wave per block: __syncthreads() is the wave's own barrier and orders the LDS traffic of an exchange
struct WaveGroup {
    using V = e2;
    e2* slots;                        // this group's kSlots x kGroup slices in LDS
    int k;                            // lane within the group
    DEVFN void open() const { __syncthreads(); }
    DEVFN void close() const { __syncthreads(); }
    DEVFN void put(int s, const V& a) const { slots[kGroup * s + k] = a; }
    DEVFN const e2* view(int s) const { return slots + kGroup * s; }
    DEVFN e2* wview(int s) const { return slots + kGroup * s; }
    DEVFN static const e2& own(const V& a, int) { return a; }
    template <class Fn> DEVFN V each(Fn fn) const { const V r = fn(k < kSlices ? k : 0); return sel2(k < kSlices, r, F2::zero()); }
    template <class Fn> DEVFN bool all(Fn fn) const {
        const bool mine = k >= kSlices || fn(k);
        const unsigned long long b = __ballot(mine);
        return ((b >> (8 * ((threadIdx.x & 63) / kGroup))) & 0xFFull) == 0xFFull;
    }
    template <class Fn> DEVFN void lanes(Fn fn) const { if (k < kSlices) fn(k); }
    template <class Fn> DEVFN void lane0(Fn fn) const { if (k == 0) fn(); }
    DEVFN static V pick(bool c, const V& a, const V& b) { return sel2(c, a, b); }
};
constexpr int kWaveLds = kGroupsPerWave * kSlots * kGroup;      // Fp2 slices of exchange slots per block (one wave)
// the calling lane's group of a one-wave block whose kWaveLds slices of LDS are lds
__device__ __forceinline__ WaveGroup wave_group(e2* lds) {
    const int t = threadIdx.x;
    return WaveGroup{lds + (t / kGroup) * (kSlots * kGroup), t % kGroup};
}
#endif

// ---- what lane k computes (operands: the six published coefficients) ----
// coefficient k of a b: the products a_i b_j with i + j = k (low) and i + j = k + 6 (high, times xi), one per trip for every k
DEVFN e2 mul12_lane(int k, const e2* a, const e2* b) {
    e2 lo = F2::zero(), hi = F2::zero();
#pragma unroll 1
    for (int i = 0; i < 6; i++) {
        const bool low = i <= k;
        const e2 m = mul2(a[i], b[low ? k - i : k + 6 - i]);
        lo = sel2(low, acc2(lo, m), lo);
        hi = sel2(low, hi, acc2(hi, m));
    }
    return red2(F2::add(red2(lo), mulxi(red2(hi))));
}
// the unordered pairs {i, j} of coefficient k of a^2, four 7-bit entries i | j << 3 | 64 (0: none); cross products take the doubled
// operand d = 2a as sqr12 does
DEVFN constexpr uint32_t sqr_pair(int i, int j) { return (uint32_t)(i | j << 3 | 64); }
DEVFN constexpr uint32_t sqr_pairs4(uint32_t p0, uint32_t p1, uint32_t p2, uint32_t p3) { return p0 | p1 << 7 | p2 << 14 | p3 << 21; }
DEVFN uint32_t sqr_pairs(int k) {
    constexpr uint32_t t0 = sqr_pairs4(sqr_pair(0, 0), sqr_pair(1, 5), sqr_pair(2, 4), sqr_pair(3, 3));
    constexpr uint32_t t1 = sqr_pairs4(sqr_pair(0, 1), sqr_pair(2, 5), sqr_pair(3, 4), 0);
    constexpr uint32_t t2 = sqr_pairs4(sqr_pair(0, 2), sqr_pair(1, 1), sqr_pair(3, 5), sqr_pair(4, 4));
    constexpr uint32_t t3 = sqr_pairs4(sqr_pair(0, 3), sqr_pair(1, 2), sqr_pair(4, 5), 0);
    constexpr uint32_t t4 = sqr_pairs4(sqr_pair(0, 4), sqr_pair(1, 3), sqr_pair(2, 2), sqr_pair(5, 5));
    constexpr uint32_t t5 = sqr_pairs4(sqr_pair(0, 5), sqr_pair(1, 4), sqr_pair(2, 3), 0);
    return k == 0 ? t0 : k == 1 ? t1 : k == 2 ? t2 : k == 3 ? t3 : k == 4 ? t4 : t5;
}
DEVFN e2 sqr12_lane(int k, const e2* a, const e2* d) {
    const uint32_t pairs = sqr_pairs(k);
    e2 lo = F2::zero(), hi = F2::zero();
#pragma unroll 1
    for (int t = 0; t < 4; t++) {
        const uint32_t e = (pairs >> (7 * t)) & 127;
        const int i = (int)(e & 7), j = (int)((e >> 3) & 7);
        const bool on = (e & 64) != 0, low = i + j < 6;
        const e2* x = (i == j) ? a + i : d + i;
        const e2 m = mul2(*x, a[j]);
        lo = sel2(on && low, acc2(lo, m), lo);
        hi = sel2(on && !low, acc2(hi, m), hi);
    }
    return red2(F2::add(red2(lo), mulxi(red2(hi))));
}
// coefficient k of f (c0 + c1 w + c3 w^3): f_k c0 + f_(k-1) c1 + f_(k-3) c3, indices below zero wrapping to xi f_(. + 6) (xf = xi f)
DEVFN e2 mul_line_lane(int k, const e2* f, const e2* xf, const e2& c0, const e2& c1, const e2& c3) {
    const e2* t1 = (k >= 1) ? f + (k - 1) : xf + 5;
    const e2* t3 = (k >= 3) ? f + (k - 3) : xf + (k + 3);
    return red2(acc2(acc2(mul2(f[k], c0), mul2(*t1, c1)), mul2(*t3, c3)));
}

// ---- Fp12 operations of the group ----
template <class G> DEVFN typename G::V one12(const G& g) { return g.each([&](int k) { return k == 0 ? F2::one() : F2::zero(); }); }
template <class G> DEVFN typename G::V load12(const G& g, const F12* p) { return g.each([&](int k) { return p->c[k]; }); }
template <class G> DEVFN void store12(const G& g, const typename G::V& a, F12* p) { g.lanes([&](int k) { p->c[k] = G::own(a, k); }); }

template <class G> DEVNOINL typename G::V mul12(G g, const typename G::V& a, const typename G::V& b) {
    g.open(); g.put(0, a); g.put(1, b); g.close();
    return g.each([&](int k) { return mul12_lane(k, g.view(0), g.view(1)); });
}
template <class G> DEVNOINL typename G::V sqr12(G g, const typename G::V& a) {
    const typename G::V d = g.each([&](int k) { return small2(G::own(a, k), 2); });
    g.open(); g.put(0, a); g.put(1, d); g.close();
    return g.each([&](int k) { return sqr12_lane(k, g.view(0), g.view(1)); });
}
template <class G> DEVNOINL typename G::V mul_line(G g, const typename G::V& f, const e2& c0, const e2& c1, const e2& c3) {
    const typename G::V xf = g.each([&](int k) { return mulxi(G::own(f, k)); });
    g.open(); g.put(0, f); g.put(1, xf); g.close();
    return g.each([&](int k) { return mul_line_lane(k, g.view(0), g.view(1), c0, c1, c3); });
}
template <class G> DEVFN typename G::V conj12(const G& g, const typename G::V& a) {
    return g.each([&](int k) { const e2& v = G::own(a, k); return sel2((k & 1) != 0, neg2(v), v); });
}
template <class G> DEVNOINL typename G::V frob12(G g, const typename G::V& a) {
    return g.each([&](int k) { const e2 c = conj2(G::own(a, k)); return sel2(k == 0, c, mul2(c, frob1(k == 0 ? 1 : k))); });
}
template <class G> DEVNOINL typename G::V frob12_2(G g, const typename G::V& a) {
    return g.each([&](int k) { const e2& v = G::own(a, k); return sel2(k == 0, v, scale2(v, frob2c(k == 0 ? 1 : k))); });
}
// once per proof: lane 0 gathers the value, runs the serial inv12 and hands the coefficients back through slot 0
template <class G> DEVNOINL typename G::V inv12(G g, const typename G::V& a) {
    g.open(); g.put(0, a); g.close();
    g.lane0([&]() {
        F12 x;
        for (int j = 0; j < 6; j++) x.c[j] = g.view(0)[j];
        const F12 r = vfy::inv12(x);
        for (int j = 0; j < 6; j++) g.wview(0)[j] = r.c[j];
    });
    g.close();
    return g.each([&](int k) { return g.view(0)[k]; });
}
template <class G> DEVFN bool is_one12(const G& g, const typename G::V& a) {
    return g.all([&](int k) { const e2& v = G::own(a, k); return k == 0 ? (eq1(v.a0, F::one()) && zero1(v.a1)) : zero2(v); });
}
template <class G> DEVNOINL typename G::V pow_x(G g, const typename G::V& a) {
    typename G::V acc = a;
    for (int i = 61; i >= 0; i--) {
        acc = sqr12(g, acc);
        if ((kX >> i) & 1) acc = mul12(g, acc, a);
    }
    return acc;
}
// verify_dev.hpp's final_exp, operation for operation
template <class G> DEVNOINL typename G::V final_exp(G g, const typename G::V& f) {
    using V = typename G::V;
    const V e1v = mul12(g, conj12(g, f), inv12(g, f));
    const V gg = mul12(g, frob12_2(g, e1v), e1v);
    V fx = gg, fx2 = gg, fx3 = gg, cur = gg;
    for (int k = 0; k < 3; k++) {
        cur = pow_x(g, cur);
        if (k == 0) fx = cur; else if (k == 1) fx2 = cur; else fx3 = cur;
    }
    const V fp2 = frob12_2(g, gg);
    const V y0 = mul12(g, mul12(g, frob12(g, gg), fp2), frob12(g, fp2));
    const V y1 = conj12(g, gg);
    const V y2 = frob12_2(g, fx2);
    const V y3 = conj12(g, frob12(g, fx));
    const V y4 = conj12(g, mul12(g, fx, frob12(g, fx2)));
    const V y5 = conj12(g, fx2);
    const V y6 = conj12(g, mul12(g, fx3, frob12(g, fx3)));
    V t0 = mul12(g, mul12(g, sqr12(g, y6), y4), y5);
    V t1 = mul12(g, mul12(g, y3, y5), t0);
    t0 = mul12(g, t0, y2);
    t1 = sqr12(g, mul12(g, sqr12(g, t1), t0));
    t0 = mul12(g, t1, y1);
    t1 = mul12(g, t1, y0);
    return mul12(g, sqr12(g, t0), t1);
}

// ---- Miller loop over precomputed lines ----
// one pair: the G1 point (in memory; negated when neg), kLineSteps lines of its G2 point, and whether the pair takes part (both points
// finite).  A pair that does not is walked on zero lines and its products are dropped: every group of a wave makes the same exchanges.
struct Stream { const VP1* p; const Line* lines; bool neg, on; };
DEVFN Stream stream(const VP1* p, const Line* lines, bool neg, bool q_inf, bool live) { return Stream{p, lines, neg, live && !q_inf && !p->inf}; }
DEVFN Stream no_stream() { return Stream{nullptr, nullptr, false, false}; }

template <class G> DEVFN typename G::V apply_stream(G g, const typename G::V& f, const Stream& st, int s) {
    e2 c0 = F2::zero(), c1 = F2::zero(), c3 = F2::zero();
    if (st.on) {
        const Line& l = st.lines[s];
        const e1 y = st.neg ? neg1(st.p->y) : st.p->y;
        c0 = scale2(l.a, y); c1 = scale2(l.b, st.p->x); c3 = l.c;
    }
    return G::pick(st.on, mul_line(g, f, c0, c1, c3), f);
}
// prod_t e(P_t, Q_t) before the final exponentiation over the first ns of four streams (ns the same for every group of the launch);
// the walk of miller<> in verify_dev.hpp with every pair on precomputed lines
template <class G> DEVNOINL typename G::V miller_few(G g, const Stream& s0, const Stream& s1, const Stream& s2, const Stream& s3, int ns) {
    typename G::V f = one12(g);
    int s = 0;
    for (int i = kLoopSteps - 1; i >= -2; i--) {
        const int nsub = (i >= 0) ? (1 + (int)((loop_bits() >> i) & 1)) : 1;
        if (i >= 0) f = sqr12(g, f);
        for (int sub = 0; sub < nsub; sub++, s++) {
            f = apply_stream(g, f, s0, s);
            if (ns > 1) f = apply_stream(g, f, s1, s);
            if (ns > 2) f = apply_stream(g, f, s2, s);
            if (ns > 3) f = apply_stream(g, f, s3, s);
        }
    }
    return f;
}

// ---- one proof per group ----
// pair_one of verify_dev.hpp: p is the group's ProofDev and var_lines the kLineSteps lines of its B (k_verify_few_lines; not read when
// A or B is infinity); live == false (no proof in this group, or prep refused it) runs on the identity and yields false.  Both passes
// of a key with a commitment always run.  f_out (optional): pass 1's reduced value.
template <class G> DEVFN bool pair_few(G g, const KeyDev& k, const ProofDev* p, const Line* var_lines, bool live, F12* f_out) {
    bool ok = live && k.fits;
    for (int pass = k.has_commitment ? 0 : 1; pass < 2; pass++) {
        Stream s0, s1, s2 = no_stream(), s3 = no_stream();
        if (pass == 0) {
            s0 = live ? stream(&p->D, k.lines[4], false, k.qinf[4] != 0, true) : no_stream();
            s1 = live ? stream(&p->pok, k.lines[3], false, k.qinf[3] != 0, true) : no_stream();
        } else {
            s0 = live ? stream(&p->A, var_lines, false, p->B.inf != 0, true) : no_stream();
            s1 = stream(&k.alpha, k.lines[0], true, k.qinf[0] != 0, live);
            s2 = live ? stream(&p->L, k.lines[1], true, k.qinf[1] != 0, true) : no_stream();
            s3 = live ? stream(&p->C, k.lines[2], true, k.qinf[2] != 0, true) : no_stream();
        }
        const typename G::V f = final_exp(g, miller_few(g, s0, s1, s2, s3, pass == 0 ? 2 : 4));
        if (pass == 1 && f_out && live) store12(g, f, f_out);
        ok = is_one12(g, f) && ok;
    }
    return ok;
}

}  // namespace few
}  // namespace vfy
}  // namespace gsc
