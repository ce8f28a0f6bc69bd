// Host build of the lane-sliced verifier arithmetic (csrc/verify_few_dev.hpp compiled by g++ with the HIP headers, the lanes of a
// group walked in a loop by HostGroup): every group operation against the serial one of verify_dev.hpp, on seeded random values and
// on values at the edge of the value discipline; bilinearity through the lane-sliced final exponentiation; the Miller loop over
// precomputed lines against miller<> with its on-the-fly pair; pair_few against pair_one on a synthetic key (with and without a
// commitment).  tests/test_verify_few_host.py builds and runs it.
//   argv[1]: seed (default 1).  stdout: "ok <checks>" and exit status 0, or "FAIL <what>" lines and exit status 1.
#include "verify_few_dev.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

using namespace gsc::vfy;
namespace few = gsc::vfy::few;
using HG = few::HostGroup;
using HV = HG::V;

static int g_checks = 0, g_fail = 0;
static void check(bool ok, const char* what) { g_checks++; if (!ok) { g_fail++; printf("FAIL %s\n", what); } }

static std::mt19937_64 g_rng;
static e1 rand1() {
    for (;;) {
        uint8_t b[32];
        for (int i = 0; i < 32; i += 8) { const uint64_t v = g_rng(); memcpy(b + i, &v, 8); }
        e1 r;
        if (fp_from_be(b, true, r)) return r;
    }
}
static e2 rand2() { return e2{rand1(), rand1()}; }
static F12 rand12() { F12 r; for (int i = 0; i < 6; i++) r.c[i] = rand2(); return r; }
// every slice a sum of two reduced values (|value| < 4.02p, tight), with either sign: the largest operands a product may be handed
static F12 edge12(bool negative) {
    F12 r;
    for (int i = 0; i < 6; i++) {
        const e2 a = red2(rand2()), b = red2(rand2());
        r.c[i] = negative ? F2::norm(F2::sub(F2::neg(a), b)) : F2::norm(F2::add(a, b));
    }
    return r;
}
static bool same1(const e1& a, const e1& b) { const auto x = F::pack(F::from_mont(a)), y = F::pack(F::from_mont(b)); return memcmp(&x, &y, sizeof x) == 0; }
static bool same2(const e2& a, const e2& b) { return same1(a.a0, b.a0) && same1(a.a1, b.a1); }
static bool same12(const F12& a, const F12& b) { bool ok = true; for (int i = 0; i < 6; i++) ok = ok && same2(a.c[i], b.c[i]); return ok; }

static HV spread(const F12& a) { HV v; for (int k = 0; k < few::kGroup; k++) v.v[k] = k < few::kSlices ? a.c[k] : F2::zero(); return v; }
static F12 gather(const HV& v) { F12 a; for (int k = 0; k < 6; k++) a.c[k] = v.v[k]; return a; }
static bool pads_zero(const HV& v) { return zero2(v.v[6]) && zero2(v.v[7]); }

// ---- points ----
static e1 dec1(const char* s) {      // decimal -> Montgomery limbs
    uint8_t b[32] = {0};
    for (; *s; s++) { int c = *s - '0'; for (int i = 31; i >= 0; i--) { c += b[i] * 10; b[i] = (uint8_t)c; c >>= 8; } }
    e1 r; if (!fp_from_be(b, false, r)) abort();
    return r;
}
static VP1 g1_gen() { VP1 p; p.x = dec1("1"); p.y = dec1("2"); p.inf = 0; return p; }
static VP2 g2_gen() {
    VP2 q; q.inf = 0;
    q.x = e2{dec1("10857046999023057135944570762232829481370756359578518086990519993285655852781"), dec1("11559732032986387107991004021392285783925812861821192530917403151452391805634")};
    q.y = e2{dec1("8495653923123431417604973247489272438418190587263600148770280649306958101930"), dec1("4082367875863433681332203403145435568316851327593401208105741076214120093531")};
    return q;
}
static VP1 inf1() { VP1 p; p.x = p.y = F::zero(); p.inf = 1; return p; }
static VP2 inf2() { VP2 q; q.x = q.y = F2::zero(); q.inf = 1; return q; }
static VP1 mul1k(const VP1& p, uint64_t k) {
    G1X acc = g1_inf();
    for (int i = 63; i >= 0; i--) { acc = bn254::G1x::dbl(acc); if ((k >> i) & 1) acc = g1_madd(acc, p); }
    return g1_affine(acc);
}
static VP2 mul2k(const VP2& q, uint64_t k) {
    using G = bn254::G2x;
    if (q.inf || !k) return inf2();
    const bn254::Aff9<F2> qa{q.x, q.y};
    auto acc = G::infinity();
    for (int i = 63; i >= 0; i--) { acc = G::dbl(acc); if ((k >> i) & 1) acc = G::madd<true>(acc, qa); }
    if (acc.inf || F2::is_zero(acc.zz)) return inf2();
    const auto a = G::to_aff(acc);
    VP2 r; r.x = red2(a.x); r.y = red2(a.y); r.inf = 0;
    return r;
}

int main(int argc, char** argv) {
    g_rng.seed(argc > 1 ? strtoull(argv[1], nullptr, 10) : 1);
    std::vector<e2> slots(few::kSlots * few::kGroup);
    const HG g{slots.data()};

    // ---- every group operation against the serial one ----
    for (int round = 0; round < 12; round++) {
        const bool edge = round >= 6;
        const F12 a = edge ? edge12(round & 1) : rand12(), b = edge ? edge12(round & 2) : rand12();
        const e2 c0 = red2(rand2()), c1 = red2(rand2()), c3 = red2(rand2());
        const HV va = spread(a), vb = spread(b);
        HV r;
        r = few::mul12(g, va, vb); check(same12(gather(r), mul12(a, b)) && pads_zero(r), "mul12");
        r = few::sqr12(g, va); check(same12(gather(r), sqr12(a)) && pads_zero(r), "sqr12");
        check(same12(gather(r), mul12(a, a)), "sqr12 vs mul12");
        r = few::mul_line(g, va, c0, c1, c3); check(same12(gather(r), mul_line(a, c0, c1, c3)) && pads_zero(r), "mul_line");
        r = few::conj12(g, va); check(same12(gather(r), conj12(a)) && pads_zero(r), "conj12");
        r = few::frob12(g, va); check(same12(gather(r), frob12(a)) && pads_zero(r), "frob12");
        r = few::frob12_2(g, va); check(same12(gather(r), frob12_2(a)) && pads_zero(r), "frob12_2");
        // the serial inverse, power and final exponentiation take reduced values (they follow a product in every caller)
        const F12 ar = mul12(a, one12());
        const HV var = spread(ar);
        r = few::inv12(g, var); check(same12(gather(r), inv12(ar)) && pads_zero(r), "inv12");
        check(few::is_one12(g, few::mul12(g, r, var)), "inv12 * a == 1");
        if (round % 3 == 0) {
            r = few::pow_x(g, var); check(same12(gather(r), pow_x(ar)) && pads_zero(r), "pow_x");
            r = few::final_exp(g, var); check(same12(gather(r), final_exp(ar)) && pads_zero(r), "final_exp");
            check(!few::is_one12(g, r), "final_exp of a random value is not one");
        }
    }
    check(few::is_one12(g, few::one12(g)) && is_one12(gather(few::one12(g))), "one12");
    { F12 o = one12(); o.c[4].a1 = F::one(); check(!few::is_one12(g, spread(o)), "is_one12 sees slice 4"); }

    // ---- Miller loop over lines_of against miller<> ----
    const VP1 P = g1_gen(); const VP2 Q = g2_gen();
    const uint64_t a = 1 + (g_rng() >> 8), b = 1 + (g_rng() >> 8);
    const VP1 aP = mul1k(P, a); const VP2 bQ = mul2k(Q, b);
    std::vector<Line> lv(kLineSteps), lf[3];
    const VP1 none_p[3] = {inf1(), inf1(), inf1()}; const Line* none_l[3] = {nullptr, nullptr, nullptr}; const bool none_inf[3] = {true, true, true};
    const few::Stream off = few::no_stream();
    {
        lines_of(bQ, lv.data());
        const F12 want = miller<3>(aP, bQ, true, none_p, none_l, none_inf);
        const HV got = few::miller_few(g, few::stream(&aP, lv.data(), false, false, true), off, off, off, 1);
        check(same12(gather(got), want) && pads_zero(got), "miller over lines_of(Q)");
        // P or Q at infinity: the pair is skipped
        const VP1 pi = inf1(); const VP2 qi = inf2();
        std::vector<Line> zero(kLineSteps);
        memset((void*)zero.data(), 0, zero.size() * sizeof(Line));
        check(same12(gather(few::miller_few(g, few::stream(&pi, lv.data(), false, false, true), off, off, off, 1)), miller<3>(pi, bQ, true, none_p, none_l, none_inf)), "miller, P infinity");
        check(same12(gather(few::miller_few(g, few::stream(&aP, zero.data(), false, true, true), off, off, off, 1)), miller<3>(aP, qi, true, none_p, none_l, none_inf)), "miller, Q infinity");
        check(is_one12(gather(few::miller_few(g, few::stream(&pi, zero.data(), false, true, true), off, off, off, 1))), "miller, both infinity");
        // four streams, the fixed ones negated, against miller<3> with the same fixed lines
        VP1 fp[3]; VP2 fq[3]; const Line* fl[3]; const bool finf[3] = {false, false, false};
        for (int t = 0; t < 3; t++) { fp[t] = mul1k(P, 3 + 5 * t + (g_rng() & 0xFFFF)); fq[t] = mul2k(Q, 7 + t + (g_rng() & 0xFFFF)); lf[t].resize(kLineSteps); lines_of(fq[t], lf[t].data()); fl[t] = lf[t].data(); }
        const VP1 np[3] = {neg_p(fp[0]), neg_p(fp[1]), neg_p(fp[2])};
        const F12 want4 = miller<3>(aP, bQ, true, np, fl, finf);
        const HV got4 = few::miller_few(g, few::stream(&aP, lv.data(), false, false, true), few::stream(&fp[0], fl[0], true, false, true),
                                        few::stream(&fp[1], fl[1], true, false, true), few::stream(&fp[2], fl[2], true, false, true), 4);
        check(same12(gather(got4), want4), "miller, four streams");
    }
    // ---- e(aP, bQ) e(-abP, Q) == 1 through the lane-sliced final exponentiation ----
    {
        const uint64_t sa = 1 + (g_rng() & 0xFFFFFFF), sb = 1 + (g_rng() & 0xFFFFFFF);
        const VP1 p1 = mul1k(P, sa), p2 = mul1k(P, sa * sb); const VP2 q1 = mul2k(Q, sb);
        std::vector<Line> l1(kLineSteps), l2(kLineSteps);
        lines_of(q1, l1.data()); lines_of(Q, l2.data());
        const HV f = few::miller_few(g, few::stream(&p1, l1.data(), false, false, true), few::stream(&p2, l2.data(), true, false, true), off, off, 2);
        check(few::is_one12(g, few::final_exp(g, f)), "e(aP, bQ) e(-abP, Q) == 1");
        const VP1 p3 = mul1k(P, sa * sb + 1);
        const HV f2 = few::miller_few(g, few::stream(&p1, l1.data(), false, false, true), few::stream(&p3, l2.data(), true, false, true), off, off, 2);
        check(!few::is_one12(g, few::final_exp(g, f2)), "e(aP, bQ) e(-(ab + 1)P, Q) != 1");
    }
    // ---- pair_few against pair_one: A = 7P, B = 11Q, alpha = 2P, beta = 3Q, L = 5P, gamma = 7Q, C = 4P, delta = 9Q (77 = 6 + 35 + 36);
    //      commitment: D = 3P, ped_gsn = 5Q, PoK = -15P, ped_g = Q ----
    for (int hc = 0; hc < 2; hc++) {
        KeyDev k{};
        k.fits = 1; k.has_commitment = hc; k.alpha = mul1k(P, 2);
        const VP2 kq[5] = {mul2k(Q, 3), mul2k(Q, 7), mul2k(Q, 9), Q, mul2k(Q, 5)};
        std::vector<Line> kl(5 * kLineSteps);
        memset((void*)kl.data(), 0, kl.size() * sizeof(Line));
        for (int t = 0; t < 5; t++) { k.qinf[t] = (t >= 3 && !hc) ? 1 : 0; k.lines[t] = &kl[t * kLineSteps]; if (!k.qinf[t]) lines_of(kq[t], &kl[t * kLineSteps]); }
        for (int bad = 0; bad < (hc ? 5 : 3); bad++) {
            ProofDev p{};
            p.ok = 1; p.A = mul1k(P, 7); p.B = mul2k(Q, 11); p.L = mul1k(P, 5); p.C = mul1k(P, bad == 1 ? 5 : 4);
            p.D = bad == 4 ? inf1() : mul1k(P, 3); p.pok = neg_p(mul1k(P, bad == 3 ? 16 : 15));
            if (bad == 2) p.A = inf1();
            std::vector<Line> pl(kLineSteps);
            memset((void*)pl.data(), 0, pl.size() * sizeof(Line));
            if (!p.A.inf && !p.B.inf) lines_of(p.B, pl.data());
            F12 f_serial = one12(), f_few = one12();
            const bool want = pair_one(k, p, &f_serial), got = few::pair_few(g, k, &p, pl.data(), true, &f_few);
            check(want == got && want == (bad == 0), "pair_few verdict");
            if (want || !hc) check(same12(f_serial, f_few), "pair_few reduced value");
        }
        check(!few::pair_few(g, k, (const ProofDev*)nullptr, (const Line*)nullptr, false, (F12*)nullptr), "pair_few without a proof");
    }
    if (g_fail) return 1;
    printf("ok %d\n", g_checks);
    return 0;
}
