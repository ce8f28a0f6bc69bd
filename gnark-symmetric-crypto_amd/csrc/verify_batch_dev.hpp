// Per-thread code of the batched Groth16 check (k_verify_batch.hip, gsc_verify_raw_batched / gsc_verify_all): with independent
// random 128-bit rho_i (and t_i for the Pedersen proof of knowledge of AES keys) a chunk is accepted iff
//   prod_i e(rho_i A_i, B_i) e(-(sum rho_i) alpha, beta) e(-sum rho_i L_i, gamma) e(-sum rho_i C_i, delta)
//   [ e(sum t_i D_i, ped_gsn) e(sum t_i PoK_i, ped_g) ] == 1,
// which fails with probability about 2^-128 when some proof would fail on its own.  Each proof pays one Miller loop over its own
// pair and a few G1 scalar multiplications; the key-side pairs and the final exponentiation are paid once per chunk.
// Like verify_dev.hpp, everything here is plain per-thread code that also compiles for the host (tests/native/verify_batch_check.cpp).
#pragma once
#include "verify_dev.hpp"

namespace gsc {
namespace vfy {

constexpr int kBatchSums = 4;        // per chunk: sum rho L, sum rho C, sum t D, sum t PoK
constexpr int kBatchFixed = 5;       // fixed pairs, in KeyDev::lines order: beta, gamma, delta, ped_g, ped_gsn
constexpr int kRandWords = 8;        // per proof: rho (4 little-endian words), t (4 words; AES keys only)

// k P over the low nbits of k (little-endian words); exact XYZZ double-and-add
DEVFN G1X g1_mul(const VP1& p, const uint32_t* k, int nbits) {
    G1X acc = g1_inf();
    if (p.inf) return acc;
    const bn254::Aff9<bn254::Fp29f> a{p.x, p.y};
    for (int i = nbits - 1; i >= 0; i--) {
        acc = bn254::G1x::dbl(acc);
        if ((k[i >> 5] >> (i & 31)) & 1) acc = bn254::G1x::madd<true>(acc, a);
    }
    return acc;
}
DEVFN G1X g1_add(const G1X& a, const G1X& b) { return bn254::G1x::add(a, b); }
DEVFN VP1 vp1_inf() { VP1 r; r.x = F::zero(); r.y = F::zero(); r.inf = 1; return r; }

// proof p's term of sum j (0: rho L, 1: rho C, 2: t D, 3: t PoK); the caller skips proofs without ok
DEVFN G1X batch_term(const ProofDev& p, int j, const uint32_t* rnd) {
    const VP1& q = j == 0 ? p.L : j == 1 ? p.C : j == 2 ? p.D : p.pok;
    return g1_mul(q, rnd + (j < 2 ? 0 : 4), 128);
}
// rho A in affine coordinates (the Miller loop's line evaluation takes affine P)
DEVFN VP1 batch_scaled_a(const ProofDev& p, const uint32_t* rnd) { return g1_affine(g1_mul(p.A, rnd, 128)); }

// sum rho_i from per-word column sums (word c of every rho added up: at most 65 536 x 2^32 < 2^48 each) -> 160-bit little-endian
DEVFN void rho_sum_words(const uint64_t (&col)[4], uint32_t (&out)[5]) {
    uint64_t c = 0;
    for (int w = 0; w < 4; w++) { c += col[w]; out[w] = (uint32_t)c; c >>= 32; }
    out[4] = (uint32_t)c;
}
// the G1 points of the fixed pairs, kBatchFixed of them: -(sum rho) alpha, -sum rho L, -sum rho C, sum t PoK, sum t D
// (sums: kBatchSums totals in batch_term order; infinity for the Pedersen pairs of a key without a commitment)
DEVFN VP1 batch_fixed_point(const KeyDev& k, int j, const G1X (&sums)[kBatchSums], const uint32_t (&rho_sum)[5]) {
    if (j == 0) return neg_p(g1_affine(g1_mul(k.alpha, rho_sum, 160)));
    if (j == 1 || j == 2) return neg_p(g1_affine(sums[j - 1]));
    if (!k.has_commitment) return vp1_inf();
    return g1_affine(sums[j == 3 ? 3 : 2]);
}

// one pair's Miller loop before the final exponentiation; lines from T = Q on the fly (lines == nullptr) or precomputed (kLineSteps
// of a key's fixed point; q is then unused).  1 when P is infinity or q_inf.  Same walk as miller<> in verify_dev.hpp.
DEVFN F12 miller_one(const VP1& p, const VP2& q, bool q_inf, const Line* lines) {
    F12 f = one12();
    if (p.inf || q_inf) return f;
    G2J T{q.x, q.y, F2::one()};
    int s = 0;
    for (int i = kLoopSteps - 1; i >= -2; i--) {
        const int nsub = (i >= 0) ? (1 + (int)((loop_bits() >> i) & 1)) : 1;
        if (i >= 0) f = sqr12(f);
        for (int sub = 0; sub < nsub; sub++, s++) {
            Line l;
            if (lines) l = lines[s];
            else if (i >= 0 && sub == 0) l = dbl_step(T);
            else if (i >= 0) l = add_step(T, q.x, q.y);
            else {
                e2 q1x, q1y, q2x, q2y; frob_points(q, q1x, q1y, q2x, q2y);
                l = (i == -1) ? add_step(T, q1x, q1y) : add_step(T, q2x, q2y);
            }
            f = apply_line(f, l, p);
        }
    }
    return f;
}
// f_i of proof p: e(rho A, B) unreduced; 1 for a proof without ok
DEVFN F12 batch_miller_proof(const ProofDev& p, const VP1& ra) { return p.ok ? miller_one(ra, p.B, p.B.inf != 0, nullptr) : one12(); }
// the fixed pair j (point from batch_fixed_point) against the key's precomputed lines
DEVFN F12 batch_miller_fixed(const KeyDev& k, int j, const VP1& pt) { VP2 none; none.x = none.y = F2::zero(); none.inf = 1; return miller_one(pt, none, k.qinf[j] != 0, k.lines[j]); }
// the chunk's verdict from the product of every f_i and fixed-pair value
DEVFN bool batch_accept(const F12& prod) { return is_one12(final_exp(prod)); }

}  // namespace vfy
}  // namespace gsc
