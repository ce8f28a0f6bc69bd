// Per-thread and per-group code of the claim-wise batched check (k_verify_claims.hip, gsc_verify_claims / VerifyClaims): the equation of
// verify_batch_dev.hpp, one per part instead of one per chunk.  A part is a contiguous run of a chunk's proofs (a claim, or the piece
// of a claim that lies in this chunk); it has its own sums, its own fixed points, its own product and its own final exponentiation,
// so no part's verdict depends on a proof outside it.  The steps, in launch order:
//   scale    per proof: rho A (affine) and the proof's own terms rho L, rho C (AES: t D, t PoK); nothing is summed here
//   sums     per part, lanes striding over its proofs: the totals of the terms and of rho; then the part's fixed points
//   miller   per proof as in the batched check; per (part, fixed pair) against the key's lines, or per part as three streams of
//            few::miller_few over one f (beta, gamma, delta; for a key with a commitment a second group: ped_g, ped_gsn)
//   product  per part, lanes striding over its Miller values
//   final    per part, one 8-lane group: few::final_exp, is_one12
// Like verify_batch_dev.hpp and verify_few_dev.hpp this compiles for the host too (tests/native/verify_claims_check.cpp walks the
// lanes in loops).
#pragma once
#include "verify_batch_dev.hpp"
#include "verify_few_dev.hpp"

namespace gsc {
namespace vfy {
namespace claims {

struct Part { uint32_t begin, end; };      // proofs [begin, end) of the chunk, begin < end
constexpr int kLanes = 64;                 // lanes that stride over one part (one wave)
constexpr int kFewStreams = 3;             // fixed pairs one 8-lane group walks over a shared f
// Miller values of a part's fixed pairs: one per pair from single threads, one per group of kFewStreams from the 8-lane groups
constexpr int fixed_pairs(bool has_commitment) { return has_commitment ? kBatchFixed : 3; }
constexpr int fixed_groups(bool has_commitment) { return has_commitment ? 2 : 1; }

// lanes that hold a value when `count` values are spread over kLanes, rounded up to a power of two: the width of the tree above them
DEVFN int tree_width(uint32_t count) {
    int w = 1;
    while (w < kLanes && (uint32_t)w < count) w <<= 1;
    return w;
}

// scale: terms[j] for j < nsums (batch_term's order); a proof without ok contributes the neutral element everywhere
DEVFN void scale_one(const ProofDev& p, const uint32_t* rnd, int nsums, VP1& ra, G1X* terms) {
    ra = p.ok ? batch_scaled_a(p, rnd) : vp1_inf();
    for (int j = 0; j < nsums; j++) terms[j] = p.ok ? batch_term(p, j, rnd) : g1_inf();
}
// sums: what lane `lane` adds up of term j (terms: kBatchSums per proof) and of the rho words of the proofs with ok
DEVFN G1X lane_sum(const G1X* terms, int j, const Part& pt, int lane) {
    G1X acc = g1_inf();
    for (uint32_t i = pt.begin + (uint32_t)lane; i < pt.end; i += kLanes) acc = g1_add(acc, terms[(size_t)kBatchSums * i + j]);
    return acc;
}
DEVFN void lane_rho(const uint32_t* rnd, const uint8_t* ok, const Part& pt, int lane, uint64_t (&col)[4]) {
    for (int c = 0; c < 4; c++) col[c] = 0;
    for (uint32_t i = pt.begin + (uint32_t)lane; i < pt.end; i += kLanes)
        if (ok[i]) for (int c = 0; c < 4; c++) col[c] += rnd[(size_t)kRandWords * i + c];
}
// product: lane `lane`'s share of the part's Miller values, its proofs' (f, indexed by proof) and the nfix of its fixed pairs
DEVFN F12 lane_product(const F12* f, const F12* fixed, int nfix, const Part& pt, int lane) {
    uint32_t i = pt.begin + (uint32_t)lane;
    F12 acc;
    if (lane < nfix) acc = fixed[lane];
    else if (i < pt.end) { acc = f[i]; i += kLanes; }
    else return one12();
    for (; i < pt.end; i += kLanes) acc = mul12(acc, f[i]);
    return acc;
}

// miller, 8-lane groups: group grp of a part's fixed pairs (pairs 3 grp .. 3 grp + 2 of its kBatchFixed points pts) over one f;
// live == false: no part in this group, it walks on the identity
template <class G> DEVFN typename G::V miller_fixed_few(G g, const KeyDev& k, const VP1* pts, int grp, bool live) {
    few::Stream st[kFewStreams];
    for (int t = 0; t < kFewStreams; t++) {
        const int j = kFewStreams * grp + t;
        st[t] = (live && j < kBatchFixed) ? few::stream(pts + j, k.lines[j], false, k.qinf[j] != 0, true) : few::no_stream();
    }
    return few::miller_few(g, st[0], st[1], st[2], few::no_stream(), kFewStreams);
}
// final: the part's verdict from its product (batch_accept by one group); live == false runs on the identity and yields false
template <class G> DEVFN bool final_few(G g, const F12* prod, bool live) {
    const typename G::V one = few::one12(g), in = few::load12(g, prod);
    return few::is_one12(g, few::final_exp(g, G::pick(live, in, one))) && live;
}

}  // namespace claims
}  // namespace vfy
}  // namespace gsc
