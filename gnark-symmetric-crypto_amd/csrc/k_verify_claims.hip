// Claim-wise batched Groth16 check of one chunk (gsc_verify_claims / VerifyClaims), after k_verify_prep has filled ProofDev: the code of
// verify_claims_dev.hpp mapped onto threads.  The chunk is cut into parts (contiguous runs of proofs); every part is an equation of
// its own.  Launch order on one stream:
//   scale    one thread per proof: rho A (affine) and the proof's own terms; nothing is summed across a block
//   sums     one wave per part: lanes stride over the part's proofs, an LDS tree adds the lanes up; sum rho by integer column sums
//   fixed    one thread per (fixed pair, part): the G1 points of the part's fixed pairs
//   miller   the proofs' own pairs by the batched check's kernels (k_verify_batch.hip, or the lines + Miller kernels of
//            k_verify_few.hip); the fixed pairs against the key's lines: one thread per (pair, part), or on the few-proof path one
//            8-lane group per part that walks beta, gamma, delta as three streams over one f (a second group for ped_g, ped_gsn)
//   product  one wave per part: lane-strided partial products of the part's Miller values, then an LDS tree
//   final    one 8-lane group per part, 8 parts per wave: the final exponentiation and is_one12
// Blocks of the group kernels are one wave; a group without a part runs on the identity (nothing returns in front of a barrier).
#include "verify_claims_kernels.hpp"
#include "verify_few_kernels.hpp"

namespace gsc {
using namespace vfy;

namespace {

using claims::Part;
constexpr int kThreads = 64;

__global__ __launch_bounds__(kThreads) void k_verify_claims_scale(const ProofDev* pd, const uint32_t* rnd, size_t n, int nsums, VP1* ra, uint8_t* okv, G1X* terms) {
    const size_t i = blockIdx.x * (size_t)kThreads + threadIdx.x;
    if (i >= n) return;
    uint32_t r[kRandWords];
    for (int w = 0; w < kRandWords; w++) r[w] = rnd[kRandWords * i + w];
    okv[i] = pd[i].ok ? 1 : 0;
    claims::scale_one(pd[i], r, nsums, ra[i], terms + kBatchSums * i);
}

// block = part.  The totals overwrite the terms of the part's first proof; slot j of that proof is read in round j only.
__global__ __launch_bounds__(claims::kLanes) void k_verify_claims_sums(const Part* parts, const uint32_t* rnd, const uint8_t* okv, int nsums, G1X* terms, uint32_t* rho) {
    __shared__ G1X red[claims::kLanes];
    __shared__ uint64_t rs[claims::kLanes][4];
    const Part pt = parts[blockIdx.x];
    const int lane = threadIdx.x, width = claims::tree_width(pt.end - pt.begin);
    for (int j = 0; j < nsums; j++) {
        red[lane] = claims::lane_sum(terms, j, pt, lane);
        __syncthreads();
        for (int h = width / 2; h > 0; h >>= 1) {
            if (lane < h) red[lane] = g1_add(red[lane], red[lane + h]);
            __syncthreads();
        }
        if (lane == 0) terms[(size_t)kBatchSums * pt.begin + j] = red[0];
        __syncthreads();
    }
    uint64_t col[4];
    claims::lane_rho(rnd, okv, pt, lane, col);
    for (int c = 0; c < 4; c++) rs[lane][c] = col[c];
    __syncthreads();
    if (lane == 0) {
        for (int t = 1; t < width; t++) for (int c = 0; c < 4; c++) col[c] += rs[t][c];
        uint32_t s[5]; rho_sum_words(col, s);
        for (int c = 0; c < 5; c++) rho[5 * (size_t)blockIdx.x + c] = s[c];
    }
}

// thread t: fixed pair t / np of part t % np, so that the lanes of a wave share the pair (alpha's multiplication or one inversion)
__global__ __launch_bounds__(kThreads) void k_verify_claims_fixed(KeyDev k, const Part* parts, size_t np, int npairs, int nsums, const G1X* terms, const uint32_t* rho, VP1* fixed) {
    const size_t t = blockIdx.x * (size_t)kThreads + threadIdx.x;
    if (t >= np * npairs) return;
    const int j = (int)(t / np);
    const size_t p = t % np;
    G1X sums[kBatchSums]; uint32_t s[5];
    for (int q = 0; q < kBatchSums; q++) sums[q] = q < nsums ? terms[(size_t)kBatchSums * parts[p].begin + q] : g1_inf();
    for (int c = 0; c < 5; c++) s[c] = rho[5 * p + c];
    fixed[kBatchFixed * p + j] = batch_fixed_point(k, j, sums, s);
}

__global__ __launch_bounds__(kThreads) void k_verify_claims_miller_fixed(KeyDev k, const VP1* fixed, size_t np, int npairs, F12* pf) {
    const size_t t = blockIdx.x * (size_t)kThreads + threadIdx.x;
    if (t >= np * npairs) return;
    const int j = (int)(t / np);
    const size_t p = t % np;
    pf[npairs * p + j] = batch_miller_fixed(k, j, fixed[kBatchFixed * p + j]);
}
// group i: group i % ngrp of part i / ngrp
__global__ __launch_bounds__(kThreads) void k_verify_claims_few_miller_fixed(KeyDev k, const VP1* fixed, size_t np, int ngrp, F12* pf) {
    __shared__ e2 lds[few::kWaveLds];
    const few::WaveGroup g = few::wave_group(lds);
    const size_t i = blockIdx.x * (size_t)few::kGroupsPerWave + threadIdx.x / few::kGroup;
    const bool live = i < np * ngrp;
    const size_t p = live ? i / ngrp : 0;
    const e2 v = claims::miller_fixed_few(g, k, fixed + kBatchFixed * p, live ? (int)(i % ngrp) : 0, live);
    if (live) few::store12(g, v, pf + i);
}

// block = part; f: the proofs' Miller values by proof, pf: nfix values of fixed pairs per part.  The product goes to the part's pf[0].
__global__ __launch_bounds__(claims::kLanes) void k_verify_claims_product(const Part* parts, const F12* f, int nfix, F12* pf) {
    __shared__ F12 red[claims::kLanes];
    const Part pt = parts[blockIdx.x];
    F12* mine = pf + (size_t)nfix * blockIdx.x;
    const uint32_t len = pt.end - pt.begin;
    const int lane = threadIdx.x, width = claims::tree_width(len > (uint32_t)nfix ? len : (uint32_t)nfix);
    red[lane] = claims::lane_product(f, mine, nfix, pt, lane);
    __syncthreads();
    for (int h = width / 2; h > 0; h >>= 1) {
        if (lane < h) red[lane] = mul12(red[lane], red[lane + h]);
        __syncthreads();
    }
    if (lane == 0) mine[0] = red[0];
}

// k_verify_few_final with one group per part: the product of part i is pf[nfix i]
__global__ __launch_bounds__(kThreads) void k_verify_claims_final(const F12* pf, int nfix, size_t np, uint8_t* flag) {
    __shared__ e2 lds[few::kWaveLds];
    const few::WaveGroup g = few::wave_group(lds);
    const size_t i = blockIdx.x * (size_t)few::kGroupsPerWave + threadIdx.x / few::kGroup;
    const bool live = i < np;
    const bool ok = claims::final_few(g, pf + (live ? (size_t)nfix * i : 0), live);
    if (live && g.k == 0) flag[i] = ok ? 1 : 0;
}

unsigned blocks(size_t n, size_t per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

void launch_verify_claims(const KeyDev& k, const ProofDev* pd, const uint32_t* rnd, size_t n, size_t np, const BatchBufs& b, const ClaimBufs& c,
                          Line* few_lines, hipStream_t s) {
    if (!n || !np) return;
    const int nsums = k.has_commitment ? kBatchSums : 2, npairs = claims::fixed_pairs(k.has_commitment != 0);
    const int nfix = few_lines ? claims::fixed_groups(k.has_commitment != 0) : npairs;
    hipLaunchKernelGGL(k_verify_claims_scale, dim3(blocks(n, kThreads)), dim3(kThreads), 0, s, pd, rnd, n, nsums, b.ra, b.ok, c.terms);
    hipLaunchKernelGGL(k_verify_claims_sums, dim3((unsigned)np), dim3(claims::kLanes), 0, s, c.parts, rnd, b.ok, nsums, c.terms, c.rho);
    hipLaunchKernelGGL(k_verify_claims_fixed, dim3(blocks(np * npairs, kThreads)), dim3(kThreads), 0, s, k, c.parts, np, npairs, nsums, c.terms, c.rho, c.fixed);
    if (few_lines) {
        launch_verify_few_lines(pd, n, few_lines, s);
        launch_verify_few_proof_miller(k, pd, b.ra, few_lines, n, b.f, s);
        hipLaunchKernelGGL(k_verify_claims_few_miller_fixed, dim3(blocks(np * nfix, few::kGroupsPerWave)), dim3(kThreads), 0, s, k, c.fixed, np, nfix, c.pf);
    } else {
        launch_verify_batch_proof_miller(k, pd, b.ra, n, b.f, s);
        hipLaunchKernelGGL(k_verify_claims_miller_fixed, dim3(blocks(np * npairs, kThreads)), dim3(kThreads), 0, s, k, c.fixed, np, npairs, c.pf);
    }
    hipLaunchKernelGGL(k_verify_claims_product, dim3((unsigned)np), dim3(claims::kLanes), 0, s, c.parts, b.f, nfix, c.pf);
    hipLaunchKernelGGL(k_verify_claims_final, dim3(blocks(np, few::kGroupsPerWave)), dim3(kThreads), 0, s, c.pf, nfix, np, c.flag);
}

}  // namespace gsc
