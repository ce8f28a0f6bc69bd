// Batched Groth16 check of one chunk (gsc_verify_raw_batched / gsc_verify_all), after k_verify_prep has filled ProofDev: the
// per-thread code of verify_batch_dev.hpp mapped onto threads.  Launch order on one stream:
//   scale  one thread per proof: rho A (affine), block partials of sum rho L, sum rho C (AES: sum t D, sum t PoK) and of sum rho
//   sum    one block: the chunk's totals and the G1 points of the fixed pairs (-(sum rho) alpha, ...)
//   miller one thread per proof: f_i = e(rho A, B) unreduced; one extra block: the fixed pairs against the key's lines
//   tree   products of 4 in place, until one Fp12 is left
//   final  the final exponentiation of that product: one flag per chunk, by one group of lanes (k_verify_few.hip)
// A chunk on the few-proof path takes k_verify_few.hip's lines + Miller kernels in place of `miller`.
#include "verify_batch_kernels.hpp"
#include "verify_few_kernels.hpp"
#include "verify_batch_dev.hpp"
#include "block_sum.hpp"

namespace gsc {
using namespace vfy;

namespace {

constexpr int kScaleThreads = 64;
constexpr int kSumThreads = 64 * kBatchFixed;       // one wave per fixed point; waves 0..3 also reduce one total each

__global__ __launch_bounds__(kScaleThreads) void k_verify_batch_scale(const ProofDev* pd, const uint32_t* rnd, size_t n, int nsums, VP1* ra,
                                                                      uint8_t* okv, G1X* part, uint64_t* rpart) {
    __shared__ G1X red[kScaleThreads];
    __shared__ uint64_t rs[kScaleThreads][4];
    const size_t i = blockIdx.x * (size_t)kScaleThreads + threadIdx.x;
    const bool ok = i < n && pd[i].ok;
    uint32_t r[kRandWords];
    for (int w = 0; w < kRandWords; w++) r[w] = ok ? rnd[kRandWords * i + w] : 0;
    if (i < n) {
        okv[i] = ok ? 1 : 0;
        ra[i] = ok ? batch_scaled_a(pd[i], r) : vp1_inf();
    }
    for (int j = 0; j < kBatchSums; j++) {
        G1X s = g1_inf();
        if (j < nsums) s = block_sum<kScaleThreads>(ok ? batch_term(pd[i], j, r) : g1_inf(), red);
        if (threadIdx.x == 0) part[kBatchSums * blockIdx.x + j] = s;
    }
    for (int w = 0; w < 4; w++) rs[threadIdx.x][w] = r[w];
    __syncthreads();
    if (threadIdx.x < 4) {
        uint64_t c = 0;
        for (int t = 0; t < kScaleThreads; t++) c += rs[t][threadIdx.x];
        rpart[4 * blockIdx.x + threadIdx.x] = c;
    }
}

__global__ __launch_bounds__(kSumThreads) void k_verify_batch_sum(KeyDev k, const G1X* part, const uint64_t* rpart, size_t nblk, VP1* fixed) {
    __shared__ G1X red[kBatchSums][64];
    __shared__ G1X tot[kBatchSums];
    __shared__ uint32_t rho[5];
    const int w = threadIdx.x / 64, lane = threadIdx.x % 64;
    if (w < kBatchSums) {
        G1X acc = g1_inf();
        for (size_t b = lane; b < nblk; b += 64) acc = g1_add(acc, part[kBatchSums * b + w]);
        red[w][lane] = acc;
    } else if (lane == 0) {
        uint64_t col[4] = {0, 0, 0, 0};
        for (size_t b = 0; b < nblk; b++) for (int c = 0; c < 4; c++) col[c] += rpart[4 * b + c];
        uint32_t s[5]; rho_sum_words(col, s);
        for (int c = 0; c < 5; c++) rho[c] = s[c];
    }
    __syncthreads();
    for (int h = 32; h > 0; h >>= 1) {
        if (w < kBatchSums && lane < h) red[w][lane] = g1_add(red[w][lane], red[w][lane + h]);
        __syncthreads();
    }
    if (w < kBatchSums && lane == 0) tot[w] = red[w][0];
    __syncthreads();
    if (lane == 0) {
        G1X sums[kBatchSums]; uint32_t s[5];
        for (int j = 0; j < kBatchSums; j++) sums[j] = tot[j];
        for (int c = 0; c < 5; c++) s[c] = rho[c];
        fixed[w] = batch_fixed_point(k, w, sums, s);
    }
}

// blocks [0, nb): proof i; block nb: fixed pair t (t < kBatchFixed), written behind the n proofs.  One copy of the loop serves both.
__global__ __launch_bounds__(64) void k_verify_batch_miller(KeyDev k, const ProofDev* pd, const VP1* ra, const VP1* fixed, size_t n, F12* f) {
    const size_t nb = (n + 63) / 64;
    VP1 p; VP2 q; bool qinf; const Line* lines; size_t o;
    if (blockIdx.x < nb) {
        const size_t i = blockIdx.x * (size_t)64 + threadIdx.x;
        if (i >= n) return;
        if (!pd[i].ok) { f[i] = one12(); return; }
        p = ra[i]; q = pd[i].B; qinf = q.inf != 0; lines = nullptr; o = i;
    } else {
        const int t = threadIdx.x;
        if (t >= kBatchFixed) return;
        p = fixed[t]; q.x = q.y = F2::zero(); q.inf = 1; qinf = k.qinf[t] != 0; lines = k.lines[t]; o = n + t;
    }
    f[o] = miller_one(p, q, qinf, lines);
}

__global__ __launch_bounds__(64) void k_verify_batch_tree(F12* f, size_t n, size_t h) {
    const size_t i = blockIdx.x * (size_t)64 + threadIdx.x;
    if (i >= h) return;
    F12 acc = f[i];
    for (size_t j = i + h; j < n; j += h) acc = mul12(acc, f[j]);
    f[i] = acc;
}

unsigned blocks(size_t n) { return (unsigned)((n + 63) / 64); }

}  // namespace

size_t batch_blocks(size_t n) { return (n + kScaleThreads - 1) / kScaleThreads; }

void launch_verify_batch_proof_miller(const KeyDev& k, const ProofDev* pd, const VP1* ra, size_t n, F12* f, hipStream_t s) {
    // without the extra block every block takes k_verify_batch_miller's proof branch
    if (n) hipLaunchKernelGGL(k_verify_batch_miller, dim3(blocks(n)), dim3(64), 0, s, k, pd, ra, (const VP1*)nullptr, n, f);
}

void launch_verify_batch(const KeyDev& k, const ProofDev* pd, const uint32_t* rnd, size_t n, const BatchBufs& b, Line* few_lines, hipStream_t s) {
    if (!n) return;
    const size_t nblk = batch_blocks(n);
    hipLaunchKernelGGL(k_verify_batch_scale, dim3((unsigned)nblk), dim3(kScaleThreads), 0, s, pd, rnd, n, k.has_commitment ? kBatchSums : 2,
                       b.ra, b.ok, b.part, b.rpart);
    hipLaunchKernelGGL(k_verify_batch_sum, dim3(1), dim3(kSumThreads), 0, s, k, b.part, b.rpart, nblk, b.fixed);
    if (few_lines) {
        launch_verify_few_lines(pd, n, few_lines, s);
        launch_verify_few_batch_miller(k, pd, b.ra, b.fixed, few_lines, n, b.f, s);
    } else hipLaunchKernelGGL(k_verify_batch_miller, dim3(blocks(n) + 1), dim3(64), 0, s, k, pd, b.ra, b.fixed, n, b.f);
    // every product pass folds 4 values into one: f[i] *= f[i + h] f[i + 2h] f[i + 3h], h = ceil(m / 4)
    for (size_t m = n + kBatchFixed; m > 1;) {
        const size_t h = (m + 3) / 4;
        hipLaunchKernelGGL(k_verify_batch_tree, dim3(blocks(h)), dim3(64), 0, s, b.f, m, h);
        m = h;
    }
    launch_verify_few_final(b.f, b.flag, s);
}

}  // namespace gsc
