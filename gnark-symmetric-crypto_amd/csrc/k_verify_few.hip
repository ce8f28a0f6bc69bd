// Few-proof verifier kernels: a group of 8 lanes inside one wave verifies one proof with the lane-sliced arithmetic of
// verify_few_dev.hpp, so that a single claim is answered in the time of one shared pairing instead of one thread's.  Reached by
// small calls of gsc_verify_raw / VerifyBatch / gsc_verify_raw_batched / gsc_verify_all (verify_gpu.cpp routes them); the final
// exponentiation of the batched check (k_verify_batch.hip) runs here at every call size.  After k_verify_prep:
//   lines    one thread per proof: the Miller lines of the proof's own B (lines_of), so that no point arithmetic is left in the loop
//   pairing  one group per proof: four line streams over a shared f, the final exponentiation, is_one12
// Every block is one wave of 8 groups; a group without a proof runs on the identity (no early return: the groups of a wave exchange
// operands behind common barriers).
#include "verify_few_kernels.hpp"
#include "verify_few_dev.hpp"
#include "verify_batch_dev.hpp"

namespace gsc {
using namespace vfy;

namespace {

constexpr int kFewThreads = 64;
constexpr int kFewLds = few::kWaveLds;      // Fp2 slices per block
using few::wave_group;

__global__ __launch_bounds__(64) void k_verify_few_lines(const ProofDev* pd, size_t n, Line* out) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i < n && pd[i].ok && !pd[i].A.inf && !pd[i].B.inf) lines_of(pd[i].B, out + kLineSteps * i);
}
__global__ __launch_bounds__(kFewThreads) void k_verify_few_pairing(KeyDev k, const ProofDev* pd, const Line* lines, uint8_t* verdict, F12* fout, size_t n) {
    __shared__ e2 lds[kFewLds];
    const few::WaveGroup g = wave_group(lds);
    const size_t i = blockIdx.x * (size_t)few::kGroupsPerWave + threadIdx.x / few::kGroup;
    const bool live = i < n && pd[i].ok;
    const bool ok = few::pair_few(g, k, live ? pd + i : nullptr, lines + kLineSteps * (live ? i : 0), live, (fout && live) ? fout + i : nullptr);
    if (i < n && g.k == 0) verdict[i] = ok ? 1 : 0;
}
// batched check, one pair per group with f unreduced: groups [0, n) e(rho A_i, B_i) over the proof's lines (1 for a proof without ok or
// with a point at infinity), groups [n, n + nfixed) the fixed pair t against the key's lines, written behind the n proofs
__global__ __launch_bounds__(kFewThreads) void k_verify_few_batch_miller(KeyDev k, const ProofDev* pd, const VP1* ra, const VP1* fixed, const Line* lines, size_t n, size_t nfixed, F12* f) {
    __shared__ e2 lds[kFewLds];
    const few::WaveGroup g = wave_group(lds);
    const size_t i = blockIdx.x * (size_t)few::kGroupsPerWave + threadIdx.x / few::kGroup;
    few::Stream st = few::no_stream();
    if (i < n) { if (pd[i].ok) st = few::stream(ra + i, lines + kLineSteps * i, false, pd[i].B.inf != 0, true); }
    else if (i < n + nfixed) st = few::stream(fixed + (i - n), k.lines[i - n], false, k.qinf[i - n] != 0, true);
    const e2 v = few::miller_few(g, st, few::no_stream(), few::no_stream(), few::no_stream(), 1);
    if (i < n + nfixed) few::store12(g, v, f + i);
}
// the chunk's verdict from the product of every Miller value (batch_accept of verify_batch_dev.hpp): group 0 works, the rest idle on 1
__global__ __launch_bounds__(kFewThreads) void k_verify_few_final(const F12* f, uint8_t* flag) {
    __shared__ e2 lds[kFewLds];
    const few::WaveGroup g = wave_group(lds);
    const bool mine = threadIdx.x < few::kGroup;
    const e2 one = few::one12(g), in = few::load12(g, f);
    const e2 v = few::final_exp(g, few::sel2(mine, in, one));
    const bool ok = few::is_one12(g, v);
    if (threadIdx.x == 0) flag[0] = ok ? 1 : 0;
}

unsigned blocks(size_t n, size_t per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

void launch_verify_few_lines(const ProofDev* pd, size_t n, Line* out, hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_verify_few_lines, dim3(blocks(n, 64)), dim3(64), 0, s, pd, n, out);
}
void launch_verify_few_pairing(const KeyDev& k, const ProofDev* pd, const Line* lines, uint8_t* verdict, F12* fout, size_t n, hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_verify_few_pairing, dim3(blocks(n, few::kGroupsPerWave)), dim3(kFewThreads), 0, s, k, pd, lines, verdict, fout, n);
}
void launch_verify_few_batch_miller(const KeyDev& k, const ProofDev* pd, const VP1* ra, const VP1* fixed, const Line* lines, size_t n, F12* f, hipStream_t s) {
    hipLaunchKernelGGL(k_verify_few_batch_miller, dim3(blocks(n + kBatchFixed, few::kGroupsPerWave)), dim3(kFewThreads), 0, s, k, pd, ra, fixed, lines, n, (size_t)kBatchFixed, f);
}
void launch_verify_few_proof_miller(const KeyDev& k, const ProofDev* pd, const VP1* ra, const Line* lines, size_t n, F12* f, hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_verify_few_batch_miller, dim3(blocks(n, few::kGroupsPerWave)), dim3(kFewThreads), 0, s, k, pd, ra, (const VP1*)nullptr, lines, n, (size_t)0, f);
}
void launch_verify_few_final(const F12* f, uint8_t* flag, hipStream_t s) {
    hipLaunchKernelGGL(k_verify_few_final, dim3(1), dim3(kFewThreads), 0, s, f, flag);
}

}  // namespace gsc
