// The prover's self-check (gsc_prove_check_init): k_check_prep turns the affine points a chunk's assembly has just left in the lane's output
// buffers into the verifier's ProofDev entries, so that the verifier's own kernels (k_verify_batch.hip, k_verify_few.hip, k_verify.hip) decide
// the chunk before anything is downloaded.  It is k_verify_prep's twin (verify_dev.hpp prep_affine_one / prep_one): no upload, no
// decompression, no square root.  One thread per statement.
#include "prove_check_kernels.hpp"

namespace gsc {
using namespace vfy;

namespace {

__global__ __launch_bounds__(64) void k_check_prep(KeyDev k, ProverOut o, const uint8_t* win, ProofDev* pd) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= o.n) return;
    ProofDev p;
    p.ok = 0;
    // a statement the prover refuses anyway (serialize: solver status, infinity flags) takes no part
    if (o.status[i] == 0xFFFFFFFFu && o.flags[i] == 0)
        prep_affine_one(k, o.out + 256 * i, o.cpts + 64 * i, o.cpts + 64 * o.B + 64 * i, win + kWindows * i, p);
    pd[i] = p;
}

// one thread: the 64 (G1) or 128 (G2) bytes of one point of one column
__global__ void k_prove_corrupt(uint8_t* out, uint8_t* cpts, size_t B, size_t n, uint32_t index, int which, int mode) {
    if (blockIdx.x || threadIdx.x || index >= n || which < 0 || which > 4) return;
    const size_t other = ((size_t)index + 1) % n;
    uint8_t* base = which < 3 ? out : cpts + (which == 4 ? 64 * B : 0);
    const size_t stride = which < 3 ? 256 : 64, at = which == 1 ? 64 : which == 2 ? 192 : 0, len = which == 1 ? 128 : 64;
    uint8_t* dst = base + stride * index + at;
    if (mode == 0) { const uint8_t* src = base + stride * other + at; for (size_t j = 0; j < len; j++) dst[j] = src[j]; }
    else dst[which < 3 ? len / 2 : 63] ^= 1;      // y: little-endian words in d_out (its first byte), big-endian bytes in d_cpts (its last)
}

}  // namespace

void launch_check_prep(const KeyDev& k, const ProverOut& o, const uint8_t* win, ProofDev* pd, hipStream_t s) {
    if (o.n) hipLaunchKernelGGL(k_check_prep, dim3((unsigned)((o.n + 63) / 64)), dim3(64), 0, s, k, o, win, pd);
}
void launch_prove_corrupt(uint8_t* out, uint8_t* cpts, size_t B, size_t n, uint32_t index, int which, int mode, hipStream_t s) {
    hipLaunchKernelGGL(k_prove_corrupt, dim3(1), dim3(1), 0, s, out, cpts, B, n, index, which, mode);
}

}  // namespace gsc
