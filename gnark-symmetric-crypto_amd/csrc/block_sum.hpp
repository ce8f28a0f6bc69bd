// The block-wide sum of group points shared by the batched verifier (k_verify_batch.hip, G1) and the key ceremony's random combinations
// (k_phase2.hip, G1 and G2).  Device code only: include it from .hip files.
#pragma once
#include "verify_batch_dev.hpp"

namespace gsc {

// pairwise sums of v over the block's threads (N = blockDim.x, a power of two; lds: N entries); every thread gets the total.
// F: the coordinate field (bn254::Fp29f: G1, vfy::G1X; bn254::Fp2x: G2), deduced from v; the additions are the exact add-2008-s.
template <int N, class F>
__device__ bn254::Xyzz9<F> block_sum(bn254::Xyzz9<F> v, bn254::Xyzz9<F>* lds) {
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (int h = N / 2; h > 0; h >>= 1) {
        if (t < h) lds[t] = bn254::Curve9<F>::add(lds[t], lds[t + h]);
        __syncthreads();
    }
    const bn254::Xyzz9<F> r = lds[0];
    __syncthreads();
    return r;
}

}  // namespace gsc
