// The block-wide sum of G1 points shared by the batched verifier (k_verify_batch.hip) and the key ceremony's random combinations
// (k_phase2.hip).  Device code only: include it from .hip files.
#pragma once
#include "verify_batch_dev.hpp"

namespace gsc {

// pairwise sums of v over the block's threads (N = blockDim.x, a power of two; lds: N entries); every thread gets the total
template <int N>
__device__ vfy::G1X block_sum(vfy::G1X v, vfy::G1X* lds) {
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (int h = N / 2; h > 0; h >>= 1) {
        if (t < h) lds[t] = vfy::g1_add(lds[t], lds[t + h]);
        __syncthreads();
    }
    const vfy::G1X r = lds[0];
    __syncthreads();
    return r;
}

}  // namespace gsc
