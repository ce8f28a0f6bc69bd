// TEST HOOK kernels of gsc_debug_tower_ops (include/libprove.h): one operation of the verifier's tower per element, raw limbs in and out
// (debug_tower_ops.hpp).  A translation unit of its own: the production verifier kernels are compiled without it, and no production
// path launches these.
//   path 0  one element per thread, the serial code of verify_dev.hpp
//   path 1  one element per 8-lane group of a one-wave block, the lane-sliced code of verify_few_dev.hpp with its exchange slots in LDS
//           as in k_verify_few.hip; a group without an element computes on the identity (no early return in front of a barrier)
#include "kernels.hpp"
#include "debug_tower_ops.hpp"

namespace gsc {
using namespace vfy;

namespace {

__global__ __launch_bounds__(64) void k_tower_ops(int op, const int32_t* in, int32_t* out, uint8_t* flags, size_t n, int in_words, int out_words) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    flags[i] = (uint8_t)dbg::tower_op(op, in + (size_t)in_words * i, out + (size_t)out_words * i);
}
__global__ __launch_bounds__(64) void k_tower_group_ops(int op, const int32_t* in, int32_t* out, uint8_t* flags, size_t n, int in_words, int out_words) {
    __shared__ e2 lds[few::kWaveLds];
    const few::WaveGroup g = few::wave_group(lds);
    const size_t i = blockIdx.x * (size_t)few::kGroupsPerWave + threadIdx.x / few::kGroup;
    const bool live = i < n;
    bool flag;
    const e2 v = dbg::tower_group_op(g, op, live ? in + (size_t)in_words * i : nullptr, flag);
    if (!live) return;      // behind the last exchange
    if (out_words) dbg::st2(out + (size_t)out_words * i + dbg::kW2 * g.k, v);
    if (g.k == 0) flags[i] = flag ? 1 : 0;
}

}  // namespace

bool tower_ops_words(int path, int op, int* in_words, int* out_words) {
    if (!dbg::tower_has(path, op)) return false;
    *in_words = dbg::tower_in_words(op); *out_words = dbg::tower_out_words(path, op);
    return true;
}
bool launch_tower_ops(int path, int op, const int32_t* in, int32_t* out, uint8_t* flags, size_t n, hipStream_t s) {
    int iw, ow;
    if (!tower_ops_words(path, op, &iw, &ow)) return false;
    if (!n) return true;
    if (path == 0) hipLaunchKernelGGL(k_tower_ops, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, op, in, out, flags, n, iw, ow);
    else hipLaunchKernelGGL(k_tower_group_ops, dim3((unsigned)((n + few::kGroupsPerWave - 1) / few::kGroupsPerWave)), dim3(64), 0, s, op, in, out, flags, n, iw, ow);
    return true;
}

}  // namespace gsc
