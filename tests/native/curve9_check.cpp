// Host build of the group-law test hook (csrc/debug_ops.hpp, dbg::curve_op): the same element function gsc_debug_curve_ops runs on the
// device, here over Curve9 with the plain-C products.  tests/test_debug_ops_host.py compares the output with the affine reference of
// tests/devref.py, which proves the case tables and the reference without a GPU.
//   stdin : group, op, n, k (int32 LE) | pts: n x k points | inf: n x k bytes | lam: n x 2 scales   (layout: include/libprove.h)
//   stdout: n affine results | n flag bytes
#include "debug_ops.hpp"
#include <cstdio>
#include <vector>
using namespace bn254;

template <class F>
static int run(int op, size_t n, size_t k) {
    constexpr size_t W = F::WORDS;
    std::vector<fe> pts(2 * W * k * n), lam(2 * W * n), out(2 * W * n);
    std::vector<uint8_t> inf(k * n), flags(n);
    if (fread(pts.data(), sizeof(fe), pts.size(), stdin) != pts.size() || fread(inf.data(), 1, inf.size(), stdin) != inf.size() ||
        fread(lam.data(), sizeof(fe), lam.size(), stdin) != lam.size()) return 2;
    for (size_t i = 0; i < n; i++) flags[i] = (uint8_t)dbg::curve_op<F>(op, k, &pts[2 * W * k * i], &inf[k * i], &lam[2 * W * i], &out[2 * W * i]);
    return fwrite(out.data(), sizeof(fe), out.size(), stdout) == out.size() && fwrite(flags.data(), 1, n, stdout) == n ? 0 : 2;
}

int main() {
    int32_t hdr[4];
    if (fread(hdr, 4, 4, stdin) != 4 || hdr[0] < 0 || hdr[0] > 1 || hdr[1] < 0 || hdr[1] >= dbg::CURVE_OPS || hdr[2] < 0 || hdr[3] < 1) return 2;
    return hdr[0] == 0 ? run<Fp29f>(hdr[1], (size_t)hdr[2], (size_t)hdr[3]) : run<Fp2x>(hdr[1], (size_t)hdr[2], (size_t)hdr[3]);
}
