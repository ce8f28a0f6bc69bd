// Host build of the raw-limb test hook (csrc/debug_ops.hpp, dbg::limb_op): the same element function gsc_debug_limb_ops runs on the
// device, with the plain-C products the headers have on a host.  Field 2 takes its products from madc::mont's host fallback, so the
// grouping of the chained form is what runs.  tests/test_debug_ops_host.py compares the output with the predictions of tests/devref.py.
//   stdin : field, op, n (int32 LE) | a, b, c, d: n x 9 int32 each
//   stdout: n x 9 int32
#include "debug_ops.hpp"
#include <cstdio>
#include <vector>
using namespace bn254;

struct Fp29Chained : Fp29 {
    static fe9 mul(const fe9& a, const fe9& b) { return madc::mont<Fp29Q, false, false>(a, b, a, b); }
    static fe9 sqr(const fe9& a) { return madc::mont<Fp29Q, false, true>(a, Fp29::dbl(a), a, a); }
    static fe9 fmms(const fe9& a, const fe9& b, const fe9& c, const fe9& d) { return madc::mont<Fp29Q, true, false>(a, b, Fp29::neg(c), d); }
};

int main() {
    int32_t hdr[3];
    if (fread(hdr, 4, 3, stdin) != 3 || hdr[0] < 0 || hdr[0] > 2 || hdr[1] < 0 || hdr[1] >= dbg::LIMB_OPS || hdr[2] < 0) return 2;
    const size_t n = (size_t)hdr[2];
    std::vector<fe9> v[4], out(n);
    for (auto& x : v) { x.resize(n); if (fread(x.data(), sizeof(fe9), n, stdin) != n) return 2; }
    for (size_t i = 0; i < n; i++)
        out[i] = hdr[0] == 0 ? dbg::limb_op<Fp29>(hdr[1], v[0][i], v[1][i], v[2][i], v[3][i])
               : hdr[0] == 1 ? dbg::limb_op<Fr29>(hdr[1], v[0][i], v[1][i], v[2][i], v[3][i])
                             : dbg::limb_op<Fp29Chained>(hdr[1], v[0][i], v[1][i], v[2][i], v[3][i]);
    return fwrite(out.data(), sizeof(fe9), n, stdout) == n ? 0 : 2;
}
