// Host build of the carry-folded Montgomery products (bn254_fp29.hpp, namespace madc): every column's terms, in the order and
// grouping the device code issues them, must give the limbs of Field29's mul / sqr / fmms exactly.  Prints the mismatch count.
#include "bn254_fp29.hpp"
#include <cstdio>
#include <random>
using namespace bn254;

int main() {
    std::mt19937_64 g(2026);
    long bad = 0, n = 0;
    // |limb| < 2^29: tight (limbs 0..7 non-negative) or signed-tight operands, with extreme limbs mixed in
    auto rnd = [&](bool sgn) {
        fe9 r;
        for (int i = 0; i < 9; i++) {
            int32_t v = (int32_t)(g() & ((1u << 29) - 1));
            if (g() % 7 == 0) v = (1 << 29) - 1;
            if (sgn && (g() & 1)) v = -v;
            r.l[i] = v;
        }
        return r;
    };
    for (int it = 0; it < 100000; it++) {
        const bool sg = it & 1;
        const fe9 a = rnd(sg), b = rnd(sg), c = rnd(sg), d = rnd(sg);
        const fe9 r[8] = {Fp29::mul(a, b), madc::mont<Fp29Q, false, false>(a, b, a, b),
                          Fp29::sqr(a), madc::mont<Fp29Q, false, true>(a, Fp29::dbl(a), a, a),
                          Fp29::fmms(a, b, c, d), madc::mont<Fp29Q, true, false>(a, b, Fp29::neg(c), d),
                          Fr29::mul(a, b), madc::mont<Fr29Q, false, false>(a, b, a, b)};
        for (int k = 0; k < 8; k += 2)
            for (int i = 0; i < 9; i++) bad += r[k].l[i] != r[k + 1].l[i];
        n += 4;
    }
    printf("%ld %ld\n", n, bad);
    return bad != 0;
}
