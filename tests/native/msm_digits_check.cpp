// Host build of the one signed-digit recoder of the MSM (csrc/msm_dev.hpp, signed_digit_step): every window of every scalar by repeated
// calls, as k_recode makes them.  tests/test_msm_digits_host.py checks the digits with Python integers for every width.
//   stdin : c, n (int32 LE) | negated: n bytes | scalars: n canonical values, 8 x u32 LE each
//   stdout: n x msm_windows(c) digits (int32 LE) | n bytes: the carry left after the last window
#include "msm_dev.hpp"
#include <cstdio>
#include <vector>
using namespace bn254;

int main() {
    int32_t hdr[2];
    if (fread(hdr, 4, 2, stdin) != 2 || hdr[0] < 2 || hdr[0] > gsc::MSM_MAX_WINDOW || hdr[1] < 0) return 2;
    const uint32_t c = (uint32_t)hdr[0]; const size_t n = (size_t)hdr[1], nwin = (size_t)gsc::msm_windows(hdr[0]);
    std::vector<uint8_t> negated(n), left(n);
    std::vector<fe> scalars(n);
    std::vector<int32_t> digits(n * nwin);
    if (fread(negated.data(), 1, n, stdin) != n || fread(scalars.data(), sizeof(fe), n, stdin) != n) return 2;
    for (size_t i = 0; i < n; i++) {
        fe s = scalars[i]; uint32_t carry = 0;
        for (size_t j = 0; j < nwin; j++) digits[i * nwin + j] = gsc::signed_digit_step(s, c, carry, negated[i] != 0);
        left[i] = (uint8_t)carry;
        for (int q = 0; q < 8; q++) if (s.l[q]) left[i] |= 2;      // bits of the scalar that no window took
    }
    return fwrite(digits.data(), 4, digits.size(), stdout) == digits.size() && fwrite(left.data(), 1, n, stdout) == n ? 0 : 2;
}
