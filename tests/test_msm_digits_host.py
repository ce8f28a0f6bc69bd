"""The signed c-bit recoding of the MSM has ONE definition (csrc/msm_dev.hpp, signed_digit_step) behind k_recode, the window octets of
k_recode_flat, k_fixed_mul and the digit-writing tail of the last quotient transform.  The GPU tests reach the widths the knobs select
(6, 9, 11, 13, 15, 17); here the helper is built for the host and every width 2 .. 17 is checked with Python integers: digit range,
the value the digits stand for, and that msm_windows(c) windows absorb the last carry (csrc/kernels.hpp)."""
import random
import struct
import subprocess

import pytest

import devref as D

R = D.R
HALF = (R - 1) // 2


def msm_windows(c):
    # the fewest windows whose top one takes the last carry without overflow: floor((r-1) / 2^(c (nwin-1))) + 1 <= 2^(c-1) - 1
    nwin = 1
    while ((R - 1) >> (c * (nwin - 1))) + 1 > (1 << (c - 1)) - 1:
        nwin += 1
    return nwin


def scalars_for(c, negated):
    nwin, Dh = msm_windows(c), 1 << (c - 1)
    bound = HALF if negated else R - 1      # a negated scalar is the magnitude sign_normalise hands the recoder: <= (r-1)/2
    vals = [0, 1, R - 1, HALF, HALF + 1]
    for w in (Dh - 1, Dh, Dh + 1):          # the carry chain and the moved threshold; the top window cleared (and the next, while too large)
        top = nwin - 1
        while True:
            v = sum(w << (c * j) for j in range(top))
            if v <= bound:
                break
            top -= 1
        vals.append(v)
    rnd = random.Random(1000 + c)
    vals += [rnd.randrange(bound + 1) for _ in range(256)]
    return [v if v <= bound else R - v for v in vals]


@pytest.fixture(scope="module")
def digits_exe():
    return D.native_exe("msm_digits_check")


@pytest.mark.parametrize("negated", [False, True], ids=["plain", "negated"])
@pytest.mark.parametrize("c", range(2, 18))
def test_signed_digits_of_every_width(digits_exe, c, negated):
    vals = scalars_for(c, negated)
    n, nwin, Dh = len(vals), msm_windows(c), 1 << (c - 1)
    payload = struct.pack("<2i", c, n) + bytes([1 if negated else 0] * n) + b"".join(v.to_bytes(32, "little") for v in vals)
    out = subprocess.run([digits_exe], input=payload, capture_output=True, timeout=60, check=True).stdout
    assert len(out) == n * (4 * nwin + 1)      # msm_windows(c) digits per scalar
    digits, left = struct.unpack("<%di" % (n * nwin), out[:4 * n * nwin]), out[4 * n * nwin:]
    for i, s in enumerate(vals):
        d = digits[i * nwin:(i + 1) * nwin]
        assert all(-Dh <= e <= Dh - 1 for e in d), (c, hex(s), d)
        assert sum(e << (c * j) for j, e in enumerate(d)) == (-s if negated else s), (c, hex(s), d)
        assert left[i] == 0, (c, hex(s))      # no carry (bit 0) and no scalar bits (bit 1) after the last window
