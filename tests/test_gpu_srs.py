"""GPU tests of gsc_srs_verify (the check of a powers file) and of the test hook that writes one.
Files come from two writers: tests/srsmodel.py (Python, from known tau, alpha, beta, L = 2) and gsc_debug_srs_generate (L = 2, 6, 7: the sums
of the check then cover 2N-2 / N-1 = 6 / 3, 126 / 63 and 254 / 127 points against the 64-thread blocks of k_phase2_rlc — one below a block, a
partial second block, a partial fourth).  A wrong file differs from a right one in ONE element, replaced by another valid point of its group
(or in one byte, for the decoding rules), so that the rule the case is about decides; the line the library prints names the rule."""
import pytest

import devref
import keyraw
import srsmodel

pytestmark = pytest.mark.gpu

RLC_THREADS = 64                                       # k_phase2.hip kThreads
SEED = bytes([7] * 32)
TAU, ALPHA, BETA = 0x1234567, 0xabcdef01, 0x31415926
OTHER1 = keyraw.enc_g1(keyraw.g1_mul(srsmodel.G1, 5), True)      # valid points that belong nowhere in the files below
OTHER2 = keyraw.enc_g2(keyraw.g2_mul(srsmodel.G2, 5), True)


def toxic(seed, label):
    """gsc_setup's seeded scalar (csrc/setup.cpp toxic): expand_message_xmd(SHA-256) of seed | label padded to 32 bytes, 48 bytes out,
    DST "gsc-test-setup", as a big-endian integer mod r"""
    msg = seed + label.encode().ljust(32, b"\0")
    return int.from_bytes(devref.expand_message_xmd48(msg, b"gsc-test-setup"), "big") % keyraw.R or 1


@pytest.fixture(scope="module")
def model_file():
    return srsmodel.write(2, TAU, ALPHA, BETA)


@pytest.fixture(scope="module")
def generated(gsc):
    return {L: gsc.debug_srs_generate(L, SEED) for L in (2, 6, 7)}


def _verdict(gsc, capfd, srs):
    capfd.readouterr()
    ok = gsc.srs_verify(srs)
    return ok, capfd.readouterr().out


@pytest.mark.parametrize("L", [2, 6, 7])
def test_a_generated_file_is_accepted(gsc, capfd, generated, L):
    N = 1 << L
    assert (2 * N - 2) % RLC_THREADS != 0 and (N - 1) % RLC_THREADS != 0 and (2 * N - 2 < RLC_THREADS) == (L == 2)
    assert len(generated[L]) == srsmodel.layout(L)["bytes"]
    ok, out = _verdict(gsc, capfd, generated[L])
    assert ok and "rule" not in out, out


def test_the_python_made_file_is_accepted(gsc, capfd, model_file):
    ok, out = _verdict(gsc, capfd, model_file)
    assert ok and "rule" not in out, out


def test_the_generator_writes_what_the_model_writes(gsc, generated):
    """the hook's file for the seed's tau, alpha, beta equals the Python writer's, byte for byte: format, element order and the derivation of
    the scalars (gsc_setup's) are pinned by a second implementation"""
    assert generated[2] == srsmodel.write(2, toxic(SEED, "tau"), toxic(SEED, "alpha"), toxic(SEED, "beta"))
    # the same tau underlies every size: a smaller file is a prefix of each section of a larger one
    for sec, count in (("tauG1", 7), ("tauG2", 4), ("alphaG1", 4), ("betaG1", 4), ("betaG2", 1)):
        w = 128 if sec.endswith("G2") else 64
        a, b = srsmodel.offset(2, sec), srsmodel.offset(6, sec)
        assert generated[2][a:a + w * count] == generated[6][b:b + w * count], sec


def _wrong_model_files(model_file):
    L, N = 2, 4
    rep = lambda sec, i, e: srsmodel.replace(model_file, L, sec, i, e)
    g1 = lambda sec, i: model_file[srsmodel.offset(L, sec, i):srsmodel.offset(L, sec, i) + 64]
    off_curve = bytearray(g1("tauG1", 3)); off_curve[63] ^= 1
    not_canonical = keyraw.be(1 + keyraw.P) + keyraw.be(2)                       # the generator with x + p: still below 2^254, flag bits 00
    assert not_canonical[0] & 0xC0 == 0
    compressed = bytearray(g1("alphaG1", 2)); compressed[0] |= 0x80
    outside = keyraw.enc_g2(keyraw.twist_point_outside_g2(), True)
    assert outside[0] & 0xC0 == 0
    # name -> (file, rule, a word the line must hold)
    return {
        "tauG1_last": (rep("tauG1", 2 * N - 2, OTHER1), 3, "tauG1"),
        "tauG1_N": (rep("tauG1", N, OTHER1), 3, "tauG1"),
        "tauG1_1": (rep("tauG1", 1, OTHER1), 3, "tauG1"),
        "tauG2_last": (rep("tauG2", N - 1, OTHER2), 4, "tauG2"),
        "tauG2_other_tau": (srsmodel.write(L, TAU, ALPHA, BETA, tau_g2=TAU + 1), 3, "tauG1"),
        "alphaG1_last": (rep("alphaG1", N - 1, OTHER1), 5, "alphaG1"),
        "betaG1_last": (rep("betaG1", N - 1, OTHER1), 6, "betaG1"),
        "betaG2_other_beta": (rep("betaG2", 0, OTHER2), 7, "betaG2"),
        "tauG1_0_not_generator": (rep("tauG1", 0, OTHER1), 2, "tauG1[0]"),
        "tauG2_0_not_generator": (rep("tauG2", 0, OTHER2), 2, "tauG2[0]"),
        "g1_off_curve": (rep("tauG1", 3, bytes(off_curve)), 1, "tauG1[3]"),
        "coordinate_not_below_p": (rep("tauG1", 0, not_canonical), 1, "tauG1[0]"),
        "g2_outside_subgroup": (rep("tauG2", 2, outside), 1, "tauG2[2]"),
        "all_zero_element": (rep("betaG1", 1, bytes(64)), 1, "betaG1[1]"),
        "all_zero_g2_element": (rep("betaG2", 0, bytes(128)), 1, "betaG2"),
        "compressed_flag": (rep("alphaG1", 2, bytes(compressed)), 1, "alphaG1[2]"),
        "truncated": (model_file[:-1], 1, "length"),
        "trailing": (model_file + b"\0", 1, "length"),
        "magic": (b"gscsrs02" + model_file[8:], 1, "magic"),
    }


WRONG_MODEL = ["tauG1_last", "tauG1_N", "tauG1_1", "tauG2_last", "tauG2_other_tau", "alphaG1_last", "betaG1_last", "betaG2_other_beta",
               "tauG1_0_not_generator", "tauG2_0_not_generator", "g1_off_curve", "coordinate_not_below_p", "g2_outside_subgroup", "all_zero_element",
               "all_zero_g2_element", "compressed_flag", "truncated", "trailing", "magic"]


@pytest.fixture(scope="module")
def wrong_model_files(model_file):
    files = _wrong_model_files(model_file)
    assert sorted(files) == sorted(WRONG_MODEL)
    return files


@pytest.mark.parametrize("name", WRONG_MODEL)
def test_a_wrong_file_is_refused_with_its_rule(gsc, capfd, wrong_model_files, name):
    srs, rule, word = wrong_model_files[name]
    ok, out = _verdict(gsc, capfd, srs)
    assert not ok, out
    lines = [l for l in out.splitlines() if l.startswith("gsc_srs_verify: ")]
    assert len(lines) == 1 and lines[0].startswith("gsc_srs_verify: rule %d:" % rule) and word in lines[0], out


# one element of the generated L = 6 file (N = 64: sums over 126 and 63 points, two blocks and one) replaced by another valid point
WRONG_L6 = {"tauG1_last": ("tauG1", 126, 3), "tauG1_N": ("tauG1", 64, 3), "tauG1_block_edge": ("tauG1", 64 + 1, 3), "tauG1_1": ("tauG1", 1, 3),
            "tauG2_last": ("tauG2", 63, 4), "tauG2_1": ("tauG2", 1, 3), "alphaG1_last": ("alphaG1", 63, 5), "alphaG1_0": ("alphaG1", 0, 5),
            "betaG1_last": ("betaG1", 63, 6), "betaG2": ("betaG2", 0, 7)}


@pytest.mark.parametrize("name", sorted(WRONG_L6))
def test_one_replaced_element_of_a_larger_file_is_refused(gsc, capfd, generated, name):
    sec, i, rule = WRONG_L6[name]
    srs = srsmodel.replace(generated[6], 6, sec, i, OTHER2 if sec.endswith("G2") else OTHER1)
    ok, out = _verdict(gsc, capfd, srs)
    assert not ok and "gsc_srs_verify: rule %d:" % rule in out, out


def test_an_element_moved_within_its_vector_is_refused(gsc, capfd, generated):
    """two neighbouring powers exchanged: every element is a valid power of the right tau, only not in its place"""
    f, L = generated[6], 6
    a, b = srsmodel.offset(L, "tauG1", 70), srsmodel.offset(L, "tauG1", 71)
    swapped = f[:a] + f[b:b + 64] + f[a:a + 64] + f[b + 64:]
    ok, out = _verdict(gsc, capfd, swapped)
    assert not ok and "rule 3" in out, out


# ---- the group transform (k_qb_stage<F> over both groups): expected values from exponent arithmetic and keyraw's multiplications ----
R = keyraw.R
ROOT_2_28 = 0x2a3c09f0a58a7e8500e0a7eb8ef62abc402d111e41112ed49bd61b6e725b19f0      # gnark-crypto's 2^28-th root of unity


def _omega(L):
    return pow(ROOT_2_28, 1 << (28 - L), R)


def _gen(group):
    return (srsmodel.G1, keyraw.g1_mul, keyraw.enc_g1, 64) if group == 0 else (srsmodel.G2, keyraw.g2_mul, keyraw.enc_g2, 128)


def _points(group, exps):
    G, mul, enc, _ = _gen(group)
    return b"".join(enc(mul(G, e % R), True) for e in exps)


def _expect(group, exps):
    """(bytes, flags) of exps[i] * G, zeros and flag 1 where the exponent is 0 mod r"""
    G, mul, enc, w = _gen(group)
    out, flags = b"", b""
    for e in exps:
        e %= R
        out += enc(mul(G, e), True) if e else bytes(w)
        flags += bytes([0 if e else 1])
    return out, flags


def _idft_exps(L, exps):
    n, w, ninv = 1 << L, _omega(L), pow(1 << L, -1, R)
    return [ninv * sum(pow(w, -j * k % n, R) * exps[k] for k in range(n)) % R for j in range(n)]


@pytest.mark.parametrize("L", [1, 2, 5])
@pytest.mark.parametrize("group", [0, 1])
def test_group_transform_on_random_exponents(gsc, group, L):
    import random
    rnd = random.Random(100 * group + L)
    exps = [rnd.randrange(1, R) for _ in range(1 << L)]
    got = gsc.debug_group_idft(group, L, _points(group, exps))
    assert got == _expect(group, _idft_exps(L, exps))


@pytest.mark.parametrize("L", [1, 2, 5])
@pytest.mark.parametrize("group", [0, 1])
def test_group_transform_of_equal_inputs_flags_infinity(gsc, group, L):
    n = 1 << L
    pts, flags = gsc.debug_group_idft(group, L, _points(group, [12345] * n))
    assert flags == bytes([0] + [1] * (n - 1))
    assert pts == _expect(group, [12345] + [0] * (n - 1))[0]


@pytest.mark.parametrize("L", [1, 2, 5])
@pytest.mark.parametrize("group", [0, 1])
def test_group_transform_of_powers_is_the_lagrange_basis(gsc, group, L):
    """inputs tau^k G: outputs L_j(tau) G with the closed form groth16_setup evaluates, L_j = (tau^n - 1) / n * w^j / (tau - w^j)"""
    n, w, tau = 1 << L, _omega(L), TAU
    lag = [(pow(tau, n, R) - 1) * pow(n, -1, R) * pow(w, j, R) * pow(tau - pow(w, j, R), -1, R) % R for j in range(n)]
    assert _idft_exps(L, [pow(tau, k, R) for k in range(n)]) == lag
    got = gsc.debug_group_idft(group, L, _points(group, [pow(tau, k, R) for k in range(n)]))
    assert got == _expect(group, lag)


# ---- the column sums (k_srs_columns.hip) against sum c * e_row on exponents ----
COL_LANES, COL_SEG_TERMS, COLS_PER_BLOCK = 64, 256, 64          # csrc/srs_columns.hpp kColLanes, kColSegTerms, kColsPerBlock
ROW_EXPS = [1, 2, 3, 5, 0x1234567, R - 1, (R + 1) // 2, 0xdeadbeefcafe]
COEFFS = [1, R - 1, (1 << 34) - 5, 0x2b3c09f0a58a7e8500e0a7eb8ef62abc402d111e41112ed49bd61b6e725b19f1 % R, 0, 2, R - 2, 3, (1 << 33) + 1]


def _columns():
    import random
    rnd = random.Random(5)
    nr, nco = len(ROW_EXPS), len(COEFFS)
    cols = [[],                                   # an empty column
            [(3, 0)], [(3, 1)], [(4, 2)], [(4, 3)], [(2, 4)],      # one term: c = 1, r - 1, 34 bits, full width, 0
            [(1, 0), (1, 0)],                     # the same row twice with c = 1: the addition must double
            [(6, 5), (6, 6)],                     # c and r - c on one row: infinity
            [(0, 0), (1, 1), (2, 0)],             # 1 - 2 + 3 = 2: meets another row's value on the way
            [(5, 4)]]                             # c = 0 alone: infinity
    for length in (COL_LANES - 1, COL_LANES, COL_LANES + 1, COL_SEG_TERMS - 1, COL_SEG_TERMS, COL_SEG_TERMS + 1, 2 * COL_SEG_TERMS + 1):
        cols.append([(rnd.randrange(nr), rnd.randrange(nco)) for _ in range(length)])
    cols += [[(rnd.randrange(nr), rnd.choice([0, 1, 5, 7]))] for _ in range(COLS_PER_BLOCK + 3 - len(cols) % COLS_PER_BLOCK)]
    assert len(cols) > COLS_PER_BLOCK and len(cols) % COLS_PER_BLOCK != 0
    return cols


@pytest.mark.parametrize("group", [0, 1])
def test_column_sums(gsc, group):
    cols = _columns()
    want_exps = [sum(COEFFS[c] * ROW_EXPS[r] for r, c in col) % R for col in cols]
    assert want_exps[0] == 0 and want_exps[5] == 0 and want_exps[7] == 0 and want_exps[9] == 0 and want_exps[6] == 4 and want_exps[8] == 2
    pts, flags = gsc.debug_column_sums(group, _points(group, ROW_EXPS), cols, COEFFS)
    want_pts, want_flags = _expect(group, want_exps)
    assert flags == want_flags
    w = 64 if group == 0 else 128
    for i in range(len(cols)):
        assert pts[w * i:w * i + w] == want_pts[w * i:w * i + w], "column %d (%d terms)" % (i, len(cols[i]))


@pytest.mark.parametrize("group", [0, 1])
def test_column_sums_refuse_a_row_at_infinity_and_bad_indices(gsc, group):
    w = 64 if group == 0 else 128
    rows = _points(group, [1, 2])
    with pytest.raises(RuntimeError):
        gsc.debug_column_sums(group, rows[:w] + bytes(w), [[(0, 0)]], [1])
    with pytest.raises(RuntimeError):
        gsc.debug_column_sums(group, rows, [[(2, 0)]], [1])          # a row past the end
    with pytest.raises(RuntimeError):
        gsc.debug_column_sums(group, rows, [[(0, 1)]], [1])          # a coefficient id past the end
    with pytest.raises(RuntimeError):
        gsc.debug_column_sums(group, rows, [[(0, 0)]], [R])          # a coefficient not below r
    assert gsc.debug_column_sums(group, rows, [[(1, 0)]], [1]) == (rows[w:], b"\0")
