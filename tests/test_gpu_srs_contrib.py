"""Key ceremony, first phase, on the device: k_fr_powers and the per-point ladder alone through gsc_debug_scale_powers,
seeded contributions recomputed with Python integers (tests/srscontribmodel.py, tests/srsmodel.py, tests/keyraw.py), the verdicts of
gsc_srs_verify_contribution on true steps and on wrong ones, and once the whole chain: gsc_srs_initial -> gsc_srs_contribute ->
gsc_srs_verify_contribution -> tests/srs_child.py (gsc_setup_from_srs -> gsc_setup_contribute -> InitAlgorithm -> proofs).  All comparisons
are exact.

A wrong step differs from the true one in ONE thing, so that the rule the case is about decides; a file edited after the contribution gets the
record's SHA-256(next) recomputed (nothing in the record binds that hash to the secrets).  The line the library prints names the rule."""
import ctypes
import hashlib
import json
import os
import random
import subprocess
import sys

import pytest

import devref
import keyraw
import srscontribmodel as model
import srsmodel
from keyraw import R
from conftest import ROOT

pytestmark = pytest.mark.gpu

G1_GEN = (1, 2)
SEED = bytes(range(7, 39))
SEED2 = bytes(range(100, 132))
THREADS = 64                                           # k_phase2.hip kThreads
OTHER1 = keyraw.enc_g1(keyraw.g1_mul(G1_GEN, 5), True)      # valid points that belong nowhere in the files below
OTHER2 = keyraw.enc_g2(keyraw.g2_mul(keyraw.G2_GEN, 5), True)


def toxic(seed, label):
    """gsc_setup's seeded scalar (csrc/setup.cpp toxic), which gsc_debug_srs_generate's file holds: expand_message_xmd(SHA-256) of seed | label
    padded to 32 bytes, 48 bytes out, DST "gsc-test-setup", as a big-endian integer mod r"""
    msg = seed + label.encode().ljust(32, b"\0")
    return int.from_bytes(devref.expand_message_xmd48(msg, b"gsc-test-setup"), "big") % R or 1


# ---- 1. the kernels alone ----
def _pool(group, count):
    gen, add, mul = (G1_GEN, keyraw.g1_add, keyraw.g1_mul) if group == 0 else (keyraw.G2_GEN, keyraw.g2_add, keyraw.g2_mul)
    pts, p = [], mul(gen, 0x1D3)
    for _ in range(count):
        pts.append(p); p = add(p, gen)
    return pts


_pools = {}
_ref_cache = {}


def _ref_mul(group, p, k):
    key = (group, p, k)
    if key not in _ref_cache:
        _ref_cache[key] = (keyraw.g1_mul if group == 0 else keyraw.g2_mul)(p, k)
    return _ref_cache[key]


def _layout(n, pool, gen):
    """n inputs (None = infinity): infinity first, in the middle and last, the generator, two equal points side by side; the rest cycles
    through the pool of distinct points (every output is compared)"""
    if n == 1:
        return [gen]
    pts = [pool[i % len(pool)] for i in range(n)]
    pts[0] = pts[n // 2] = pts[n - 1] = None
    pts[1] = gen
    pts[3] = pts[2]
    return pts


def _scale_powers(gsc, group, pts, x, m, first):
    enc = keyraw.enc_g1 if group == 0 else keyraw.enc_g2
    w = 64 if group == 0 else 128
    raw = b"".join(bytes(w) if p is None else enc(p, True) for p in pts)
    out, inf = gsc.debug_scale_powers(group, raw, bytes(1 if p is None else 0 for p in pts), x, m, first)
    dec = keyraw.decode_g1 if group == 0 else keyraw.decode_g2
    got = []
    for i in range(len(pts)):
        e = out[w * i:w * (i + 1)]
        if inf[i]:
            assert e == bytes(w)
            got.append(None)
        else:
            st, p = dec(e)
            assert st == 0, i
            got.append(p)
    return got


def _check_powers(gsc, group, n, x, m, first):
    assert 0 <= x < R and 0 <= m < R
    if group not in _pools:
        _pools[group] = _pool(group, 24 if group == 0 else 6)
    pts = _layout(n, _pools[group], G1_GEN if group == 0 else keyraw.G2_GEN)
    got = _scale_powers(gsc, group, pts, x, m, first)
    want = []
    for i, p in enumerate(pts):
        k = m * pow(x, first + i, R) % R
        q = None if p is None or k == 0 else _ref_mul(group, p, k)
        want.append(q)
    assert got == want


_rnd = random.Random(0x51C0)
_X = {"one": 1, "two": 2, "r-1": R - 1, "(r-1)/2": (R - 1) // 2, "random": _rnd.randrange(2, R)}
_M = {"one": 1, "r-1": R - 1, "random": _rnd.randrange(2, R)}
_EDGE = (1 << 16) - 2                                  # first + i crosses 2^16 at i = 2, inside the first block
# every n, x, m and first of the issue at least once; x = r - 1 makes the scalars alternate +-m (two reference multiplications per point of the pool)
G1_CASES = [(1, "random", "random", 0), (63, "two", "one", 0), (64, "r-1", "random", 1), (65, "(r-1)/2", "r-1", _EDGE), (130, "random", "random", _EDGE),
            (65, "one", "r-1", 0), (65, "one", "one", 1), (65, "random", "one", 1), (64, "two", "r-1", _EDGE)]
G2_CASES = [(1, "random", "random", 0), (65, "r-1", "random", _EDGE), (65, "random", "one", 1), (65, "one", "r-1", 0)]


@pytest.mark.parametrize("n,x,m,first", G1_CASES, ids=["%d-x=%s-m=%s-first=%d" % c for c in G1_CASES])
def test_scale_powers_g1(gsc, n, x, m, first):
    _check_powers(gsc, 0, n, _X[x], _M[m], first)


@pytest.mark.parametrize("n,x,m,first", G2_CASES, ids=["%d-x=%s-m=%s-first=%d" % c for c in G2_CASES])
def test_scale_powers_g2(gsc, n, x, m, first):
    _check_powers(gsc, 1, n, _X[x], _M[m], first)


def test_scale_powers_refusals(gsc, capfd):
    g = keyraw.enc_g1(G1_GEN, True)
    off_curve = g[:63] + bytes([g[63] ^ 1])
    for pts, inf, x, m, word in ((g, b"\0", R, 1, "a scalar is not below r"), (g, b"\0", 1, R, "a scalar is not below r"), (g, b"\0", (1 << 256) - 1, 1, "a scalar is not below r"),
                                 (bytes([0x80]) + g[1:], b"\0", 2, 1, "a point that is not raw and finite"), (bytes(64), b"\0", 2, 1, "a point that is not raw and finite"),
                                 (off_curve, b"\0", 2, 1, "bad point")):
        capfd.readouterr()
        with pytest.raises(RuntimeError):
            gsc.debug_scale_powers(0, pts, inf, x, m, 0)
        ctypes.CDLL(None).fflush(None)
        assert "gsc_debug_scale_powers: " + word in capfd.readouterr().out, word
    out, inf = gsc.debug_scale_powers(0, bytes(64), b"\1", 2, 1, 0)      # a flagged infinity is no refusal: infinity out
    assert out == bytes(64) and inf == b"\1"


# ---- 2. contributions ----
@pytest.fixture(scope="module")
def initial(gsc):
    return {L: gsc.srs_initial(L) for L in (2, 3, 6, 7)}


@pytest.fixture(scope="module")
def step(gsc, initial):
    """the seeded contribution to gsc_srs_initial(2): (next, record)"""
    return gsc.srs_contribute(initial[2], SEED)


@pytest.fixture(scope="module")
def scalars():
    return model.scalars(SEED)


def _verdict(gsc, capfd, prev, nxt, rec):
    capfd.readouterr()
    ok = gsc.srs_verify_contribution(prev, nxt, rec)
    ctypes.CDLL(None).fflush(None)
    return ok, capfd.readouterr().out


def test_seeded_contribution_to_the_initial_file(gsc, capfd, initial, step, scalars):
    """the file and the record, byte for byte, against two Python models: this pins the format"""
    secrets, nonces = scalars
    nxt, rec = step
    assert initial[2] == srsmodel.write(2, 1, 1, 1)
    assert nxt == srsmodel.write(2, *secrets)
    assert rec == model.record(initial[2], nxt, 2, secrets, nonces) and len(rec) == 544
    assert gsc.srs_contribute(initial[2], SEED) == step                  # the same seed: the same bytes
    ok, out = _verdict(gsc, capfd, initial[2], nxt, rec)
    assert ok and "rule" not in out, out


def test_a_second_contribution_gives_the_products(gsc, capfd, step, scalars):
    s1, (s2, k2) = scalars[0], model.scalars(SEED2)
    nxt2, rec2 = gsc.srs_contribute(step[0], SEED2)
    assert nxt2 == srsmodel.write(2, *[a * b % R for a, b in zip(s1, s2)])
    assert rec2 == model.record(step[0], nxt2, 2, s2, k2)
    ok, out = _verdict(gsc, capfd, step[0], nxt2, rec2)
    assert ok and "rule" not in out, out
    ok, out = _verdict(gsc, capfd, step[0], nxt2, step[1])               # link 1's record over link 2's files
    assert not ok and "gsc_srs_verify_contribution: rule 2:" in out, out


def test_contribution_to_a_generated_file(gsc, capfd):
    """a file of unknown-looking scalars (the generator hook's, for a seed) contributed to: the file of the products, every element"""
    L = 5
    prev = gsc.debug_srs_generate(L, SEED)
    s2, k2 = model.scalars(SEED2)
    nxt, rec = gsc.srs_contribute(prev, SEED2)
    want = srsmodel.write(L, *[toxic(SEED, n) * s % R for n, s in zip(("tau", "alpha", "beta"), s2)])
    assert nxt == want
    assert rec == model.record(prev, nxt, L, s2, k2)
    ok, out = _verdict(gsc, capfd, prev, nxt, rec)
    assert ok and "rule" not in out, out


@pytest.mark.parametrize("L", [6, 7])
def test_ragged_last_blocks(gsc, capfd, initial, step, scalars, L):
    N = 1 << L
    assert (4 * N - 1) % THREADS != 0 and (N + 1) % THREADS != 0 and (2 * N - 1) % THREADS != 0 and N % THREADS == 0
    (tau, alpha, beta), _ = scalars
    nxt, rec = gsc.srs_contribute(initial[L], SEED)
    assert len(nxt) == srsmodel.layout(L)["bytes"]
    capfd.readouterr()
    assert gsc.srs_verify(nxt)
    ok, out = _verdict(gsc, capfd, initial[L], nxt, rec)
    assert ok and "rule" not in out, out
    g1 = lambda k: keyraw.enc_g1(keyraw.g1_mul(G1_GEN, k % R), True)
    g2 = lambda k: keyraw.enc_g2(keyraw.g2_mul(keyraw.G2_GEN, k % R), True)
    for i in (1, 64, 65, 2 * N - 2):
        assert model.element(nxt, L, "tauG1", i) == g1(pow(tau, i, R)), i
    assert model.element(nxt, L, "tauG2", N - 1) == g2(pow(tau, N - 1, R))
    assert model.element(nxt, L, "alphaG1", N - 1) == g1(alpha * pow(tau, N - 1, R))
    assert model.element(nxt, L, "betaG1", N - 1) == g1(beta * pow(tau, N - 1, R))
    assert model.element(nxt, L, "betaG2") == g2(beta)
    for sec in model.SECTIONS:                                           # the same seed underlies every size
        w, a, b = (128 if sec.endswith("G2") else 64) * model.count(2, sec), srsmodel.offset(2, sec), srsmodel.offset(L, sec)
        assert step[0][a:a + w] == nxt[b:b + w], sec


def test_unseeded_contributions_differ_and_verify(gsc, capfd, initial):
    a, b = gsc.srs_contribute(initial[2]), gsc.srs_contribute(initial[2])
    assert a[0] != b[0] and a[1] != b[1] and model.element(a[0], 2, "tauG1", 1) != model.element(b[0], 2, "tauG1", 1)
    for nxt, rec in (a, b):
        ok, out = _verdict(gsc, capfd, initial[2], nxt, rec)
        assert ok and "rule" not in out, out


# ---- 3. wrong steps ----
def _rehash(rec, nxt):
    return rec[:32] + hashlib.sha256(nxt).digest() + rec[64:]


def _with(rec, s, part, value):
    """the record with new_s (part 0), T_s (1) or z_s (2) replaced"""
    o = model.proof_offset(s) + (0, 64, 128)[part]
    return rec[:o] + value + rec[o + len(value):]


def _proof(rec, s):
    o = model.proof_offset(s)
    return rec[o:o + 64], rec[o + 64:o + 128], int.from_bytes(rec[o + 128:o + 160], "big")


def _wrong_steps(gsc, initial, step):
    L = 2
    prev, (nxt, rec) = initial[L], step
    other_prev = gsc.srs_contribute(prev, SEED2)[0]
    unrelated = srsmodel.write(L, 0x1234567, 0xabcdef01, 0x31415926)
    unrelated_rec = _rehash(rec, unrelated)
    for s, (sec, i) in enumerate(model.BASES):
        unrelated_rec = _with(unrelated_rec, s, 0, model.element(unrelated, L, sec, i))
    T0 = keyraw.decode_g1(_proof(rec, 0)[1])[1]
    off_curve = bytearray(model.element(nxt, L, "tauG1", 3)); off_curve[63] ^= 1

    def edited(sec, i, e):
        f = srsmodel.replace(nxt, L, sec, i, e)
        return prev, f, _rehash(rec, f)

    # name -> (prev, next, record, what the one line starts with after "gsc_srs_verify_contribution: ")
    cases = {
        "different_L": (initial[3], nxt, rec, "rule 1:"),
        "truncated_prev": (prev[:-1], nxt, rec, "rule 1: prev:"),
        "replayed_over_another_prev": (other_prev, nxt, rec, "rule 2:"),
        "hash_prev_flipped": (prev, nxt, bytes([rec[0] ^ 1]) + rec[1:], "rule 2:"),
        "hash_next_flipped": (prev, nxt, rec[:32] + bytes([rec[32] ^ 1]) + rec[33:], "rule 2:"),
        "T_tau_doubled": (prev, nxt, _with(rec, 0, 1, keyraw.enc_g1(keyraw.g1_add(T0, T0), True)), "rule 4: tau:"),
        "T_alpha_all_zero": (prev, nxt, _with(rec, 1, 1, bytes(64)), "rule 4: alpha:"),
        "z_beta_not_below_r": (prev, nxt, _with(rec, 2, 2, R.to_bytes(32, "big")), "rule 4: beta:"),
        "unrelated_powers_file": (prev, unrelated, unrelated_rec, "rule 4: tau:"),
        "tauG1_replaced": edited("tauG1", 3, OTHER1) + ("rule 5: next: rule 3:",),
        "tauG2_replaced": edited("tauG2", 2, OTHER2) + ("rule 5: next: rule 4:",),
        "alphaG1_replaced": edited("alphaG1", 2, OTHER1) + ("rule 5: next: rule 5:",),
        "betaG2_replaced": edited("betaG2", 0, OTHER2) + ("rule 5: next: rule 7:",),
        "g1_off_curve": edited("tauG1", 3, bytes(off_curve)) + ("rule 5: next: rule 1: srs: tauG1[3]",),
    }
    for s, name in enumerate(("tau", "alpha", "beta")):
        cases["record_%s_replaced" % name] = (prev, nxt, _with(rec, s, 0, OTHER1), "rule 3:")
        cases["z_%s_plus_1" % name] = (prev, nxt, _with(rec, s, 2, ((_proof(rec, s)[2] + 1) % R).to_bytes(32, "big")), "rule 4: %s:" % name)
    return cases


WRONG = ["different_L", "truncated_prev", "replayed_over_another_prev", "hash_prev_flipped", "hash_next_flipped", "record_tau_replaced", "record_alpha_replaced",
         "record_beta_replaced", "z_tau_plus_1", "z_alpha_plus_1", "z_beta_plus_1", "T_tau_doubled", "T_alpha_all_zero", "z_beta_not_below_r",
         "unrelated_powers_file", "tauG1_replaced", "tauG2_replaced", "alphaG1_replaced", "betaG2_replaced", "g1_off_curve"]


@pytest.fixture(scope="module")
def wrong_steps(gsc, initial, step):
    cases = _wrong_steps(gsc, initial, step)
    assert sorted(cases) == sorted(WRONG)
    return cases


@pytest.mark.parametrize("name", WRONG)
def test_a_wrong_step_is_refused_with_its_rule(gsc, capfd, wrong_steps, name):
    prev, nxt, rec, start = wrong_steps[name]
    ok, out = _verdict(gsc, capfd, prev, nxt, rec)
    assert not ok, out
    lines = [l for l in out.splitlines() if l.startswith("gsc_srs_verify_contribution: ")]
    assert len(lines) == 1 and lines[0].startswith("gsc_srs_verify_contribution: " + start), out


def test_the_unrelated_file_is_a_powers_file(gsc, wrong_steps):
    """the rule 4 case above is refused for its proofs alone: its next file passes gsc_srs_verify"""
    assert gsc.srs_verify(wrong_steps["unrelated_powers_file"][1])


# ---- 4. the whole chain, once ----
SMALL_ENGINE = {"GSC_MAX_BATCH": "128", "GSC_Z_TABLE_GB": "4", "GSC_W_TABLE_GB": "4", "GSC_ENABLE_TEST_HOOKS": "1"}


def test_the_chain_from_the_initial_file_to_proofs(gsc, capfd, tmp_path):
    """gsc_srs_initial(15) -> one unseeded contribution -> its check -> tests/srs_child.py in a process of its own on that file:
    gsc_setup_from_srs -> gsc_setup_contribute -> InitAlgorithm -> ChaCha20 proofs, accepted under the new vk, refused with a flipped signal and
    under the delta = 1 vk.  No test hook makes the file."""
    L, n = 15, 8
    start = gsc.srs_initial(L)
    assert len(start) == srsmodel.layout(L)["bytes"]
    nxt, rec = gsc.srs_contribute(start)
    ok, out = _verdict(gsc, capfd, start, nxt, rec)
    assert ok and "rule" not in out, out
    open(os.path.join(str(tmp_path), "srs"), "wb").write(nxt)
    env = {k: v for k, v in os.environ.items() if not k.startswith("GSC_")}
    env.update(SMALL_ENGINE)
    facts = os.path.join(str(tmp_path), "facts.json")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "srs_child.py"), ROOT, "0", str(n), facts, str(tmp_path)], env=env, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0 and "CHILD-OK" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
    f = json.load(open(facts))
    assert f["srs_ok"] and f["step_ok"], f
    assert f["lens"] == [164] * n and f["new"] == [True] * n and f["flipped"] is False and f["old"] == [False] * n, f
