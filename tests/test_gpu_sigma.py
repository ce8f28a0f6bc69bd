"""The sigma ceremony on the device: gsc_setup_contribute_sigma on synthetic pairs (tests/sigmamodel.py) with every
rewritten byte recomputed with Python integers, the verdicts of gsc_setup_verify_sigma_contribution on the true link and on fifteen wrong
ones, gsc_pedersen_verify, sigma and delta links interleaved on the AES-128 pair with the final keys at work in a child process
(tests/phase2_child.py), and gsc_setup_verify_from_srs on production pairs of both kinds of circuit.  All comparisons are exact.

A file edited after the contribution gets the record's SHA-256(pk_next) recomputed (nothing in the record binds that hash to the secret), so
that the rule the case is about decides, not the hash; the line the library prints names the rule."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import pytest

import keyraw
import sigmamodel
from keyraw import P, R
from conftest import ROOT, golden_bytes

pytestmark = pytest.mark.gpu

SEED = bytes(range(11, 43))
SEED2 = bytes(range(90, 122))
SEED3 = bytes(range(150, 182))
SIZES = (1, 63, 64, 65, 257)                                         # one each side of a wave and of the random combination's block
_pairs = {}


def pair(n):
    if n not in _pairs:
        _pairs[n] = sigmamodel.build(n)
    return _pairs[n]


def _secs(sections, key):
    return {name: el for name, _, _, el in sections(key)}


def _elem(sections, key, name, i):
    o, sz = _secs(sections, key)[name][i]
    return key[o:o + sz]


# ---- 1. synthetic pairs: every rewritten byte ----
@pytest.mark.parametrize("n", SIZES)
def test_contribution_to_a_synthetic_pair(gsc, n):
    p = pair(n)
    seed = bytes([n & 0xFF]) + SEED[1:]
    x, k = sigmamodel.seeded(seed)
    pk2, vk2, rec = gsc.setup_contribute_sigma(p.pk, p.vk, seed)
    want = sigmamodel.contribution(p, x, k)
    # every BasisExpSigma' element, GSigmaNeg', the record's 224 bytes, everything else unchanged, the rewritten points compressed
    so, sn = _secs(keyraw.pk_sections, p.pk), _secs(keyraw.pk_sections, pk2)
    assert len(sn["ped.sigma"]) == n and all(sz == 32 for _, sz in sn["ped.sigma"])
    for j in range(n):
        assert _elem(keyraw.pk_sections, pk2, "ped.sigma", j) == keyraw.enc_g1(sigmamodel.g1(x * p.sigma * p.b[j]), False), j
    assert pk2[:sn["ped.sigma"][0][0]] == p.pk[:so["ped.sigma"][0][0]]
    assert _elem(keyraw.vk_sections, vk2, "ped.gsn", 0) == keyraw.enc_g2(sigmamodel.g2(-x * p.sigma * p.g), False) and vk2[:-64] == p.vk[:-64]
    assert len(rec) == 224 and rec == want[2]
    assert (pk2, vk2) == want[:2]
    assert gsc.setup_verify_sigma_contribution(p.pk, p.vk, pk2, vk2, rec)
    assert gsc.pedersen_verify(p.pk, p.vk) and gsc.pedersen_verify(pk2, vk2)


def test_the_same_seed_gives_the_same_bytes_and_raw_input_is_written_compressed(gsc, link):
    p, step = link
    assert gsc.setup_contribute_sigma(p.pk, p.vk, SEED) == step
    # the same pair with some elements raw: the rewritten ones come back compressed, the others stay raw
    mpk = keyraw.rewrite_pk(p.pk, lambda name, i: (name == "ped.sigma" and i % 3 == 0) or (name, i) == ("ped.basis", 1))
    mvk = keyraw.rewrite_vk(p.vk, lambda name, i: name in ("ped.g", "ped.gsn"))
    pk2, vk2, rec = gsc.setup_contribute_sigma(mpk, mvk, SEED)
    x, k = sigmamodel.seeded(SEED)
    want_pk, want_vk = sigmamodel.scaled(p, x)
    assert pk2 == keyraw.rewrite_pk(want_pk, lambda name, i: (name, i) == ("ped.basis", 1))
    assert vk2 == keyraw.rewrite_vk(want_vk, lambda name, i: name == "ped.g")
    # the same new element and T; the challenge binds the hash of the other file
    assert rec[64:192] == step[2][64:192] and rec[:32] == hashlib.sha256(mpk).digest() and rec[32:64] == hashlib.sha256(pk2).digest()
    base = keyraw.enc_g1(sigmamodel.g1(p.sigma * p.b[p.j0]), True)
    assert int.from_bytes(rec[192:], "big") == (k + sigmamodel.challenge(rec[:32], base, rec[64:128], rec[128:192]) * x) % R
    assert gsc.setup_verify_sigma_contribution(mpk, mvk, pk2, vk2, rec)


FORCED = [("one", 1), ("two", 2), ("r-1", R - 1), ("(r-1)/2", (R - 1) // 2), ("bit253", 1 << 253)]


@pytest.mark.parametrize("name,x", FORCED, ids=[nm for nm, _ in FORCED])
def test_forced_scalars_through_the_ladder(gsc, name, x):
    """the scalar classes no seed reaches, through the launcher a contribution uses (gsc_debug_scale_points), on the n = 65 pair's elements"""
    p = pair(65)
    pts = [sigmamodel.g1(p.sigma * b) for b in p.b]
    out, inf = gsc.debug_scale_points(0, b"".join(keyraw.enc_g1(q, True) for q in pts), bytes(1 if q is None else 0 for q in pts), x)
    want_pk, want_vk = sigmamodel.scaled(p, x)
    for j in range(65):
        e = out[64 * j:64 * j + 64]
        assert bool(inf[j]) == (p.b[j] == 0)
        got = None if inf[j] else keyraw.decode_g1(e)[1]
        assert keyraw.enc_g1(got, False) == _elem(keyraw.pk_sections, want_pk, "ped.sigma", j), j
    gsn = sigmamodel.g2(-p.sigma * p.g)
    out, inf = gsc.debug_scale_points(1, keyraw.enc_g2(gsn, True), bytes(1), x)
    assert not inf[0] and keyraw.enc_g2(keyraw.decode_g2(out)[1], False) == _elem(keyraw.vk_sections, want_vk, "ped.gsn", 0)


def test_unseeded_contributions_differ_and_verify(gsc, link):
    p, _ = link
    a, b = gsc.setup_contribute_sigma(p.pk, p.vk), gsc.setup_contribute_sigma(p.pk, p.vk)
    assert a[2][64:128] != b[2][64:128] and a[0] != b[0] and a[1] != b[1]
    assert gsc.setup_verify_sigma_contribution(p.pk, p.vk, *a) and gsc.setup_verify_sigma_contribution(p.pk, p.vk, *b)


# ---- 2. verdicts on the n = 65 pair ----
@pytest.fixture(scope="module")
def link(gsc):
    p = pair(65)
    return p, gsc.setup_contribute_sigma(p.pk, p.vk, SEED)


@pytest.fixture(scope="module")
def golden_pair():
    return golden_bytes("pk.chacha20"), golden_bytes("vk.chacha20")


def _verdict(gsc, capfd, prev, nxt, rec):
    capfd.readouterr()
    ok = gsc.setup_verify_sigma_contribution(prev[0], prev[1], nxt[0], nxt[1], rec)
    ctypes.CDLL(None).fflush(None)
    return ok, capfd.readouterr().out


def _call(capfd, f, *args):
    capfd.readouterr()
    ok = f(*args)
    ctypes.CDLL(None).fflush(None)
    return ok, capfd.readouterr().out


def _rehash(rec, pk_next):
    return rec[:32] + hashlib.sha256(pk_next).digest() + rec[64:]


def _neg_g1(e):
    st, p = keyraw.decode_g1(e)
    assert st == 0
    return keyraw.enc_g1((p[0], -p[1] % P), False)


def _swap(pk, name, i, j):
    a, b = _elem(keyraw.pk_sections, pk, name, i), _elem(keyraw.pk_sections, pk, name, j)
    assert a != b
    return keyraw.rewrite_pk(pk, replace={(name, i): b, (name, j): a})


@pytest.fixture(scope="module")
def wrong_links(gsc, link, golden_pair):
    p, (pk2, vk2, rec) = link
    pk, vk = p.pk, p.vk
    z = int.from_bytes(rec[192:], "big")
    T = keyraw.decode_g1(rec[128:192])[1]
    assert p.b[0] == 0 and p.b[4] and p.b[5] and p.b[4] != p.b[5] and p.j0 == 1
    swapped = _swap(pk2, "ped.sigma", 4, 5)
    negated = keyraw.rewrite_pk(pk2, replace={("ped.sigma", 5): _neg_g1(_elem(keyraw.pk_sections, pk2, "ped.sigma", 5))})
    old_gsn = keyraw.rewrite_vk(vk2, replace={("ped.gsn", 0): _elem(keyraw.vk_sections, vk, "ped.gsn", 0)})
    assert old_gsn == vk
    y_pk, y_vk = sigmamodel.scaled(p, 0xC0FFEE)
    basis = keyraw.rewrite_pk(pk2, replace={("ped.basis", 5): keyraw.enc_g1(sigmamodel.g1(999), False)})
    g_changed = keyraw.rewrite_vk(vk2, replace={("ped.g", 0): keyraw.enc_g2(sigmamodel.g2(7), False)})
    b_raw = keyraw.rewrite_pk(pk2, choose=lambda name, i: name == "g2.B" and i == 0)
    moved = _swap(pk2, "ped.sigma", 0, 4)                              # the infinity of element 0 now sits at 4
    assert len(b_raw) == len(pk2) + 64
    delta_rec = gsc.setup_contribute(pk, vk, SEED)[2]
    prev, nxt = (pk, vk), (pk2, vk2)
    # name -> (prev, next, record, the rules that may refuse it)
    return {
        "z_plus_1": (prev, nxt, rec[:192] + ((z + 1) % R).to_bytes(32, "big"), (4,)),
        "T_doubled": (prev, nxt, rec[:128] + keyraw.enc_g1(keyraw.g1_add(T, T), True) + rec[192:], (4,)),
        "hash_flipped": (prev, nxt, bytes([rec[0] ^ 1]) + rec[1:], (3,)),
        "sigma_swapped": (prev, (swapped, vk2), _rehash(rec, swapped), (5,)),
        "sigma_negated": (prev, (negated, vk2), _rehash(rec, negated), (5,)),
        "old_gsn": (prev, (pk2, old_gsn), rec, (5,)),
        "scaled_by_another": (prev, (y_pk, y_vk), _rehash(rec, y_pk), (3, 4)),
        "basis_changed": (prev, (basis, vk2), _rehash(rec, basis), (2,)),
        "g_changed": (prev, (pk2, g_changed), rec, (2,)),
        "B2_reencoded_raw": (prev, (b_raw, vk2), _rehash(rec, b_raw), (2,)),
        "infinity_moved": (prev, (moved, vk2), _rehash(rec, moved), (3,)),
        "next_is_prev": (prev, prev, rec, (3,)),
        "exchanged": (nxt, prev, rec, (3,)),
        "delta_record": (prev, nxt, delta_rec, (3, 4)),
        "no_commitment": (golden_pair, golden_pair, rec, (1,)),
    }


WRONG = ["z_plus_1", "T_doubled", "hash_flipped", "sigma_swapped", "sigma_negated", "old_gsn", "scaled_by_another", "basis_changed", "g_changed",
         "B2_reencoded_raw", "infinity_moved", "next_is_prev", "exchanged", "delta_record", "no_commitment"]


def test_the_true_link_is_accepted(gsc, capfd, link):
    p, (pk2, vk2, rec) = link
    ok, out = _verdict(gsc, capfd, (p.pk, p.vk), (pk2, vk2), rec)
    assert ok and "rule" not in out, out


@pytest.mark.parametrize("name", WRONG)
def test_a_wrong_link_is_refused(gsc, capfd, wrong_links, name):
    prev, nxt, rec, rules = wrong_links[name]
    ok, out = _verdict(gsc, capfd, prev, nxt, rec)
    assert not ok
    assert any("gsc_setup_verify_sigma_contribution: rule %d:" % r in out for r in rules), out


# ---- 3. gsc_pedersen_verify ----
@pytest.fixture(scope="module")
def other_key(gsc, aes_keys):
    return gsc.setup(aes_keys["aes128"][0], bytes([77] * 32))


def _refused(capfd, f, args, rule, who):
    ok, out = _call(capfd, f, *args)
    assert not ok and "%s: rule %d:" % (who, rule) in out, out


def test_pedersen_verify(gsc, capfd, aes_keys, other_key, golden_pair):
    _, pk, vk = aes_keys["aes128"]
    who = "gsc_pedersen_verify"
    ok, out = _call(capfd, gsc.pedersen_verify, pk, vk)
    assert ok and "rule" not in out, out
    _refused(capfd, gsc.pedersen_verify, (_swap(pk, "ped.sigma", 6, 7), vk), 2, who)
    other_gsn = _elem(keyraw.vk_sections, other_key[1], "ped.gsn", 0)
    assert other_gsn != _elem(keyraw.vk_sections, vk, "ped.gsn", 0)
    _refused(capfd, gsc.pedersen_verify, (pk, keyraw.rewrite_vk(vk, replace={("ped.gsn", 0): other_gsn})), 2, who)
    outside = keyraw.enc_g2(keyraw.twist_point_outside_g2(), False)
    _refused(capfd, gsc.pedersen_verify, (pk, keyraw.rewrite_vk(vk, replace={("ped.g", 0): outside})), 1, who)
    _refused(capfd, gsc.pedersen_verify, golden_pair, 1, who)


def test_the_randomizers_are_used(gsc, capfd, aes_keys):
    """two exchanged elements leave the plain sum as it was: with every rho = 1 the pair passes, with fresh rho it does not"""
    _, pk, vk = aes_keys["aes128"]
    bad = _swap(pk, "ped.sigma", 6, 7)
    try:
        assert gsc.debug_verify_randomizers(all_ones=True) == 0
        ok, out = _call(capfd, gsc.pedersen_verify, bad, vk)
        assert ok, out
    finally:
        gsc.debug_verify_randomizers()
    _refused(capfd, gsc.pedersen_verify, (bad, vk), 2, "gsc_pedersen_verify")


# ---- 4. sigma and delta links interleave ----
SMALL_ENGINE = {"GSC_MAX_BATCH": "64", "GSC_WINDOW_Z": "8", "GSC_W_TABLE_GB": "8", "GSC_ENABLE_TEST_HOOKS": "1"}
_state = {"dead": None}


def _child(tmp, algo, keys, old_vk, n):
    """tests/phase2_child.py in a process of its own: InitAlgorithm(pk'), gsc_verify_init(vk'), n proofs, their verdicts under vk' (the library's
    and the oracle's) and under the old vk.  After a child that aborted or ran into its time limit no further child is started."""
    if _state["dead"]:
        pytest.fail("not started: the child of '%s' aborted or ran into its time limit" % _state["dead"])
    for name, b in (("pk.new", keys[0]), ("vk.new", keys[1]), ("vk.old", old_vk)):
        open(os.path.join(str(tmp), name), "wb").write(b)
    env = {k: v for k, v in os.environ.items() if not k.startswith("GSC_")}
    env.update(SMALL_ENGINE)
    out = os.path.join(str(tmp), "facts.json")
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "phase2_child.py"), ROOT, str(algo), str(n), out, str(tmp)], env=env, capture_output=True,
                           text=True, timeout=300)
    except subprocess.TimeoutExpired:
        _state["dead"] = str(tmp)
        raise
    if p.returncode < 0 or p.returncode in (124, 134, 137, 139):
        _state["dead"] = str(tmp)
    assert p.returncode == 0 and "CHILD-OK" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
    return json.load(open(out))


def test_sigma_and_delta_links_interleave(gsc, capfd, aes_keys, tmp_path):
    _, pk0, vk0 = aes_keys["aes128"]
    pk1, vk1, rec1 = gsc.setup_contribute(pk0, vk0, SEED)                # delta
    pk2, vk2, rec2 = gsc.setup_contribute_sigma(pk1, vk1, SEED2)         # sigma
    pk3, vk3, rec3 = gsc.setup_contribute(pk2, vk2, SEED3)               # delta
    delta_links = (((pk0, vk0), (pk1, vk1), rec1), ((pk2, vk2), (pk3, vk3), rec3))
    sigma_link = ((pk1, vk1), (pk2, vk2), rec2)
    # the sigma link copied delta, Z and K; the delta links copied the commitment key
    s1, s2, s3 = (_secs(keyraw.pk_sections, k) for k in (pk1, pk2, pk3))
    for nm in ("g1.delta", "g1.Z", "g1.K", "g2.delta", "ped.basis"):
        assert [pk1[o:o + sz] for o, sz in s1[nm]] == [pk2[o:o + sz] for o, sz in s2[nm]], nm
    assert [pk1[o:o + sz] for o, sz in s1["ped.sigma"]] != [pk2[o:o + sz] for o, sz in s2["ped.sigma"]]
    assert [pk2[o:o + sz] for o, sz in s2["ped.sigma"]] == [pk3[o:o + sz] for o, sz in s3["ped.sigma"]] and vk2[-128:] == vk3[-128:]
    x, _ = sigmamodel.seeded(SEED2)
    for j in (0, 1, len(s1["ped.sigma"]) - 1):
        o, sz = s1["ped.sigma"][j]
        st, q = keyraw.decode_g1(pk1[o:o + sz])
        assert _elem(keyraw.pk_sections, pk2, "ped.sigma", j) == keyraw.enc_g1(None if q is None else keyraw.g1_mul(q, x), False), j
    # each link is accepted by its own verifier and refused under rule 2 by the other's
    for prev, nxt, rec in delta_links:
        ok, out = _call(capfd, gsc.setup_verify_contribution, prev[0], prev[1], nxt[0], nxt[1], rec)
        assert ok, out
        ok, out = _verdict(gsc, capfd, prev, nxt, rec)
        assert not ok and "gsc_setup_verify_sigma_contribution: rule 2:" in out, out
    prev, nxt, rec = sigma_link
    ok, out = _verdict(gsc, capfd, prev, nxt, rec)
    assert ok and "rule" not in out, out
    ok, out = _call(capfd, gsc.setup_verify_contribution, prev[0], prev[1], nxt[0], nxt[1], rec)
    assert not ok and "gsc_setup_verify_contribution: rule 2:" in out, out
    assert gsc.pedersen_verify(pk3, vk3)
    # the final pair at work; the vk from before the sigma link refuses its proofs
    f = _child(tmp_path, 1, (pk3, vk3), vk1, 2)
    assert f["lens"] == [196] * 2 and f["new"] == [1] * 2 and f["oracle_new"] == [True] * 2 and f["old"] == [0] * 2, f


# ---- 5. gsc_setup_verify_from_srs ----
SRS_SEED = bytes([61] * 32)


@pytest.fixture(scope="module")
def srs_files(gsc):
    return {L: gsc.debug_srs_generate(L, SRS_SEED) for L in (15, 17)}


@pytest.fixture(scope="module")
def aes_production(gsc, aes_keys, srs_files):
    r1cs = aes_keys["aes128"][0]
    return r1cs, gsc.setup_from_srs(r1cs, srs_files[17]), gsc.setup_from_srs(r1cs, srs_files[17])


def test_verify_from_srs_chacha(gsc, capfd, srs_files):
    r1cs = golden_bytes("r1cs.chacha20")
    pk, vk = gsc.setup_from_srs(r1cs, srs_files[15])
    ok, out = _call(capfd, gsc.setup_verify_from_srs, r1cs, srs_files[15], pk, vk)
    assert ok and "rule" not in out, out
    last = bytes([vk[-1] ^ 1])                                         # without a commitment the whole of both files is compared
    _refused(capfd, gsc.setup_verify_from_srs, (r1cs, srs_files[15], pk, vk[:-1] + last), 1, "gsc_setup_verify_from_srs")


def test_verify_from_srs_aes128(gsc, capfd, aes_production, srs_files):
    r1cs, (pk_a, vk_a), (pk_b, vk_b) = aes_production
    who = "gsc_setup_verify_from_srs"
    srs = srs_files[17]
    # two production runs differ exactly in BasisExpSigma, G and GSigmaNeg, and both are accepted
    sa, sb = _secs(keyraw.pk_sections, pk_a), _secs(keyraw.pk_sections, pk_b)
    assert sa == sb and pk_a[:sa["ped.sigma"][0][0]] == pk_b[:sb["ped.sigma"][0][0]] and vk_a[:-128] == vk_b[:-128]
    assert all(pk_a[o:o + sz] != pk_b[o:o + sz] or pk_a[o] & 0xC0 == 0x40 for o, sz in sa["ped.sigma"])
    assert vk_a[-128:-64] != vk_b[-128:-64] and vk_a[-64:] != vk_b[-64:]
    for pk, vk in ((pk_a, vk_a), (pk_b, vk_b)):
        ok, out = _call(capfd, gsc.setup_verify_from_srs, r1cs, srs, pk, vk)
        assert ok and "rule" not in out, out
    dpk, dvk, _ = gsc.setup_contribute(pk_a, vk_a, SEED)
    _refused(capfd, gsc.setup_verify_from_srs, (r1cs, srs, dpk, dvk), 1, who)
    at = sa["g1.A"][0][0] + 31
    _refused(capfd, gsc.setup_verify_from_srs, (r1cs, srs, pk_a[:at] + bytes([pk_a[at] ^ 1]) + pk_a[at + 1:], vk_a), 1, who)
    _refused(capfd, gsc.setup_verify_from_srs, (r1cs, srs, pk_a, vk_a[:-64] + vk_b[-64:]), 2, who)


def test_verify_from_srs_refuses_a_tampered_file(gsc, capfd, aes_production, srs_files):
    r1cs, (pk_a, vk_a), _ = aes_production
    srs = bytearray(srs_files[17])
    at = 12 + 64 * 5                                                   # tauG1[5] <- tauG1[6]: a point of the curve, not the power
    srs[at:at + 64] = srs[at + 64:at + 128]
    capfd.readouterr()
    with pytest.raises(RuntimeError, match="-2"):
        gsc.setup_verify_from_srs(r1cs, bytes(srs), pk_a, vk_a)
    ctypes.CDLL(None).fflush(None)
    assert "gsc_setup_verify_from_srs: the powers file is refused" in capfd.readouterr().out
