"""Key ceremony, second phase, on the device: k_scale_points alone through gsc_debug_scale_points, a contribution to the
golden ChaCha20 pair recomputed with Python integers (tests/keyraw.py), the verdicts of gsc_setup_verify_contribution on the true step and on
twelve wrong ones, a chain of two contributions, AES-128, and — in child processes of their own (tests/phase2_child.py: the session's
fixtures keep their keys) — the new keys at work: InitAlgorithm, gsc_verify_init, proofs accepted under the new vk and refused under the old.
All comparisons are exact.

A file edited after the contribution gets the record's SHA-256(pk_next) recomputed (nothing in the record binds that hash to the secret), so
that the rule the case is about decides, not the hash; the line the library prints names the rule."""
import ctypes
import hashlib
import json
import os
import random
import subprocess
import sys

import pytest

import keyraw
from keyraw import P, R
from conftest import ROOT, golden_bytes

pytestmark = pytest.mark.gpu

G1_GEN = (1, 2)
SEED = bytes(range(7, 39))
SEED2 = bytes(range(100, 132))


# ---- 1. the kernel alone ----
def _points_g1(count):
    pts, p = [], keyraw.g1_mul(G1_GEN, 0x1D3)
    for _ in range(count):
        pts.append(p); p = keyraw.g1_add(p, G1_GEN)
    return pts


DISTINCT_G1 = 24
_ref_cache = {}


def _ref_mul(group, p, k):
    key = (group, p, k)
    if key not in _ref_cache:
        _ref_cache[key] = (keyraw.g1_mul if group == 0 else keyraw.g2_mul)(p, k)
    return _ref_cache[key]


def _layout(n, pool, gen):
    """n inputs (None = infinity): infinity first, in the middle and last, the generator, two equal points side by side; the rest cycles
    through the pool of distinct points (every output is compared; the pool keeps the Python reference's time down)"""
    if n == 1:
        return [gen]
    pts = [pool[i % len(pool)] for i in range(n)]
    pts[0] = pts[n // 2] = pts[n - 1] = None
    pts[1] = gen
    pts[3] = pts[2]
    return pts


def _scale(gsc, group, pts, k):
    enc = keyraw.enc_g1 if group == 0 else keyraw.enc_g2
    w = 64 if group == 0 else 128
    raw = b"".join(bytes(w) if p is None else enc(p, True) for p in pts)
    out, inf = gsc.debug_scale_points(group, raw, bytes(1 if p is None else 0 for p in pts), k)
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


_rnd = random.Random(0x9A5E2)
G1_CASES = [(n, "random%d" % n, _rnd.randrange(1, R)) for n in (1, 63, 64, 65, 257)] + \
           [(65, "one", 1), (65, "two", 2), (65, "r-1", R - 1), (65, "(r-1)/2", (R - 1) // 2), (65, "bit253", 1 << 253), (65, "low64", (1 << 64) - 1)]


@pytest.mark.parametrize("n,name,k", G1_CASES, ids=["%d-%s" % (n, nm) for n, nm, _ in G1_CASES])
def test_scale_points_g1(gsc, n, name, k):
    assert k < R
    pts = _layout(n, _points_g1(DISTINCT_G1), G1_GEN)
    got = _scale(gsc, 0, pts, k)
    assert got == [None if p is None else _ref_mul(0, p, k) for p in pts]


G2_CASES = [(1, "r-1", R - 1), (1, "random", _rnd.randrange(1, R)), (65, "r-1", R - 1), (65, "random", _rnd.randrange(1, R))]


@pytest.mark.parametrize("n,name,k", G2_CASES, ids=["%d-%s" % (n, nm) for n, nm, _ in G2_CASES])
def test_scale_points_g2(gsc, n, name, k):
    pool, p = [], keyraw.g2_mul(keyraw.G2_GEN, 0x2B7)
    for _ in range(6):                                   # with the generator: 7 distinct points
        pool.append(p); p = keyraw.g2_add(p, keyraw.G2_GEN)
    pts = _layout(n, pool, keyraw.G2_GEN)
    got = _scale(gsc, 1, pts, k)
    assert got == [None if q is None else _ref_mul(1, q, k) for q in pts]


# ---- 2. a contribution to the golden pair ----
def _scalar(label, seed):
    return int.from_bytes(hashlib.sha256(label + seed).digest(), "big") % R


def _elems(secs, key):
    return {name: [key[o:o + sz] for o, sz in el] for name, _, _, el in secs}


REWRITTEN_PK = ("g1.delta", "g1.Z", "g1.K", "g2.delta")
REWRITTEN_VK = ("g1.delta", "g2.delta")


def _untouched_equal(old, new, sections, rewritten):
    so, sn = sections(old), sections(new)
    assert [(nm, g, c, len(el)) for nm, g, c, el in so] == [(nm, g, c, len(el)) for nm, g, c, el in sn]      # the same sets and counts
    # every byte outside the rewritten elements: the header, the counts, the wire masks, every other point
    def outside(key, secs):
        cut = sorted((o, sz) for nm, _, _, el in secs if nm in rewritten for o, sz in el)
        out, at = [], 0
        for o, sz in cut:
            out.append(key[at:o]); at = o + sz
        return out + [key[at:]]
    assert outside(old, so) == outside(new, sn)
    eo, en = _elems(so, old), _elems(sn, new)
    for nm in eo:
        if nm not in rewritten:
            assert eo[nm] == en[nm], nm
    return eo, en


@pytest.fixture(scope="module")
def golden_pair():
    return golden_bytes("pk.chacha20"), golden_bytes("vk.chacha20")


@pytest.fixture(scope="module")
def step(gsc, golden_pair):
    pk, vk = golden_pair
    return gsc.setup_contribute(pk, vk, SEED)


def _check_contribution(pk, vk, pk2, vk2, rec, seed, positions=8):
    x, k = _scalar(b"gsc-phase2-x", seed), _scalar(b"gsc-phase2-k", seed)
    xi = pow(x, -1, R)
    eo, en = _untouched_equal(pk, pk2, keyraw.pk_sections, REWRITTEN_PK)
    vo, vn = _untouched_equal(vk, vk2, keyraw.vk_sections, REWRITTEN_VK)
    d1 = keyraw.decode_g1(eo["g1.delta"][0])[1]; d2 = keyraw.decode_g2(eo["g2.delta"][0])[1]
    nd1, nd2 = keyraw.g1_mul(d1, x), keyraw.g2_mul(d2, x)
    assert en["g1.delta"][0] == keyraw.enc_g1(nd1, False) == vn["g1.delta"][0]
    assert en["g2.delta"][0] == keyraw.enc_g2(nd2, False) == vn["g2.delta"][0]
    assert keyraw.decode_g1(vo["g1.delta"][0])[1] == d1
    for nm in ("g1.Z", "g1.K"):
        n = len(eo[nm])
        infinite = [i for i, e in enumerate(eo[nm]) if e[0] & 0xC0 == 0x40 or e == bytes(64)]      # infinity in the input stays infinity
        rnd = random.Random(n)
        where = sorted(set([0, n - 1] + [rnd.randrange(n) for _ in range(positions - 2)] + infinite[:4]))
        assert len(where) >= min(positions, n)
        for i in where:
            st, p = keyraw.decode_g1(eo[nm][i])
            assert st in (0, 2)
            want = keyraw.enc_g1(None if p is None else keyraw.g1_mul(p, xi), False)
            assert en[nm][i] == want, (nm, i)
        assert all(len(e) == 32 for e in en[nm])                       # written compressed
    T = keyraw.g1_mul(d1, k)
    h_prev = hashlib.sha256(pk).digest()
    raw = lambda p: keyraw.enc_g1(p, True)
    c = int.from_bytes(hashlib.sha256(b"gsc-phase2-v1" + h_prev + raw(d1) + raw(nd1) + raw(T)).digest()[:31], "big")
    assert rec == h_prev + hashlib.sha256(pk2).digest() + raw(nd1) + raw(T) + ((k + c * x) % R).to_bytes(32, "big")
    assert len(rec) == 224


def test_contribution_on_the_golden_pair(gsc, golden_pair, step):
    pk, vk = golden_pair
    pk2, vk2, rec = step
    assert len(pk2) == len(pk) and len(vk2) == len(vk)
    _check_contribution(pk, vk, pk2, vk2, rec, SEED)
    assert gsc.setup_contribute(pk, vk, SEED) == step                  # the same seed: the same bytes


def test_unseeded_contributions_differ(gsc, golden_pair):
    pk, vk = golden_pair
    a, b = gsc.setup_contribute(pk, vk), gsc.setup_contribute(pk, vk)
    da, db = a[2][64:128], b[2][64:128]
    assert da != db and keyraw.decode_g1(da)[0] == 0 and keyraw.decode_g1(db)[0] == 0
    assert gsc.setup_verify_contribution(pk, vk, a[0], a[1], a[2])


# ---- 4. verdicts ----
def _verdict(gsc, capfd, prev, nxt, rec):
    capfd.readouterr()
    ok = gsc.setup_verify_contribution(prev[0], prev[1], nxt[0], nxt[1], rec)
    ctypes.CDLL(None).fflush(None)
    return ok, capfd.readouterr().out


def _rehash(rec, pk_next):
    return rec[:32] + hashlib.sha256(pk_next).digest() + rec[64:]


def _pk_elem(pk, name, i):
    secs = {nm: el for nm, _, _, el in keyraw.pk_sections(pk)}
    o, sz = secs[name][i]
    return pk[o:o + sz]


def _neg_g1(e):
    st, p = keyraw.decode_g1(e)
    assert st == 0
    return keyraw.enc_g1((p[0], -p[1] % P), False)


def _wrong_steps(golden_pair, step):
    pk, vk = golden_pair
    pk2, vk2, rec = step
    z = int.from_bytes(rec[192:], "big")
    T = keyraw.decode_g1(rec[128:192])[1]
    swap = lambda name: keyraw.rewrite_pk(pk2, replace={(name, 0): _pk_elem(pk2, name, 1), (name, 1): _pk_elem(pk2, name, 0)})
    neg_z = keyraw.rewrite_pk(pk2, replace={("g1.Z", 5): _neg_g1(_pk_elem(pk2, "g1.Z", 5))})
    old_d2 = keyraw.rewrite_pk(pk2, replace={("g2.delta", 0): _pk_elem(pk, "g2.delta", 0)})
    vk_old_d1 = keyraw.rewrite_vk(vk2, replace={("g1.delta", 0): _pk_elem(pk, "g1.delta", 0)})
    a_at = keyraw.pk_sections(pk2)[3][3][0][0]
    a_byte = pk2[:a_at + 31] + bytes([pk2[a_at + 31] ^ 1]) + pk2[a_at + 32:]
    b_raw = keyraw.rewrite_pk(pk2, choose=lambda name, i: name == "g2.B" and i == 0)
    assert swap("g1.Z") != pk2 and swap("g1.K") != pk2 and len(b_raw) == len(pk2) + 64
    prev, nxt = (pk, vk), (pk2, vk2)
    # name -> (prev, next, record, the rules that may refuse it)
    return {
        "z_plus_1": (prev, nxt, rec[:192] + ((z + 1) % R).to_bytes(32, "big"), (5,)),
        "T_doubled": (prev, nxt, rec[:128] + keyraw.enc_g1(keyraw.g1_add(T, T), True) + rec[192:], (5,)),
        "hash_flipped": (prev, nxt, bytes([rec[0] ^ 1]) + rec[1:], (4,)),
        "Z_swapped": (prev, (swap("g1.Z"), vk2), _rehash(rec, swap("g1.Z")), (7,)),
        "K_swapped": (prev, (swap("g1.K"), vk2), _rehash(rec, swap("g1.K")), (7,)),
        "Z_negated": (prev, (neg_z, vk2), _rehash(rec, neg_z), (7,)),
        "pk_old_delta2": (prev, (old_d2, vk2), _rehash(rec, old_d2), (3,)),
        "vk_old_delta1": (prev, (pk2, vk_old_d1), rec, (3,)),
        "A_byte": (prev, (a_byte, vk2), _rehash(rec, a_byte), (1, 2)),      # another x: no point of the curve (1) or another point (2)
        "B2_reencoded_raw": (prev, (b_raw, vk2), _rehash(rec, b_raw), (2,)),
        "next_is_prev": (prev, prev, rec, (4,)),
        "exchanged": (nxt, prev, rec, (4,)),
    }


WRONG = ["z_plus_1", "T_doubled", "hash_flipped", "Z_swapped", "K_swapped", "Z_negated", "pk_old_delta2", "vk_old_delta1", "A_byte", "B2_reencoded_raw",
         "next_is_prev", "exchanged"]


@pytest.fixture(scope="module")
def wrong_steps(golden_pair, step):
    return _wrong_steps(golden_pair, step)


def test_the_true_step_is_accepted(gsc, capfd, golden_pair, step):
    ok, out = _verdict(gsc, capfd, golden_pair, step[:2], step[2])
    assert ok and "rule" not in out, out


@pytest.mark.parametrize("name", WRONG)
def test_a_wrong_step_is_refused(gsc, capfd, wrong_steps, name):
    prev, nxt, rec, rules = wrong_steps[name]
    ok, out = _verdict(gsc, capfd, prev, nxt, rec)
    assert not ok
    assert any("gsc_setup_verify_contribution: rule %d:" % r in out for r in rules), out


# ---- children: the new keys at work ----
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


def test_the_new_key_proves_and_the_old_vk_rejects(golden_pair, step, tmp_path):
    f = _child(tmp_path, 0, step[:2], golden_pair[1], 4)
    assert f["lens"] == [164] * 4 and f["new"] == [1] * 4 and f["oracle_new"] == [True] * 4 and f["old"] == [0] * 4, f


# ---- 5. a chain ----
def test_chain_of_two_contributions(gsc, capfd, golden_pair, step, tmp_path):
    pk, vk = golden_pair
    pk1, vk1, rec1 = step
    pk2, vk2, rec2 = gsc.setup_contribute(pk1, vk1, SEED2)
    assert _verdict(gsc, capfd, (pk, vk), (pk1, vk1), rec1)[0]
    assert _verdict(gsc, capfd, (pk1, vk1), (pk2, vk2), rec2)[0]
    ok, out = _verdict(gsc, capfd, (pk, vk), (pk1, vk1), rec2)            # link 2's record against link 1's keys
    assert not ok and "rule 4" in out, out
    f = _child(tmp_path, 0, (pk2, vk2), vk1, 4)
    assert f["new"] == [1] * 4 and f["oracle_new"] == [True] * 4 and f["old"] == [0] * 4, f


# ---- 6. AES-128: 196-byte proofs, a commitment key, a K set without the committed wires ----
def test_aes128_contribution(gsc, capfd, aes_keys, tmp_path):
    r1cs, pk, vk = aes_keys["aes128"]
    pk2, vk2, rec = gsc.setup_contribute(pk, vk, SEED)
    eo, en = _untouched_equal(pk, pk2, keyraw.pk_sections, REWRITTEN_PK)
    assert len(eo["ped.basis"]) > 0 and eo["ped.basis"] == en["ped.basis"] and eo["ped.sigma"] == en["ped.sigma"]
    vo, vn = _untouched_equal(vk, vk2, keyraw.vk_sections, REWRITTEN_VK)
    assert vo["ped.g"] == vn["ped.g"] and vo["ped.gsn"] == vn["ped.gsn"]
    _check_contribution(pk, vk, pk2, vk2, rec, SEED, positions=4)
    ok, out = _verdict(gsc, capfd, (pk, vk), (pk2, vk2), rec)
    assert ok, out
    f = _child(tmp_path, 1, (pk2, vk2), vk, 2)
    assert f["lens"] == [196] * 2 and f["new"] == [1] * 2 and f["oracle_new"] == [True] * 2 and f["old"] == [0] * 2, f
