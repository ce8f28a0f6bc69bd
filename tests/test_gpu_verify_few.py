"""GPU tests of the few-proof verifier kernels (k_verify_few.hip: a group of 8 lanes per proof) and of their routing:
gsc_debug_pairing_few against gsc_debug_pairing, verdicts under gsc_debug_verify_path(2) against libverify.so's Verify and against
the per-thread kernels, the batched entries on that path, the routing by GSC_VERIFY_FEW_MAX, and gsc_verify_json.
The sizes cross every boundary of the layout: one group, a wave of 8 groups, the 64-proof wave of the per-thread kernels."""
import base64
import json
import os
import random
import subprocess
import sys

import pytest

from conftest import KAT, ROOT, golden_bytes
from test_gpu_verify import G1, G2, NAMES, _cpu, _point_variants, _records, _chacha_items, _smul
from test_gpu_verify_batched import _args, naive_sum

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 8, 9, 64, 65)


class path:
    """route every verifier call inside the block: 1 one thread per proof, 2 the few-proof groups; automatic again afterwards"""
    def __init__(self, gsc, mode):
        self.g, self.mode = gsc, mode

    def __enter__(self):
        assert self.g.debug_verify_path(self.mode) == 0

    def __exit__(self, *exc):
        assert self.g.debug_verify_path(0) == 0


@pytest.fixture(scope="module")
def gv(gsc):
    vk = golden_bytes("vk.chacha20")
    assert gsc.init_verifier(0, vk) and gsc.verify_init(0, vk)
    yield gsc
    gsc.debug_verify_path(0)


def _kat_sig():
    return KAT["ciphertext"] + KAT["nonce"] + KAT["counter"].to_bytes(4, "little") + KAT["input"]


# ---- pairing hook ----
@pytest.fixture(scope="module")
def points():
    rnd = random.Random(808)
    return [(_smul(G1, rnd.getrandbits(40) + 1, False), _smul(G2, rnd.getrandbits(40) + 1, True)) for _ in range(65)]


@pytest.mark.parametrize("n", [1, 7, 8, 9, 65])
def test_pairing_hook_equals_the_per_thread_hook(gv, points, n):
    """fails without the feature: the hook symbol does not exist"""
    Ps, Qs = [p for p, _ in points[:n]], [q for _, q in points[:n]]
    # a skipped pair first in a group, last in a wave and first in the next wave
    for at, (no_p, no_q) in ((0, (True, False)), (7, (False, True)), (8, (True, True))):
        if at < n and n > 1:
            if no_p:
                Ps[at] = None
            if no_q:
                Qs[at] = None
    want = gv.debug_pairing(Ps, Qs)
    assert gv.debug_pairing(Ps, Qs, few=True) == want
    one = tuple([1] + [0] * 11)
    assert [i for i in range(n) if want[i] == one] == ([i for i in (0, 7, 8) if i < n] if n > 1 else [])
    if n == 1:      # and a single skipped pair
        for P_, Q_ in ((None, Qs[0]), (Ps[0], None), (None, None)):
            assert gv.debug_pairing([P_], [Q_], few=True) == [one]


# ---- verdicts ----
def _flip(b, pos, bit=1):
    out = bytearray(b); out[pos] ^= bit
    return bytes(out)


def _layouts(valid, invalid, n):
    """lists of n items: valid ones with invalid ones first, last, first and last of a wave of 8 groups, and isolated; every
    invalid item is used at least once"""
    if n == 1:
        return [[valid[0]]] + [[it] for it in invalid]
    spots = sorted({0, n - 1} | ({7, 8, n // 2 - 1} & set(range(n)))) if n > 2 else None
    out, pool = [], list(invalid)
    while pool:
        if n == 2:      # the invalid item first and last in turn
            a, b = pool.pop(), valid[len(pool) % len(valid)]
            out.append([a, b] if len(pool) % 2 else [b, a])
            continue
        items = [valid[i % len(valid)] for i in range(n)]
        for s in spots:
            if pool:
                items[s] = pool.pop()
        out.append(items)
    return out


def _gpu(gsc, algo, items):
    return gsc.verify_raw(algo, *_args(items))


def _check_verdicts(gsc, algo, valid, invalid, n):
    seen = 0
    for items in _layouts(valid, invalid, n):
        with path(gsc, 2):
            got = _gpu(gsc, algo, items)
            assert gsc.verify_last_path(algo) == 2
        with path(gsc, 1):
            thread = _gpu(gsc, algo, items)
            assert gsc.verify_last_path(algo) == 1
        want = _cpu(gsc, algo, items)
        assert got == want, (n, got, want)
        assert thread == want
        seen += sum(got)
    assert seen > 0


@pytest.fixture(scope="module")
def chacha_corpus():
    sig = _kat_sig()
    valid = [(bytes.fromhex(h), sig) for h in KAT["proofs"].values()]
    proof = valid[0][0]
    invalid = [(_flip(proof, 1), sig), (_flip(proof, 40), sig), (_flip(proof, 100), sig)]               # A, B, C
    invalid += [(proof, _flip(sig, pos)) for pos in (0, 70, 77, 100)]                                # ciphertext, nonce, counter, input
    invalid += [(v, sig) for v in _point_variants(proof, 0, False)]                                  # decoder: A
    invalid += [(v, sig) for v in _point_variants(proof, 32, True)[:22]]                             # decoder: B, the point outside G2 included
    invalid += [(v, sig) for v in _point_variants(proof, 96, False)[:8]]
    invalid += [(proof[:-1], sig), (proof + bytes(32), sig), (_flip(proof, 131), sig)]               # wrong proof_len, commitment count
    return valid, invalid


@pytest.mark.parametrize("n", SIZES)
def test_verdicts_chacha20(gv, chacha_corpus, n):
    valid, invalid = chacha_corpus
    _check_verdicts(gv, 0, valid, invalid, n)


@pytest.fixture(scope="module")
def aes128(gsc, aes_keys):
    r1cs, pk, vk = aes_keys["aes128"]
    assert gsc.init_algorithm(1, pk, r1cs) and gsc.init_verifier(1, vk) and gsc.verify_init(1, vk)
    rnd = random.Random(301)
    n = 12
    recs = b"".join(rnd.randbytes(32) + rnd.randbytes(12) + rnd.getrandbits(31).to_bytes(4, "little") + rnd.randbytes(64) for _ in range(n))
    ok, proofs, lens, cts = gsc.prove_raw(1, recs, n)
    assert ok == n
    valid = [(proofs[196 * k:196 * k + lens[k]], cts[64 * k:64 * k + 64] + recs[112 * k + 32:112 * k + 44] + recs[112 * k + 44:112 * k + 48][::-1] + recs[112 * k + 48:112 * k + 112])
             for k in range(n)]
    proof, sig = valid[0]
    invalid = [(_flip(proof, 140), sig), (_flip(proof, 150), sig), (_flip(proof, 170), sig), (_flip(proof, 190), sig)]      # D, PoK
    invalid.append((proof[:132] + bytes([0x40]) + bytes(31) + proof[164:], sig))                                          # D = infinity
    invalid += [(_flip(proof, 1), sig), (_flip(proof, 40), sig), (_flip(proof, 100), sig), (proof, valid[1][1]), (proof[:-1], sig)]
    return valid, invalid


@pytest.mark.parametrize("n", SIZES)
def test_verdicts_aes128(gv, aes128, n):
    valid, invalid = aes128
    _check_verdicts(gv, 1, valid, invalid, n)


# ---- batched entries ----
def test_batched_entries_on_the_few_path(gv, chacha_corpus):
    valid, invalid = chacha_corpus
    with path(gv, 2):
        for items in _layouts(valid, invalid[:10], 65) + _layouts(valid, invalid[:4], 9):
            assert gv.verify_raw_batched(0, *_args(items)) == _gpu(gv, 0, items)
            assert gv.verify_last_path(0) == 2
        for n in (3, 9):
            items = [valid[i % len(valid)] for i in range(n)]
            assert gv.verify_all(0, *_args(items)) == 1
            assert gv.verify_raw_batched(0, *_args(items)) == [1] * n
        for at in (0, 7, 8):
            items = [valid[i % len(valid)] for i in range(9)]
            items[at] = invalid[3]                                                                   # signals changed: decodes, fails the pairing
            assert gv.verify_all(0, *_args(items)) == 0
            items[at] = invalid[-2]                                                                  # too long: refused before the device
            assert gv.verify_all(0, *_args(items)) == 0


def test_final_exponentiation_of_a_large_call(gv, chacha_corpus):
    """the per-thread kernels with the batched check's final exponentiation on one group of lanes"""
    valid, invalid = chacha_corpus
    items = [valid[i % len(valid)] for i in range(64)]
    with path(gv, 1):
        assert gv.verify_all(0, *_args(items)) == 1
        assert gv.verify_last_path(0) == 1
        items[63] = invalid[3]
        assert gv.verify_all(0, *_args(items)) == 0
        assert gv.verify_raw_batched(0, *_args(items)) == [1] * 63 + [0]


def test_swapped_public_inputs_on_the_few_path(gsc_chacha, gv):
    rnd = random.Random(77)
    recs = _records(rnd, 9)
    ok, proofs, lens, cts = gsc_chacha.prove_raw(0, recs, 9)
    assert ok == 9
    items = _chacha_items(recs, proofs, lens, cts, 9)
    items[3], items[8] = (items[3][0], items[8][1]), (items[8][0], items[3][1])
    want = [1, 1, 1, 0, 1, 1, 1, 1, 0]
    with path(gv, 2):
        assert gv.verify_raw_batched(0, *_args(items)) == want
        assert _gpu(gv, 0, items) == want
        assert gv.verify_all(0, *_args(items)) == 0
        with naive_sum(gv):      # every randomizer 1: the sum the randomizers exist to defeat holds
            assert gv.verify_all(0, *_args(items)) == 1
        assert gv.verify_all(0, *_args(items)) == 0


# ---- routing ----
_CHILD = """
import sys
sys.path[:0] = [%r, %r]
import gsc_loader
from conftest import KAT, golden_bytes
g = gsc_loader.load()
out = [g.verify_last_path(0)]
assert g.verify_init(0, golden_bytes("vk.chacha20"))
out.append(g.verify_last_path(0))
sig = KAT["ciphertext"] + KAT["nonce"] + KAT["counter"].to_bytes(4, "little") + KAT["input"]
proof = bytes.fromhex(KAT["proofs"][(0, 0)])
for n in %r:
    assert g.verify_raw(0, proof.ljust(196, b"\\0") * n, [len(proof)] * n, sig * n) == [1] * n
    out.append(g.verify_last_path(0))
print(*out)
"""


def _child(few_max, sizes):
    env = dict(os.environ, GSC_ENABLE_TEST_HOOKS="1")
    env.pop("GSC_VERIFY_FEW_MAX", None)
    if few_max is not None:
        env["GSC_VERIFY_FEW_MAX"] = str(few_max)
    code = _CHILD % (ROOT, os.path.join(ROOT, "tests"), tuple(sizes))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, timeout=600, check=True).stdout.decode()
    return [int(x) for x in out.split()[-(2 + len(sizes)):]]


def test_routing_follows_gsc_verify_few_max(gv, chacha_corpus):
    valid, _ = chacha_corpus
    assert gv.debug_verify_path(0) == 0
    assert _gpu(gv, 0, valid[:1]) == [1] and gv.verify_last_path(0) == 2
    assert gv.verify_last_path(3) == -1
    # a fresh process per environment: the variable is read when the key loads
    assert _child(8, (1, 8, 9, 1)) == [-1, 0, 2, 2, 1, 2]
    assert _child(0, (1,)) == [-1, 0, 1]
    # a value that is not a number of proofs is refused and the default stands: it neither switches the path off nor forces it
    assert _child("-1", (1, 8193)) == [-1, 0, 2, 1]


def test_path_hook_refused_without_test_hooks():
    code = "import sys; sys.path.insert(0, %r); import gsc_loader; g = gsc_loader.load(); print(g.debug_verify_path(2), g.lib().gsc_debug_pairing_few(None, None, 0, None))" % ROOT
    env = {k: v for k, v in os.environ.items() if k != "GSC_ENABLE_TEST_HOOKS"}
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, timeout=600, check=True).stdout.decode()
    assert out.split()[-2:] == ["-1", "-1"]


# ---- gsc_verify_json ----
def test_verify_json(gv):
    sig, proof = _kat_sig(), bytes.fromhex(KAT["proofs"][(0, 0)])
    good = {"cipher": "chacha20", "proof": base64.b64encode(proof).decode(), "publicSignals": base64.b64encode(sig).decode()}
    cases = [json.dumps(good), json.dumps(dict(good, proof=list(proof), publicSignals=list(sig))),
             json.dumps(dict(good, publicSignals=base64.b64encode(_flip(sig, 5)).decode())),
             json.dumps(good)[:-1], "", "[" + json.dumps(good) + "]", json.dumps({k: v for k, v in good.items() if k != "proof"}),
             json.dumps({k: v for k, v in good.items() if k != "publicSignals"}), json.dumps(dict(good, cipher="chacha21")),
             json.dumps(dict(good, cipher=7)), "null", "17"]
    got = [gv.verify_json(c.encode()) for c in cases]
    assert got == [True, True] + [False] * (len(cases) - 2)
    assert got == [gv.verify(c.encode()) for c in cases]
    assert gv.verify_last_path(0) == 2
