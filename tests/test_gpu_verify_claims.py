"""GPU tests of the claim-wise batched check in libprove.so (gsc_verify_claims / VerifyClaims, k_verify_claims.hip): a claim's verdict is
the AND of gsc_verify_raw's verdicts over its items, every claim is decided by an equation of its own (a bad proof costs its own claim
only), and the random rho_i / t_i reject inside a claim what a naive sum (every randomizer 1, gsc_debug_verify_randomizers) accepts."""
import ctypes
import itertools
import os
import random
import subprocess
import sys
import threading

import pytest

from conftest import AES, ROOT
from test_gpu_verify import P, _add, _corpus, _gpu, _records, _smul, aes_valid, chacha_batch, gv  # noqa: F401  (fixtures)
from test_gpu_verify_batched import _args, _g1_decode, _json_items, _one_bad, _with_point, naive_sum

pytestmark = pytest.mark.gpu


def _cut(n, sizes):
    """claim ends over n items: claim sizes cycle through `sizes`, the last claim takes what is left"""
    ends, at = [], 0
    for s in itertools.cycle(sizes):
        if at >= n:
            return ends
        at = min(n, at + s)
        ends.append(at)


def _claims(gsc, algo, items, ends):
    return gsc.verify_claims(algo, *_args(items), ends)


def _and(verdicts, ends):
    return [int(all(verdicts[a:b])) for a, b in zip([0] + ends[:-1], ends)]


def _expect_only(gsc, algo, items, ends, bad_claims):
    got = _claims(gsc, algo, items, ends)
    assert [j for j, v in enumerate(got) if not v] == sorted(bad_claims)


# ---- 1. valid claims ----
def test_valid_claims_are_accepted(gv, chacha_batch, aes_valid):
    ends = _cut(300, [1, 2, 7, 8, 9, 0, 63, 64, 65])
    assert 0 in [b - a for a, b in zip([0] + ends[:-1], ends)] and ends[-1] == 300
    assert _claims(gv, 0, chacha_batch[:300], ends) == [1] * len(ends)
    for name, (algo, _, _) in AES.items():
        valid = aes_valid[name]
        ends = _cut(len(valid), [1, 2, 7, 8, 9, 0])
        assert _claims(gv, algo, valid, ends) == [1] * len(ends)
    assert _claims(gv, 0, [], []) == []
    assert gv.lib().gsc_verify_claims(0, b"", None, b"", 0, None, 0, None) == 0
    assert _claims(gv, 0, [], [0, 0]) == [1, 1]                            # empty claims hold


# ---- 2. agreement with gsc_verify_raw ----
def _corpus_claims(gsc, algo, items, seed):
    rnd = random.Random(seed)
    ends, at = [], 0
    while at < len(items):
        at = min(len(items), at + rnd.randint(1, 4))
        ends.append(at)
    want = _and(_gpu(gsc, algo, items), ends)
    assert 0 < sum(want) < len(want)                                      # neither outcome is vacuous
    return items, ends, want


@pytest.fixture(scope="module")
def chacha_corpus(gv, chacha_batch):
    return _corpus_claims(gv, 0, _corpus(random.Random(2000), chacha_batch[:260], False), 31)


def test_agreement_corpus_chacha(gv, chacha_corpus):
    items, ends, want = chacha_corpus
    assert _claims(gv, 0, items, ends) == want


@pytest.mark.parametrize("name", list(AES))
def test_agreement_corpus_aes(gv, aes_valid, name):
    algo = AES[name][0]
    items, ends, want = _corpus_claims(gv, algo, _corpus(random.Random(algo), aes_valid[name], True), 32 + algo)
    assert _claims(gv, algo, items, ends) == want


# ---- 3. one bad proof costs its own claim only ----
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_one_bad_proof(gv, chacha_batch, where):
    items = chacha_batch[:65 * 7]
    ends = _cut(len(items), [65])
    k = 3 * 65 + {"first": 0, "middle": 32, "last": 64}[where]
    _expect_only(gv, 0, _one_bad(items, k), ends, [3])


# ---- 4. undecodable items ----
def test_undecodable_items_beside_valid_ones(gv, chacha_batch):
    items = list(chacha_batch[:300])
    for k in range(0, 300, 7):
        p, s = items[k]
        items[k] = (p[:-1], s) if k % 2 else (bytes([0x40]) + bytes(30) + b"\x01" + p[32:], s)      # short / A: infinity flag with a stray bit
    ends = _cut(300, [3])
    want = _and(_gpu(gv, 0, items), ends)
    assert want == [int(not any(k % 7 == 0 for k in range(a, b))) for a, b in zip([0] + ends[:-1], ends)] and 0 < sum(want) < len(want)
    assert _claims(gv, 0, items, ends) == want


# ---- 5. attacks that the naive sum accepts ----
def _naive(gsc, algo, vk, items, ends, tmp_path):
    """the claims' verdicts with every randomizer 1; in a child process when the session's library was loaded without test hooks"""
    if gsc.debug_verify_randomizers(None, False) == 0:
        with naive_sum(gsc):
            return _claims(gsc, algo, items, ends)
    slots, lens, sigs = _args(items)
    path = str(tmp_path / "naive.bin")
    words = [algo, len(vk), len(lens), len(ends)] + lens + ends
    open(path, "wb").write(b"".join(v.to_bytes(4, "little") for v in words) + vk + slots + sigs)
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_verify_claims as t; t._naive_child(%r)"
            % (ROOT, os.path.join(ROOT, "tests"), path))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, GSC_ENABLE_TEST_HOOKS="1"), capture_output=True, timeout=600, check=True)
    return [int(c) for c in out.stdout.decode().split()[-1]]


def _naive_child(path):
    import gsc_loader
    g = gsc_loader.load()
    b = open(path, "rb").read()
    algo, nvk, n, m = (int.from_bytes(b[4 * i:4 * i + 4], "little") for i in range(4))
    words = [int.from_bytes(b[16 + 4 * i:20 + 4 * i], "little") for i in range(n + m)]
    at = 16 + 4 * (n + m)
    assert g.verify_init(algo, b[at:at + nvk])
    at += nvk
    assert g.debug_verify_randomizers(None, True) == 0
    print("".join(str(v) for v in g.verify_claims(algo, b[at:at + 196 * n], words[:n], b[at + 196 * n:], words[n:])))


def _chacha_vk():
    from conftest import golden_bytes
    return golden_bytes("vk.chacha20")


def test_swapped_public_signals_inside_a_claim(gv, chacha_batch, tmp_path):
    items, ends = list(chacha_batch[:64]), _cut(64, [8])
    items[3], items[5] = (items[3][0], items[5][1]), (items[5][0], items[3][1])
    assert _and(_gpu(gv, 0, items), ends) == [0] + [1] * 7
    assert _claims(gv, 0, items, ends) == [0] + [1] * 7
    assert _naive(gv, 0, _chacha_vk(), items, ends, tmp_path) == [1] * 8


def test_swapped_public_signals_across_two_claims(gv, chacha_batch, tmp_path):
    items, ends = list(chacha_batch[:64]), _cut(64, [8])
    items[3], items[40] = (items[3][0], items[40][1]), (items[40][0], items[3][1])
    want = [0, 1, 1, 1, 1, 0, 1, 1]
    assert _and(_gpu(gv, 0, items), ends) == want
    assert _claims(gv, 0, items, ends) == want
    assert _naive(gv, 0, _chacha_vk(), items, ends, tmp_path) == want          # the claims do not share an equation


def test_c_plus_p_and_c_minus_p_inside_a_claim(gv, chacha_batch, tmp_path):
    items, ends = list(chacha_batch[:64]), _cut(64, [8])
    pt = _smul((1, 2), 0xdeadbeefcafe, False)
    for k, sign in ((9, 1), (14, -1)):
        p, s = items[k]
        q = pt if sign > 0 else (pt[0], P - pt[1])
        items[k] = (_with_point(p, 96, _add(_g1_decode(p[96:128]), q, False)), s)
    want = [1, 0, 1, 1, 1, 1, 1, 1]
    assert _and(_gpu(gv, 0, items), ends) == want
    assert _claims(gv, 0, items, ends) == want
    assert _naive(gv, 0, _chacha_vk(), items, ends, tmp_path) == [1] * 8


@pytest.mark.parametrize("field", ["pok", "d"])
def test_aes_swapped_commitment_fields_inside_a_claim(gv, aes_valid, aes_keys, tmp_path, field):
    algo = AES["aes128"][0]
    items, ends = list(aes_valid["aes128"][:64]), _cut(64, [8])
    lo, hi = (164, 196) if field == "pok" else (132, 164)
    (p2, s2), (p5, s5) = items[2], items[5]
    assert p2[lo:hi] != p5[lo:hi]
    items[2] = (p2[:lo] + p5[lo:hi] + p2[hi:], s2)
    items[5] = (p5[:lo] + p2[lo:hi] + p5[hi:], s5)
    assert _and(_gpu(gv, algo, items), ends) == [0] + [1] * 7
    assert _claims(gv, algo, items, ends) == [0] + [1] * 7
    assert _naive(gv, algo, aes_keys["aes128"][2], items, ends, tmp_path) == [1] * 8


# ---- 6. both routes ----
def test_both_routes_give_the_same_verdicts(gv, chacha_corpus):
    items, ends, want = chacha_corpus
    try:
        for mode in (1, 2):
            assert gv.debug_verify_path(mode) == 0
            assert _claims(gv, 0, items, ends) == want
            assert gv.verify_last_path(0) == mode
    finally:
        assert gv.debug_verify_path(0) == 0


# ---- 7. a claim across a chunk boundary ----
def test_claim_across_a_chunk_boundary_of_the_few_proof_route(gv, chacha_batch):
    n = 8192 + 100
    base = [chacha_batch[i % len(chacha_batch)] for i in range(n)]          # valid proofs, repeated
    ends = _cut(8150, [50]) + [8250, n]
    across = ends.index(8250)
    try:
        assert gv.debug_verify_path(2) == 0
        assert _claims(gv, 0, base, ends) == [1] * len(ends)
        for k in (8191, 8192, 8249):
            _expect_only(gv, 0, _one_bad(base, k), ends, [across])
        assert gv.verify_last_path(0) == 2
    finally:
        assert gv.debug_verify_path(0) == 0


def test_claim_across_a_chunk_boundary_of_the_per_thread_route(gv, chacha_batch):
    n = 65536 + 1000
    base = [chacha_batch[i % len(chacha_batch)] for i in range(n)]
    ends = _cut(n, [100])                                                   # claim 655 covers [65 500, 65 600)
    assert ends[655] == 65600
    for k in (65535, 65536):
        _expect_only(gv, 0, _one_bad(base, k), ends, [655])
    assert gv.verify_last_path(0) == 1


# ---- 8. one long claim beside short ones ----
def test_one_long_claim_beside_short_ones(gv, chacha_batch):
    items = chacha_batch[:1000]
    ends = [700] + list(range(701, 1001))
    assert _claims(gv, 0, items, ends) == [1] * 301
    _expect_only(gv, 0, _one_bad(items, 699), ends, [0])


# ---- 9. arguments ----
def test_bad_claim_ends_are_refused_before_anything_is_written(gv, chacha_batch):
    slots, lens, sigs = _args(chacha_batch[:10])
    lens_arr = (ctypes.c_uint32 * 10)(*lens)
    for ends in ([4, 3, 10], [4, 9], [4, 11], []):
        out = ctypes.create_string_buffer(b"\xaa" * 8, 8)
        arr = (ctypes.c_uint64 * max(1, len(ends)))(*ends)
        assert gv.lib().gsc_verify_claims(0, slots, lens_arr, sigs, 10, arr, len(ends), out) == -3
        assert out.raw == b"\xaa" * 8
    with pytest.raises(RuntimeError, match="-3"):
        gv.verify_claims(0, slots, lens, sigs, [4, 3, 10])


def test_no_key_loaded():
    code = ("import sys; sys.path.insert(0, %r); import gsc_loader; g = gsc_loader.load()\n"
            "try:\n    g.verify_claims(0, bytes(196), [164], bytes(144), [1])\nexcept RuntimeError as e:\n    print(e)" % ROOT)
    env = {k: v for k, v in os.environ.items() if k != "GSC_VK_DIR"}
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, timeout=300, check=True).stdout.decode()
    assert "(-1)" in out.splitlines()[-1]


# ---- 10. VerifyClaims ----
def test_verify_claims_json(gv, chacha_batch, aes_valid):
    items = _json_items(chacha_batch, aes_valid)                            # the three ciphers in turn
    claims = [items[0:5], items[5:6], items[6:12]]
    assert gv.verify_claims_json(claims) == [True, True, True]
    bad = [[dict(it) for it in cl] for cl in claims]
    p = bytearray(bad[1][0]["proof"])
    p[100] ^= 1
    bad[1][0]["proof"] = list(p)
    assert gv.verify_claims_json(bad) == [True, False, True]
    odd = [claims[0], {}, claims[1], [], [1], claims[2], [items[0], {"cipher": "chacha21", "proof": [], "publicSignals": []}], claims[0]]
    assert gv.verify_claims_json(odd) == [True, False, True, False, False, True, False, True]
    assert gv.verify_claims_json(b"[]") == []
    assert set(gv.verify_claims_json(b"[1,")) == {"Offset"}
    assert gv.verify_claims_json(b'{"cipher":"chacha20"}') == "VerifyClaims expects a JSON array"


# ---- 11. the randomizer hook governs this path too ----
def test_fixed_seed_gives_the_same_verdicts_twice(gv, chacha_corpus):
    items, ends, want = chacha_corpus
    try:
        assert gv.debug_verify_randomizers(bytes(range(32))) == 0
        a = _claims(gv, 0, items, ends)
        b = _claims(gv, 0, items, ends)
    finally:
        assert gv.debug_verify_randomizers(None, False) == 0
    assert a == b == want


# ---- 12. beside a prover ----
def test_concurrent_claim_and_plain_verifiers_beside_a_prover(gsc_chacha, gv, chacha_batch):
    recs = _records(random.Random(19), 2048)
    ends = _cut(1000, [7])
    done = {}

    def prove():
        done["prove"] = gsc_chacha.prove_raw(0, recs, 2048)

    def verify(t):
        items = chacha_batch[t * 1000:(t + 1) * 1000]
        items = [(p, s if i % 30 else chacha_batch[0][1]) for i, (p, s) in enumerate(items)]
        per_item = [int(i % 30 != 0 or t * 1000 + i == 0) for i in range(len(items))]
        if t % 2 == 0:
            done[t] = (_claims(gv, 0, items, ends), _and(per_item, ends))
        else:
            done[t] = (_gpu(gv, 0, items), per_item)

    th = [threading.Thread(target=prove)] + [threading.Thread(target=verify, args=(t,)) for t in range(4)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert done["prove"][0] == 2048
    for t in range(4):
        assert done[t][0] == done[t][1] and 0 < sum(done[t][0]) < len(done[t][0])
