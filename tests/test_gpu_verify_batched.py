"""GPU tests of the batched Groth16 check in libprove.so (gsc_verify_raw_batched / gsc_verify_all / VerifyAll, k_verify_batch.hip):
its verdicts equal gsc_verify_raw's element for element, and the random rho_i / t_i reject the sets of invalid proofs that a naive
sum (every randomizer 1, gsc_debug_verify_randomizers) accepts."""
import base64
import os
import random
import subprocess
import sys
import threading

import pytest

from conftest import AES, ROOT
from test_gpu_verify import P, _corpus, _gpu, _records, _smul, _add, aes_valid, chacha_batch, gv  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def _args(items):
    slots = b"".join(p[:196].ljust(196, b"\0") for p, _ in items)
    lens = [len(p) if len(p) <= 196 else 0xFFFFFFFF for p, _ in items]
    return slots, lens, b"".join(s for _, s in items)


def _batched(gsc, algo, items):
    return gsc.verify_raw_batched(algo, *_args(items))


def _all(gsc, algo, items):
    return gsc.verify_all(algo, *_args(items))


class naive_sum:
    """every randomizer 1 inside the block; the OS CSPRNG again afterwards"""
    def __init__(self, gsc):
        self.g = gsc

    def __enter__(self):
        assert self.g.debug_verify_randomizers(None, True) == 0

    def __exit__(self, *exc):
        assert self.g.debug_verify_randomizers(None, False) == 0


# ---- G1 points in gnark's compressed form ----
def _g1_decode(b):
    assert b[0] & 0x80
    x = int.from_bytes(bytes([b[0] & 0x3F]) + b[1:32], "big")
    y = pow((x ** 3 + 3) % P, (P + 1) // 4, P)
    assert y * y % P == (x ** 3 + 3) % P
    if (b[0] & 0xC0 == 0xC0) != (y > (P - 1) // 2):
        y = P - y
    return (x, y)


def _g1_encode(pt):
    x, y = pt
    enc = bytearray(x.to_bytes(32, "big"))
    enc[0] |= 0xC0 if y > (P - 1) // 2 else 0x80
    return bytes(enc)


def _with_point(proof, off, pt):
    return proof[:off] + _g1_encode(pt) + proof[off + 32:]


# ---- valid sets ----
def test_valid_sets_are_accepted(gv, chacha_batch, aes_valid):
    assert _all(gv, 0, chacha_batch) == 1
    assert _batched(gv, 0, chacha_batch) == [1] * len(chacha_batch)
    for name, (algo, _, _) in AES.items():
        valid = aes_valid[name]
        assert _all(gv, algo, valid) == 1
        assert _batched(gv, algo, valid) == [1] * len(valid)
    assert _all(gv, 0, []) == 1 and _batched(gv, 0, []) == []


def test_agreement_corpus_chacha(gv, chacha_batch):
    items = _corpus(random.Random(2000), chacha_batch[:260], False)
    got = _batched(gv, 0, items)
    assert sum(got) > 0 and got == _gpu(gv, 0, items)
    assert _all(gv, 0, items) == 0


@pytest.mark.parametrize("name", list(AES))
def test_agreement_corpus_aes(gv, aes_valid, name):
    algo = AES[name][0]
    items = _corpus(random.Random(algo), aes_valid[name], True)
    got = _batched(gv, algo, items)
    assert sum(got) > 0 and got == _gpu(gv, algo, items)


def test_undecodable_items_beside_valid_ones(gv, chacha_batch):
    """the batch check holds over the items that decode; the rest are rejected as gsc_verify_raw rejects them"""
    items = list(chacha_batch[:300])
    for k in range(0, 300, 7):
        p, s = items[k]
        items[k] = (p[:-1], s) if k % 2 else (bytes([0x40]) + bytes(30) + b"\x01" + p[32:], s)      # short / A: infinity flag with a stray bit
    want = _gpu(gv, 0, items)
    assert 0 < sum(want) < len(items)
    assert _batched(gv, 0, items) == want
    assert _all(gv, 0, items) == 0


# ---- one bad proof ----
def _one_bad(items, k):
    out = list(items)
    j = (k + 1) % len(items)
    out[k] = (items[k][0], items[j][1])                                  # signals of another statement
    return out


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_one_bad_proof(gv, chacha_batch, where):
    n = len(chacha_batch)
    k = {"first": 0, "middle": n // 2, "last": n - 1}[where]
    items = _one_bad(chacha_batch, k)
    assert _all(gv, 0, items) == 0
    want = [1] * n; want[k] = 0
    assert _batched(gv, 0, items) == want


def test_one_bad_proof_across_a_chunk_boundary(gv, chacha_batch):
    n = 65536 + 1000
    base = [chacha_batch[i % len(chacha_batch)] for i in range(n)]                  # valid proofs, repeated
    assert _all(gv, 0, base) == 1
    for k in (65535, 65536, n - 1):
        items = _one_bad(base, k)
        assert _all(gv, 0, items) == 0
        want = [1] * n; want[k] = 0
        assert _batched(gv, 0, items) == want


# ---- attacks that the naive sum accepts ----
def _expect_rejected(gsc, algo, items, bad):
    want = [0 if i in bad else 1 for i in range(len(items))]
    assert _batched(gsc, algo, items) == want
    assert _all(gsc, algo, items) == 0
    assert gsc.verify_raw(algo, *_args(items)) == want


def test_swapped_public_signals(gv, chacha_batch, tmp_path):
    items = list(chacha_batch[:64])
    items[3], items[40] = (items[3][0], items[40][1]), (items[40][0], items[3][1])
    _expect_rejected(gv, 0, items, {3, 40})
    if gv.debug_verify_randomizers(None, False) == 0:
        with naive_sum(gv):
            assert _all(gv, 0, items) == 1
        return
    # the session's library was loaded without test hooks: the control runs in a child process that has them
    slots, lens, sigs = _args(items)
    path = str(tmp_path / "swapped.bin")
    open(path, "wb").write(len(lens).to_bytes(4, "little") + b"".join(v.to_bytes(4, "little") for v in lens) + slots + sigs)
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_verify_batched as t; sys.exit(t._naive_child(%r))"
            % (ROOT, os.path.join(ROOT, "tests"), path))
    assert subprocess.run([sys.executable, "-c", code], env=dict(os.environ, GSC_ENABLE_TEST_HOOKS="1"), timeout=600).returncode == 0


def _naive_child(path):
    import gsc_loader
    from conftest import golden_bytes
    g = gsc_loader.load()
    assert g.verify_init(0, golden_bytes("vk.chacha20"))
    b = open(path, "rb").read()
    n = int.from_bytes(b[:4], "little")
    lens = [int.from_bytes(b[4 + 4 * i:8 + 4 * i], "little") for i in range(n)]
    slots, sigs = b[4 + 4 * n:4 + 4 * n + 196 * n], b[4 + 4 * n + 196 * n:]
    assert g.debug_verify_randomizers(None, True) == 0
    return 0 if g.verify_all(0, slots, lens, sigs) == 1 else 1


def test_c_plus_p_and_c_minus_p(gv, chacha_batch):
    items = list(chacha_batch[:64])
    pt = _smul((1, 2), 0xdeadbeefcafe, False)
    for k, sign in ((5, 1), (50, -1)):
        p, s = items[k]
        q = pt if sign > 0 else (pt[0], P - pt[1])
        items[k] = (_with_point(p, 96, _add(_g1_decode(p[96:128]), q, False)), s)
    _expect_rejected(gv, 0, items, {5, 50})
    with naive_sum(gv):
        assert _all(gv, 0, items) == 1


@pytest.mark.parametrize("field", ["pok", "d"])
def test_aes_swapped_commitment_fields(gv, aes_valid, field):
    algo = AES["aes128"][0]
    items = list(aes_valid["aes128"][:64])
    lo, hi = (164, 196) if field == "pok" else (132, 164)
    (p2, s2), (p9, s9) = items[2], items[9]
    assert p2[lo:hi] != p9[lo:hi]
    items[2] = (p2[:lo] + p9[lo:hi] + p2[hi:], s2)
    items[9] = (p9[:lo] + p2[lo:hi] + p9[hi:], s9)
    _expect_rejected(gv, algo, items, {2, 9})
    with naive_sum(gv):
        assert _all(gv, algo, items) == 1


# ---- VerifyAll ----
def _json_items(chacha_batch, aes_valid):
    items = []
    for k in range(4):
        p, s = chacha_batch[k]
        items.append({"cipher": "chacha20", "proof": base64.b64encode(p).decode(), "publicSignals": base64.b64encode(s).decode()})
        for name, (algo, cipher, _) in AES.items():
            p, s = aes_valid[name][k]
            items.append({"cipher": cipher, "proof": list(p), "publicSignals": list(s)})
    return items


def test_verify_all_json(gv, chacha_batch, aes_valid):
    items = _json_items(chacha_batch, aes_valid)
    assert gv.verify_all_json(items) is True
    for k in (0, 5, len(items) - 1):
        bad = [dict(it) for it in items]
        p = bytearray(base64.b64decode(bad[k]["proof"]) if isinstance(bad[k]["proof"], str) else bytes(bad[k]["proof"]))
        p[100] ^= 1
        bad[k]["proof"] = list(p)
        assert gv.verify_all_json(bad) is False
    assert gv.verify_all_json(items[:1] + [{"cipher": "chacha21", "proof": [], "publicSignals": []}]) is False
    assert gv.verify_all_json(b"[1,") is False
    assert gv.verify_all_json(b"[]") is False
    assert gv.verify_all_json(b'{"cipher":"chacha20"}') is False


# ---- the test hook ----
def test_randomizer_hook_refused_without_test_hooks():
    code = "import sys; sys.path.insert(0, %r); import gsc_loader; print(gsc_loader.load().debug_verify_randomizers(bytes(32)))" % ROOT
    env = {k: v for k, v in os.environ.items() if k != "GSC_ENABLE_TEST_HOOKS"}
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, timeout=300, check=True).stdout.decode().split()
    assert out[-1] == "-1"


def test_fixed_seed_gives_the_same_verdicts_twice(gv, chacha_batch):
    items = _corpus(random.Random(77), chacha_batch[:40], False)
    try:
        assert gv.debug_verify_randomizers(bytes(range(32))) == 0
        a = _batched(gv, 0, items)
        b = _batched(gv, 0, items)
        c = _all(gv, 0, chacha_batch)
    finally:
        assert gv.debug_verify_randomizers(None, False) == 0
    assert a == b == _gpu(gv, 0, items) and c == 1


# ---- beside a prover ----
def test_concurrent_batched_and_plain_verifiers_beside_a_prover(gsc_chacha, gv, chacha_batch):
    rnd = random.Random(19)
    recs = _records(rnd, 2048)
    done = {}

    def prove():
        done["prove"] = gsc_chacha.prove_raw(0, recs, 2048)

    def verify(t):
        items = chacha_batch[t * 1000:(t + 1) * 1000]
        items = [(p, s if i % 3 else chacha_batch[0][1]) for i, (p, s) in enumerate(items)]
        fn = _batched if t % 2 == 0 else _gpu
        done[t] = (fn(gv, 0, items), [int(i % 3 != 0 or t * 1000 + i == 0) for i in range(len(items))])

    th = [threading.Thread(target=prove)] + [threading.Thread(target=verify, args=(t,)) for t in range(4)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert done["prove"][0] == 2048
    for t in range(4):
        assert done[t][0] == done[t][1]
