"""GPU tests of the prover's self-check (gsc_prove_check_init, k_prove_check.hip): with the check on, every chunk is verified on the device from
the prover's own output buffers before anything is released.  A clean run gives the bytes of an unchecked run; a proof changed on the device
behind the assembly (gsc_debug_prove_corrupt) is refused alone, and the same change with the check off is released and rejected by libverify.so —
so the hook bites and the check is what stops it.  Small calls beside the session's loaded algorithms; the check is off again afterwards."""
import base64
import json
import random
import threading

import pytest

from conftest import AES, golden_bytes

pytestmark = pytest.mark.gpu

R, S, MASK = 0x1234567, 0xabcdef0123456789abcdef, 0x77
N = 65      # two 64-column groups: the second holds one statement and 63 padding columns


def _records(n, seed, aes=False):
    rnd = random.Random(seed)
    return b"".join(rnd.randbytes(44) + rnd.getrandbits(31 if aes else 32).to_bytes(4, "little") + rnd.randbytes(64) for _ in range(n))


def _signals(rec, ct, aes=False):
    return ct + rec[32:44] + (rec[44:48][::-1] if aes else rec[44:48]) + rec[48:112]


def _verdicts(g, cipher, recs, proofs, lens, cts, aes=False):
    """libverify.so on every released item (an item that was not released: None)"""
    out = []
    for k, ln in enumerate(lens):
        sig = _signals(recs[112 * k:112 * k + 112], cts[64 * k:64 * k + 64], aes)
        out.append(g.verify({"cipher": cipher, "proof": proofs[196 * k:196 * k + ln], "publicSignals": sig}) if ln else None)
    return out


def _fixed(g, algo, recs, n):
    g.set_deterministic_randomness(R, S, MASK)
    try:
        return g.prove_raw(algo, recs, n)
    finally:
        g.set_deterministic_randomness(None)


def _delta(g, algo, before):
    return tuple(a - b for a, b in zip(g.prove_check_stats(algo), before))


@pytest.fixture(scope="module")
def chk(gsc_chacha, request):
    g = gsc_chacha

    def off():
        for algo in (0, 1, 2):
            g.prove_check_init(algo)      # (-1 for an algorithm the session never loaded)
    request.addfinalizer(off)
    assert g.init_verifier(0, golden_bytes("vk.chacha20"))
    assert g.prove_check_init(0) == 1 and "check=off" in g.describe(0)
    return g


@pytest.fixture(scope="module")
def clean(chk):
    """the reference run, computed once: N fixed statements, fixed randomness, the check off"""
    recs = _records(N, 650)
    ok, proofs, lens, cts = _fixed(chk, 0, recs, N)
    assert ok == N and set(lens) == {164}
    return recs, proofs, lens, cts


def test_checked_and_unchecked_runs_are_byte_identical(chk, clean):
    g = chk; recs, proofs, lens, cts = clean
    assert g.prove_check_stats(0) == (0, 0, 0, 0)
    assert g.prove_check_init(0, golden_bytes("vk.chacha20")) == 1
    assert "check=on(" in g.describe(0)
    before = g.prove_check_stats(0)
    ok, p2, l2, c2 = _fixed(g, 0, recs, N)
    assert _delta(g, 0, before) == (1, N, 0, 0)
    assert (ok, p2, l2, c2) == (N, proofs, lens, cts)
    assert _verdicts(g, "chacha20", recs, p2, l2, c2) == [True] * N


@pytest.mark.parametrize("which,mode", [("A", 0), ("B", 0), ("C", 0), ("C", 1)])
def test_a_corrupted_statement_is_refused_alone(chk, clean, which, mode):
    g = chk; recs, proofs, lens, cts = clean
    last = N - 1
    # control, the check off: the changed proof is released
    assert g.prove_check_init(0) == 1
    assert g.debug_prove_corrupt(0, last, which, mode) == 0
    ok, pc, lc, cc = _fixed(g, 0, recs, N)
    assert ok == N and pc[:196 * last] == proofs[:196 * last]
    got = _verdicts(g, "chacha20", recs, pc, lc, cc)
    if mode == 0:
        assert got == [True] * last + [False], "the hook did not bite"
    else:
        # a y off the curve does not survive compression: the released bytes are rejected, or they are the clean proof's (they decode to the point
        # the device no longer held).  Either way the device's point was not the one the bytes stand for, and the check must refuse it.
        assert got[:last] == [True] * last and (got[last] is False or pc[196 * last:] == proofs[196 * last:])
    # the check on: item 64 is refused, the others are the clean run's bytes
    assert g.prove_check_init(0, golden_bytes("vk.chacha20")) == 1
    before = g.prove_check_stats(0)
    assert g.debug_prove_corrupt(0, last, which, mode) == 0
    ok, p2, l2, c2 = _fixed(g, 0, recs, N)
    assert ok == last and l2 == lens[:last] + [0] and p2[196 * last:] == bytes(196)
    assert p2[:196 * last] == proofs[:196 * last] and c2 == cts
    assert _delta(g, 0, before) == (1, N, 1, 1)
    # one shot: the next call is clean again
    ok, p3, l3, _ = _fixed(g, 0, recs, N)
    assert (ok, p3, l3) == (N, proofs, lens)
    assert _delta(g, 0, before) == (2, 2 * N, 1, 1)


def test_single_prove_through_the_micro_batcher(chk):
    g = chk
    assert g.prove_check_init(0, golden_bytes("vk.chacha20")) == 1
    rec = _records(1, 651)
    req = {"cipher": "chacha20", "key": list(rec[:32]), "nonce": list(rec[32:44]), "counter": int.from_bytes(rec[44:48], "little"), "input": list(rec[48:112])}

    def accepted():
        out = json.loads(g.prove(req))
        if out == {}:
            return None
        return g.verify({"cipher": "chacha20", "proof": base64.b64decode(out["proof"]["proofJson"]), "publicSignals": _signals(rec, base64.b64decode(out["publicSignals"]))})
    before = g.prove_check_stats(0)
    assert accepted() is True
    assert g.debug_prove_corrupt(0, 0, "A", 1) == 0      # (mode 0 of a lone statement would copy its own point)
    assert accepted() is None
    assert accepted() is True
    assert _delta(g, 0, before) == (3, 3, 1, 1)


@pytest.fixture(scope="module")
def aes(chk, aes_keys):
    g = chk
    for name, (algo, cipher, keylen) in AES.items():
        r1cs, pk, vk = aes_keys[name]
        assert g.init_algorithm(algo, pk, r1cs), name
        assert g.init_verifier(algo, vk)
    return g


def test_aes128_commitment_points(aes, aes_keys):
    g = aes; vk = aes_keys["aes128"][2]
    recs = _records(3, 652, aes=True)
    ok, proofs, lens, cts = _fixed(g, 1, recs, 3)
    assert ok == 3 and lens == [196] * 3
    assert g.prove_check_init(1, vk) == 1
    before = g.prove_check_stats(1)
    ok, p2, l2, c2 = _fixed(g, 1, recs, 3)
    assert (ok, p2, l2, c2) == (3, proofs, lens, cts) and _delta(g, 1, before) == (1, 3, 0, 0)
    assert _verdicts(g, "aes-128-ctr", recs, p2, l2, c2, aes=True) == [True] * 3
    for which in ("D", "PoK"):
        before = g.prove_check_stats(1)
        assert g.debug_prove_corrupt(1, 1, which, 0) == 0
        ok, p2, l2, c2 = _fixed(g, 1, recs, 3)
        assert ok == 2 and l2 == [196, 0, 196] and p2[196:392] == bytes(196)
        assert p2[:196] == proofs[:196] and p2[392:] == proofs[392:]
        assert _delta(g, 1, before) == (1, 3, 1, 1)
    assert g.debug_prove_corrupt(0, 0, "D", 0) == -1      # a ChaCha20 proof has no commitment


def test_aes256_one_statement(aes, aes_keys):
    g = aes
    assert g.prove_check_init(2, aes_keys["aes256"][2]) == 1
    recs = _records(1, 653, aes=True)
    before = g.prove_check_stats(2)
    ok, proofs, lens, cts = g.prove_raw(2, recs, 1)
    assert ok == 1 and lens == [196] and _delta(g, 2, before) == (1, 1, 0, 0)
    assert _verdicts(g, "aes-256-ctr", recs, proofs, lens, cts, aes=True) == [True]


def test_a_wrong_key_refuses_everything_and_a_garbage_key_changes_nothing(aes, aes_keys):
    g = aes; r1cs, _, vk = aes_keys["aes128"]
    _, other = g.setup(r1cs, bytes([0x5A] * 32))      # a verifying key of the same circuit from another setup
    assert other != vk
    recs = _records(3, 654, aes=True)
    assert g.prove_check_init(1, other) == 1
    before = g.prove_check_stats(1)
    ok, proofs, lens, _ = g.prove_raw(1, recs, 3)
    assert ok == 0 and lens == [0] * 3 and proofs == bytes(3 * 196)
    assert _delta(g, 1, before) == (1, 3, 3, 1)
    assert g.prove_check_init(1, vk) == 1
    ok, proofs, lens, cts = g.prove_raw(1, recs, 3)
    assert ok == 3 and _verdicts(g, "aes-128-ctr", recs, proofs, lens, cts, aes=True) == [True] * 3
    # a slice that is no key: refused, and the right key stays loaded
    assert g.prove_check_init(1, b"\x01" * 100) == 0 and g.prove_check_init(1, vk[:-1]) == 0
    before = g.prove_check_stats(1)
    assert g.prove_raw(1, recs, 3)[0] == 3 and _delta(g, 1, before) == (1, 3, 0, 0)


def test_two_threads_share_the_context(chk, clean):
    g = chk
    assert g.prove_check_init(0, golden_bytes("vk.chacha20")) == 1
    before = g.prove_check_stats(0)
    sets = [_records(N, 660 + t) for t in range(2)]
    res = [None, None]

    def work(t):
        res[t] = g.prove_raw(0, sets[t], N)
    th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for t in range(2):
        ok, proofs, lens, cts = res[t]
        assert ok == N and _verdicts(g, "chacha20", sets[t], proofs, lens, cts) == [True] * N
    assert _delta(g, 0, before) == (2, 2 * N, 0, 0)
    total, dirty, info = g.debug_secret_scan(0)
    assert total == 0 and not dirty and info["registered"] == info["allocated"]


def test_an_empty_key_turns_the_check_off(chk, clean):
    g = chk; recs, proofs, lens, cts = clean
    assert g.prove_check_init(0, golden_bytes("vk.chacha20")) == 1
    _fixed(g, 0, recs, N)
    assert g.prove_check_stats(0)[0] >= 1
    assert g.prove_check_init(0) == 1
    assert g.prove_check_stats(0) == (0, 0, 0, 0) and "check=off" in g.describe(0)
    ok, p2, l2, c2 = _fixed(g, 0, recs, N)
    assert (ok, p2, l2, c2) == (N, proofs, lens, cts)
    assert g.prove_check_stats(0) == (0, 0, 0, 0)
