"""GPU tests of the Groth16 verifier in libprove.so (gsc_verify_init / gsc_verify_raw / VerifyBatch / gsc_debug_pairing, k_verify.hip):
every verdict must equal libverify.so's Verify on the same input, element for element."""
import base64
import json
import random
import threading
from concurrent.futures import ThreadPoolExecutor

import pytest

from conftest import AES, KAT, golden_bytes
from test_verifier import _twist_point_outside_g2

pytestmark = pytest.mark.gpu

P = 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47
R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
NAMES = {0: "chacha20", 1: "aes-128-ctr", 2: "aes-256-ctr"}


def _kat_sig():
    return KAT["ciphertext"] + KAT["nonce"] + KAT["counter"].to_bytes(4, "little") + KAT["input"]


def _cpu(gsc, algo, items):
    """libverify's verdicts, 16 host threads (Verify releases the GIL)."""
    with ThreadPoolExecutor(16) as ex:
        return list(ex.map(lambda it: int(gsc.verify({"cipher": NAMES[algo], "proof": it[0], "publicSignals": it[1]})), items))


def _gpu(gsc, algo, items):
    slots = b"".join(p[:196].ljust(196, b"\0") for p, _ in items)
    lens = [len(p) if len(p) <= 196 else 0xFFFFFFFF for p, _ in items]
    return gsc.verify_raw(algo, slots, lens, b"".join(s for _, s in items))


@pytest.fixture(scope="module")
def gv(gsc):
    vk = golden_bytes("vk.chacha20")
    assert gsc.init_verifier(0, vk) and gsc.verify_init(0, vk)
    return gsc


def test_kat_and_every_single_bit_flip(gv):
    sig = _kat_sig()
    for h in KAT["proofs"].values():
        proof = bytes.fromhex(h)
        items = [(proof, sig)]
        for i in range(8 * len(sig)):
            b = bytearray(sig); b[i // 8] ^= 1 << (i % 8); items.append((proof, bytes(b)))
        for i in range(8 * len(proof)):
            b = bytearray(proof); b[i // 8] ^= 1 << (i % 8); items.append((bytes(b), sig))
        got = _gpu(gv, 0, items)
        assert got[0] == 1
        assert got == _cpu(gv, 0, items)


def _records(rnd, n):
    return b"".join(rnd.randbytes(32) + rnd.randbytes(12) + rnd.getrandbits(32).to_bytes(4, "little") + rnd.randbytes(64) for _ in range(n))


def _chacha_items(recs, proofs, lens, cts, n):
    out = []
    for k in range(n):
        rec = recs[112 * k:112 * k + 112]
        out.append((proofs[196 * k:196 * k + lens[k]], cts[64 * k:64 * k + 64] + rec[32:44] + rec[44:48] + rec[48:]))
    return out


@pytest.fixture(scope="module")
def chacha_batch(gsc_chacha, gv):
    rnd = random.Random(4099)
    recs = _records(rnd, 4099)
    ok, proofs, lens, cts = gsc_chacha.prove_raw(0, recs, 4099)
    assert ok == 4099
    return _chacha_items(recs, proofs, lens, cts, 4099)


def test_prover_round_trip(gsc_chacha, gv, chacha_batch):
    rnd = random.Random(5)
    for n in (1, 63, 64, 65):
        recs = _records(rnd, n)
        ok, proofs, lens, cts = gsc_chacha.prove_raw(0, recs, n)
        assert ok == n
        assert _gpu(gv, 0, _chacha_items(recs, proofs, lens, cts, n)) == [1] * n
    assert _gpu(gv, 0, chacha_batch) == [1] * 4099
    shifted = [(chacha_batch[i][0], chacha_batch[(i + 1) % 4099][1]) for i in range(4099)]
    assert _gpu(gv, 0, shifted) == [0] * 4099


def test_batch_larger_than_a_device_chunk(gsc_chacha, gv):
    n = 65536 + 1000
    rnd = random.Random(66)
    recs = _records(rnd, n)
    ok, proofs, lens, cts = gsc_chacha.prove_raw(0, recs, n)
    assert ok == n
    items = _chacha_items(recs, proofs, lens, cts, n)
    items[66000] = (items[66000][0], items[0][1])
    want = [1] * n; want[66000] = 0
    assert _gpu(gv, 0, items) == want


def _point_variants(proof, off, g2):
    """encodings of the point at `off` that exercise the decoder: flag patterns with and without stray bits, x = p / p+1, no root."""
    n = 64 if g2 else 32
    out = []
    for flag in (0x00, 0x40, 0x80, 0xC0):
        for stray in (False, True):
            enc = bytearray(n)
            enc[0] = flag
            if stray:
                enc[n - 1] = 1
            out.append(proof[:off] + bytes(enc) + proof[off + n:])
            enc2 = bytearray(proof[off:off + n]); enc2[0] = (enc2[0] & 0x3F) | flag
            out.append(proof[:off] + bytes(enc2) + proof[off + n:])
    for x in (P, P + 1):
        enc = bytearray(x.to_bytes(32, "big")); enc[0] |= 0x80
        out.append(proof[:off] + bytes(enc) + proof[off + 32:])
    # x with no square root of x^3 + 3 (G1) / of x^3 + b' (twist): 5 and (5, 1) in the first word
    for k in range(2, 40):
        if not g2 and pow((k ** 3 + 3) % P, (P - 1) // 2, P) == P - 1:
            out.append(proof[:off] + bytes([0x80]) + k.to_bytes(32, "big")[1:] + proof[off + 32:])
            break
    if g2:
        out.append(proof[:off] + _twist_point_outside_g2() + proof[off + 64:])
        for k in range(1, 40):
            out.append(proof[:off] + bytes([0x80]) + bytes(30) + bytes([1]) + k.to_bytes(32, "big") + proof[off + 64:])
    return out


def _corpus(rnd, valid, has_commitment):
    items = []
    offs = [(0, False), (32, True), (96, False)] + ([(132, False), (164, False)] if has_commitment else [(132, False)])
    for idx, (proof, sig) in enumerate(valid):
        items.append((proof, sig))
        for _ in range(3):
            off, g2 = rnd.choice(offs)
            b = bytearray(proof); b[off + rnd.randrange(64 if g2 else 32)] ^= 1 << rnd.randrange(8); items.append((bytes(b), sig))
        if idx % 4 == 0:
            off, g2 = offs[idx // 4 % len(offs)]
            items += [(v, sig) for v in _point_variants(proof, off, g2)]
        items.append((proof[:-1], sig))
        items.append((proof + bytes(32), sig))
        b = bytearray(proof); b[131] ^= 1; items.append((bytes(b), sig))
        items.append((proof, valid[(idx + 1) % len(valid)][1]))                                # signals of another statement
    rnd.shuffle(items)
    return items


def test_agreement_corpus_chacha(gv, chacha_batch):
    rnd = random.Random(2000)
    items = _corpus(rnd, chacha_batch[:260], False)
    assert len(items) >= 2000
    got = _gpu(gv, 0, items)
    assert sum(got) > 0 and got == _cpu(gv, 0, items)


@pytest.fixture(scope="module")
def aes_valid(gsc, aes_keys):
    out = {}
    for name, (algo, cipher, keylen) in AES.items():
        r1cs, pk, vk = aes_keys[name]
        assert gsc.init_algorithm(algo, pk, r1cs) and gsc.init_verifier(algo, vk) and gsc.verify_init(algo, vk)
        rnd = random.Random(300 + algo)
        n = 160
        recs = b"".join(rnd.randbytes(32) + rnd.randbytes(12) + rnd.getrandbits(31).to_bytes(4, "little") + rnd.randbytes(64) for _ in range(n))
        ok, proofs, lens, cts = gsc.prove_raw(algo, recs, n)
        assert ok == n
        out[name] = [(proofs[196 * k:196 * k + lens[k]], cts[64 * k:64 * k + 64] + recs[112 * k + 32:112 * k + 44] + recs[112 * k + 44:112 * k + 48][::-1] + recs[112 * k + 48:112 * k + 112])
                     for k in range(n)]
    return out


@pytest.mark.parametrize("name", list(AES))
def test_aes_commitment_proofs_and_agreement(gv, aes_valid, name):
    algo = AES[name][0]
    valid = aes_valid[name]
    assert _gpu(gv, algo, valid) == [1] * len(valid)
    tampered = []
    for proof, sig in valid[:20]:
        for pos in (140, 150, 170, 190):                                                     # D, PoK
            b = bytearray(proof); b[pos] ^= 1; tampered.append((bytes(b), sig))
    got = _gpu(gv, algo, tampered)
    assert sum(got) == 0 and got == _cpu(gv, algo, tampered)
    items = _corpus(random.Random(algo), valid, True)
    assert len(items) >= 2000
    assert _gpu(gv, algo, items) == _cpu(gv, algo, items)


# ---- pairing hook: bilinearity, non-degeneracy, order r ----
def _f2mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def _f2inv(a):
    n = pow(a[0] * a[0] + a[1] * a[1], -1, P)
    return (a[0] * n % P, -a[1] * n % P)


def _add(p, q, f2):
    if p is None:
        return q
    if q is None:
        return p
    mul = _f2mul if f2 else (lambda a, b: a * b % P)
    inv = _f2inv if f2 else (lambda a: pow(a, -1, P))
    sub = (lambda a, b: ((a[0] - b[0]) % P, (a[1] - b[1]) % P)) if f2 else (lambda a, b: (a - b) % P)
    sc = (lambda a, k: (a[0] * k % P, a[1] * k % P)) if f2 else (lambda a, k: a * k % P)
    if p[0] == q[0]:
        if p[1] != q[1]:
            return None
        lam = mul(sc(mul(p[0], p[0]), 3), inv(sc(p[1], 2)))
    else:
        lam = mul(sub(q[1], p[1]), inv(sub(q[0], p[0])))
    x3 = sub(sub(mul(lam, lam), p[0]), q[0])
    return (x3, sub(mul(lam, sub(p[0], x3)), p[1]))


def _smul(p, k, f2):
    acc = None
    for bit in bin(k)[2:]:
        acc = _add(acc, acc, f2)
        if bit == "1":
            acc = _add(acc, p, f2)
    return acc


G1 = (1, 2)
G2 = ((0x1800deef121f1e76426a00665e5c4479674322d4f75edadd46debd5cd992f6ed, 0x198e9393920d483a7260bfb731fb5d25f1aa493335a9e71297e485b7aef312c2),
      (0x12c85ea5db8c6deb4aab71808dcb408fe3d1e7690c43d37b4ce6cc0166fa7daa, 0x090689d0585ff075ec9e99ad690c3395bc4b313370b38ef355acdadcd122975b))


def test_pairing_hook_bilinear_nondegenerate_order_r(gv):
    a, b = 0x1234567890abcdef, 0xfedcba987654321
    Ps = [_smul(G1, a, False), _smul(G1, a * b % R, False), G1, G1, None]
    Qs = [_smul(G2, b, True), G2, G2, _smul(G2, R - 1, True), G2]
    e = gv.debug_pairing(Ps, Qs)
    one = tuple([1] + [0] * 11)
    assert e[0] == e[1]                                  # e([a]P, [b]Q) == e([ab]P, Q)
    assert e[2] != one                                   # non-degenerate
    assert e[4] == one                                   # infinity skipped
    # e(P, Q) e(P, [r-1]Q) = e(P, Q)^r = 1: multiply the two results in Fp12 = Fp2[w]/(w^6 - (9+u))
    def f12(v):
        return [(v[2 * i], v[2 * i + 1]) for i in range(6)]
    x, y = f12(e[2]), f12(e[3])
    t = [(0, 0)] * 11
    for i in range(6):
        for j in range(6):
            m = _f2mul(x[i], y[j]); t[i + j] = ((t[i + j][0] + m[0]) % P, (t[i + j][1] + m[1]) % P)
    prod = []
    for k in range(6):
        v = t[k]
        if k + 6 < 11:
            m = _f2mul(t[k + 6], (9, 1)); v = ((v[0] + m[0]) % P, (v[1] + m[1]) % P)
        prod += [v[0], v[1]]
    assert tuple(prod) == one


# ---- VerifyBatch ----
def test_verify_batch(gv, aes_valid, chacha_batch):
    items = []
    for k in range(6):
        p, s = chacha_batch[k]
        items.append({"cipher": "chacha20", "proof": base64.b64encode(p).decode(), "publicSignals": base64.b64encode(s).decode()})
        p, s = aes_valid["aes128"][k]
        items.append({"cipher": "aes-128-ctr", "proof": list(p), "publicSignals": list(s)})
    items.insert(3, {"cipher": "chacha20", "proof": [1, 2, 3], "publicSignals": [0] * 144})
    items.insert(5, {"cipher": "chacha21", "proof": [], "publicSignals": []})
    items.insert(7, [1, 2])
    items.insert(9, {"cipher": "chacha20", "proof": "!!!", "publicSignals": "AAAA"})
    got = gv.verify_batch(items)
    want = [gv.verify(json.dumps(it)) if isinstance(it, dict) else False for it in items]
    assert got == want and got.count(True) == 12
    assert gv.verify_batch([]) == []
    assert json.loads(gv.verify_batch_bytes(b'{"cipher":"chacha20"}')) == "VerifyBatch expects a JSON array"
    assert json.loads(gv.verify_batch_bytes(b"[1,")) == {"Offset": 3}


def test_concurrent_verifiers_beside_a_prover(gsc_chacha, gv, chacha_batch):
    rnd = random.Random(9)
    recs = _records(rnd, 2048)
    done = {}

    def prove():
        done["prove"] = gsc_chacha.prove_raw(0, recs, 2048)

    def verify(t):
        items = chacha_batch[t * 1000:(t + 1) * 1000]
        items = [(p, s if i % 3 else chacha_batch[0][1]) for i, (p, s) in enumerate(items)]
        done[t] = (_gpu(gv, 0, items), [int(i % 3 != 0 or t * 1000 + i == 0) for i in range(len(items))])

    th = [threading.Thread(target=prove)] + [threading.Thread(target=verify, args=(t,)) for t in range(4)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert done["prove"][0] == 2048
    for t in range(4):
        assert done[t][0] == done[t][1]
