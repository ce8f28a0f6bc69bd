"""GPU tests of key loading as gnark's ReadFrom does it: InitAlgorithm and gsc_verify_init take keys whose points are raw (WriteRawTo: X | Y,
flag bits 00) or compressed, element by element, and InitAlgorithm refuses a G2 point of the key that lies on the twist but outside the
r-torsion subgroup (gnark: "subgroup check failed").  Keys are rewritten by tests/keyraw.py from the reference's pk.chacha20 / vk.chacha20.

Every InitAlgorithm runs in a child process with the small engine settings of tests/test_gpu_degenerate.py."""
import os
import random
import subprocess
import sys

import pytest

import keyraw
from conftest import KAT, ROOT, golden_bytes

pytestmark = pytest.mark.gpu

SMALL_ENGINE = dict(GSC_MAX_BATCH="128", GSC_WINDOW_Z="6", GSC_W_TABLE_GB="8")
N_BATCH, N_FEW = 70, 3


def _write(name, data):
    path = os.path.join(ROOT, "build", name)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    open(path, "wb").write(data)
    return path


def _records(rnd, n):
    return [rnd.randbytes(44) + rnd.getrandbits(32).to_bytes(4, "little") + rnd.randbytes(64) for _ in range(n)]


def _signals(rec, ct):
    return ct + rec[32:44] + rec[44:48] + rec[48:]                    # ciphertext | nonce | counter (little-endian) | plaintext


# 70 statements in one call (the batch route), then 3 in a call of their own (the latency route), under fixed randomness
_PROVE = r"""
import random, sys
sys.path.insert(0, sys.argv[1])
import gsc_loader
from bench import golden
g = gsc_loader.load()
ok = g.init_algorithm(g.CHACHA20, open(sys.argv[2], "rb").read(), golden("r1cs.chacha20"))
print("INIT", int(ok))
if not ok:
    sys.exit(0)
rnd = random.Random(2024)
recs = [rnd.randbytes(44) + rnd.getrandbits(32).to_bytes(4, "little") + rnd.randbytes(64) for _ in range(73)]
g.set_deterministic_randomness(rnd.getrandbits(250), rnd.getrandbits(250), 0)
for first, n in ((0, 70), (70, 3)):
    ok, proofs, lens, cts = g.prove_raw(g.CHACHA20, b"".join(recs[first:first + n]), n)
    print("OK", ok)
    for k in range(n):
        print("PROOF", first + k, lens[k], proofs[196 * k:196 * k + 164].hex(), cts[64 * k:64 * k + 64].hex())
"""


def _start(script, *args):
    env = dict(os.environ, **SMALL_ENGINE)
    return subprocess.Popen([sys.executable, "-c", script, ROOT] + list(args), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def _finish(proc):
    out, err = proc.communicate(timeout=600)
    assert proc.returncode == 0, out + err
    return out


def test_mixed_raw_proving_key_gives_the_proofs_of_the_compressed_key(gsc):
    pk = golden_bytes("pk.chacha20")
    mixed = keyraw.mixed_pk(pk)
    secs = keyraw.pk_sections(mixed)
    nraw = {name: sum(sz in (64, 128) and mixed[o] & 0xC0 == 0 for o, sz in elems) for name, _, _, elems in secs}
    assert nraw["g1.alpha"] == nraw["g1.beta"] == nraw["g1.delta"] == nraw["g2.beta"] == nraw["g2.delta"] == 1
    assert nraw["g1.A"] == nraw["g1.B"] == nraw["g1.Z"] == nraw["g1.K"] == 667 and nraw["g2.B"] == 500
    # the two keys side by side, each in a process of its own (InitAlgorithm keeps the first key it was given)
    procs = [_start(_PROVE, _write("pk.chacha20.mixed_raw", mixed)), _start(_PROVE, _write("pk.chacha20.compressed", pk))]
    out_mixed, out_plain = [_finish(p) for p in procs]
    assert "INIT 1" in out_mixed, out_mixed                            # (the parent commit stops here: "uncompressed point encoding is not supported")
    assert "INIT 1" in out_plain, out_plain
    proofs = [l.split() for l in out_mixed.splitlines() if l.startswith("PROOF")]
    assert len(proofs) == N_BATCH + N_FEW and all(int(p[2]) == 164 for p in proofs), out_mixed
    assert [l for l in out_mixed.splitlines() if l.startswith(("OK", "PROOF"))] == [l for l in out_plain.splitlines() if l.startswith(("OK", "PROOF"))]
    assert [l for l in out_mixed.splitlines() if l.startswith("OK")] == ["OK %d" % N_BATCH, "OK %d" % N_FEW]
    # ... and libverify accepts every one of them
    assert gsc.init_verifier(0, golden_bytes("vk.chacha20"))
    recs = _records(random.Random(2024), N_BATCH + N_FEW)
    for k, (_, idx, ln, proof, ct) in enumerate(proofs):
        assert int(idx) == k
        assert gsc.verify({"cipher": "chacha20", "proof": bytes.fromhex(proof), "publicSignals": _signals(recs[k], bytes.fromhex(ct))}), k


# a key with a G2 point outside the subgroup must not load; the good key then loads in the same process and proves
_REFUSE = r"""
import random, sys
sys.path.insert(0, sys.argv[1])
import gsc_loader
from bench import golden
g = gsc_loader.load()
print("BAD", int(g.init_algorithm(g.CHACHA20, open(sys.argv[2], "rb").read(), golden("r1cs.chacha20"))))
print("GOOD", int(g.init_algorithm(g.CHACHA20, golden("pk.chacha20"), golden("r1cs.chacha20"))))
rnd = random.Random(7)
rec = rnd.randbytes(44) + rnd.getrandbits(32).to_bytes(4, "little") + rnd.randbytes(64)
ok, proofs, lens, cts = g.prove_raw(g.CHACHA20, rec, 1)
print("PROOF", ok, lens[0], proofs[:164].hex(), cts[:64].hex())
"""


@pytest.mark.parametrize("where,raw", [(("g2.B", 5), False), (("g2.beta", 0), True), (("g2.delta", 0), False)], ids=["G2.B[5]", "beta2-raw", "delta2"])
def test_g2_key_point_outside_the_subgroup_is_refused(gsc, where, raw):
    bad_point = keyraw.twist_point_outside_g2()
    assert not keyraw.g2_in_subgroup(bad_point) and keyraw.g2_in_subgroup(keyraw.G2_GEN)
    bad = keyraw.rewrite_pk(golden_bytes("pk.chacha20"), replace={where: keyraw.enc_g2(bad_point, raw)})
    out = _finish(_start(_REFUSE, _write("pk.chacha20.bad_%s" % where[0].replace(".", "_"), bad)))
    lines = out.splitlines()
    assert "BAD 0" in lines, out                                       # (the parent commit loads this key)
    assert any(l.startswith("pk: ") for l in lines[:lines.index("BAD 0")]), out      # one line on stdout, as the reference prints its read error
    assert "GOOD 1" in lines, out                                      # nothing of the failed attempt is in the way of the next one
    proof = [l.split() for l in lines if l.startswith("PROOF")][0]
    assert proof[1] == "1" and proof[2] == "164", out
    rnd = random.Random(7)
    rec = _records(rnd, 1)[0]
    assert gsc.init_verifier(0, golden_bytes("vk.chacha20"))
    assert gsc.verify({"cipher": "chacha20", "proof": bytes.fromhex(proof[3]), "publicSignals": _signals(rec, bytes.fromhex(proof[4]))})


def test_gpu_verifier_loads_the_raw_verifying_key(gsc):
    vk = golden_bytes("vk.chacha20")
    raw = keyraw.raw_vk(vk)
    sig = KAT["ciphertext"] + KAT["nonce"] + KAT["counter"].to_bytes(4, "little") + KAT["input"]
    good = [bytes.fromhex(h) for h in KAT["proofs"].values()]
    bad_sig = bytearray(sig); bad_sig[70] ^= 1
    bad_proof = bytearray(good[0]); bad_proof[40] ^= 1
    items = [(p, sig) for p in good] + [(good[0], bytes(bad_sig)), (bytes(bad_proof), sig), (good[1], sig)]
    proofs = b"".join(p + bytes(196 - len(p)) for p, _ in items)
    lens = [len(p) for p, _ in items]
    signals = b"".join(s for _, s in items)
    verdicts = {}
    try:
        for tag, key in (("compressed", vk), ("raw", raw)):
            assert gsc.verify_init(0, key), tag
            for mode in (1, 2):                                        # one thread per proof, the few-proof groups
                assert gsc.debug_verify_path(mode) == 0
                verdicts[tag, mode] = gsc.verify_raw(0, proofs, lens, signals)
                assert gsc.verify_last_path(0) == mode
    finally:
        gsc.debug_verify_path(0)
    assert verdicts["compressed", 1] == [1, 1, 0, 0, 1]
    assert all(v == verdicts["compressed", 1] for v in verdicts.values()), verdicts
    # a raw y off by one, and a raw gamma outside the subgroup: refused, and the key loaded before stays in force
    o, sz = dict((name, elems) for name, _, _, elems in keyraw.vk_sections(raw))["g1.K"][4][:2]
    off = bytearray(raw); off[o + 63] ^= 1
    assert not gsc.verify_init(0, bytes(off))
    outside = keyraw.rewrite_vk(raw, replace={("g2.gamma", 0): keyraw.enc_g2(keyraw.twist_point_outside_g2(), True)})
    assert not gsc.verify_init(0, outside)
    assert gsc.verify_raw(0, proofs, lens, signals) == [1, 1, 0, 0, 1]
    assert gsc.verify_init(0, vk)
