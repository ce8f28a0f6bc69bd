"""The prover process of tests/test_gpu_setup_from_srs.py: the production path from a powers file to proofs, in a process of its own (the pytest
session keeps its own algorithms and verifying keys loaded).
python srs_child.py <root> <algorithm id> <n> <out.json> <dir with srs>: gsc_setup_from_srs (delta = 1) -> one gsc_setup_contribute ->
gsc_setup_verify_contribution -> InitAlgorithm with the contributed pk -> n proofs, their verdicts under the contributed vk by libverify.so's
verifier, with a flipped public-signal bit, and under the delta = 1 vk.  Writes the facts as JSON and prints CHILD-OK; the test judges."""
import base64
import json
import os
import sys

ROOT, ALGO, N, OUT, DIR = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5]
sys.path.insert(0, ROOT)
import bench          # noqa: E402
import gsc_loader     # noqa: E402

g = gsc_loader.load()
NAME = {0: "chacha20", 1: "aes-128-ctr", 2: "aes-256-ctr"}[ALGO]
R1CS = bench.golden({0: "r1cs.chacha20", 1: "r1cs.aes128", 2: "r1cs.aes256"}[ALGO])

if __name__ == "__main__":
    srs = open(os.path.join(DIR, "srs"), "rb").read()
    facts = {"srs_ok": bool(g.srs_verify(srs))}
    pk0, vk0 = g.setup_from_srs(R1CS, srs)
    pk1, vk1, rec = g.setup_contribute(pk0, vk0)
    facts["step_ok"] = bool(g.setup_verify_contribution(pk0, vk0, pk1, vk1, rec))
    assert g.init_algorithm(ALGO, pk1, R1CS)
    recs = bench.xoshiro_records(N, 0x515 << 20)
    ok, proofs, lens, cts = g.prove_raw(ALGO, recs, N)
    assert ok == N, ok
    facts["lens"] = list(lens)

    def signals(k):      # libverify's publicSignals: ciphertext | nonce | counter (ChaCha20: little-endian; AES: big-endian) | input
        rec = recs[112 * k:112 * (k + 1)]
        return cts[64 * k:64 * k + 64] + rec[32:44] + (rec[44:48] if ALGO == 0 else rec[44:48][::-1]) + rec[48:]

    def verdict(k, sig):
        return bool(g.verify({"cipher": NAME, "proof": base64.b64encode(proofs[196 * k:196 * k + lens[k]]).decode(), "publicSignals": base64.b64encode(sig).decode()}))

    assert g.init_verifier(ALGO, vk1)
    facts["new"] = [verdict(k, signals(k)) for k in range(N)]
    flipped = bytearray(signals(0)); flipped[5] ^= 0x10
    facts["flipped"] = verdict(0, bytes(flipped))
    assert g.init_verifier(ALGO, vk0)
    facts["old"] = [verdict(k, signals(k)) for k in range(N)]
    json.dump(facts, open(OUT, "w"))
    print("CHILD-OK", flush=True)
