"""The prover process of tests/test_gpu_phase2.py: a key pair that came out of gsc_setup_contribute, loaded like any other (the pytest session
keeps its own algorithms and verifying keys loaded; loading others there would take them from the other tests).
python phase2_child.py <root> <algorithm id> <n> <out.json> <dir with pk.new / vk.new / vk.old>: InitAlgorithm(pk.new), gsc_verify_init(vk.new), n
statements proved, their verdicts under vk.new by gsc_verify_raw and by the oracle, then under vk.old.  Writes the facts as JSON and prints
CHILD-OK; the test judges."""
import json
import os
import sys

ROOT, ALGO, N, OUT, KEYS = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5]
sys.path.insert(0, ROOT)
import bench          # noqa: E402
import gsc_loader     # noqa: E402
from oracle import oracle as O      # noqa: E402

g = gsc_loader.load()
NAME = {0: "chacha20", 1: "aes-128-ctr", 2: "aes-256-ctr"}[ALGO]
R1CS = bench.golden({0: "r1cs.chacha20", 1: "r1cs.aes128", 2: "r1cs.aes256"}[ALGO])


def read(name):
    return open(os.path.join(KEYS, name), "rb").read()


if __name__ == "__main__":
    pk, vk, vk_old = read("pk.new"), read("vk.new"), read("vk.old")
    assert g.init_algorithm(ALGO, pk, R1CS)
    recs = bench.xoshiro_records(N, 0x9A5E << 20)
    ok, proofs, lens, cts = g.prove_raw(ALGO, recs, N)
    assert ok == N, ok
    sig = [bench.signals_of(NAME, recs[112 * k:112 * (k + 1)], cts[64 * k:64 * k + 64]) for k in range(N)]
    facts = {"lens": list(lens)}
    assert g.verify_init(ALGO, vk)
    facts["new"] = list(g.verify_raw(ALGO, proofs, list(lens), b"".join(sig), N))
    ovk = O.VerifyingKey(vk)
    facts["oracle_new"] = [bool(O.verify(ovk, NAME, proofs[196 * k:196 * k + lens[k]], sig[k])) for k in range(N)]
    assert g.verify_init(ALGO, vk_old)
    facts["old"] = list(g.verify_raw(ALGO, proofs, list(lens), b"".join(sig), N))
    json.dump(facts, open(OUT, "w"))
    print("CHILD-OK", flush=True)
