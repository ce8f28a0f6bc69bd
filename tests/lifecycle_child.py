"""The prover process of tests/test_gpu_lifecycle.py: one case per run, with engines of its own (the pytest session keeps its algorithms
loaded, and a release there would take them from the other tests).  python lifecycle_child.py <root> <case> <out.json> <dir with pk.b / vk.b>;
writes the facts of the case as JSON and prints CHILD-OK.  Nothing is asserted here beyond what the case needs to go on: the test judges."""
import base64
import json
import os
import sys
import threading
import time

ROOT, CASE, OUT, KEYS = sys.argv[1:5]
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench          # noqa: E402
import gsc_loader     # noqa: E402

g = gsc_loader.load()
N = 65                                                       # two 64-column groups
R, S = 0x1234567, 0xabcdef0123456789abcdef
NOT_INIT = b'"proving params are not initialized for cipher: chacha20"'
R1CS = bench.golden("r1cs.chacha20")
PK_A, VK_A = bench.golden("pk.chacha20"), bench.golden("vk.chacha20")
RECS = bench.xoshiro_records(N, 0x11FE << 20)


def key_b():
    return open(os.path.join(KEYS, "pk.b"), "rb").read(), open(os.path.join(KEYS, "vk.b"), "rb").read()


def params(rec):
    return json.dumps({"cipher": "chacha20", "key": list(rec[:32]), "nonce": list(rec[32:44]), "counter": int.from_bytes(rec[44:48], "little"),
                       "input": list(rec[48:112])}).encode()


def prove_all():
    """the 65 statements in one gsc_prove_raw call, then statement 64 once more as a single Prove (the micro-batcher) -> hex of it all"""
    ok, proofs, lens, cts = g.prove_raw(0, RECS, N)
    assert ok == N and set(lens) == {164}, (ok, set(lens))
    single = json.loads(g.prove(params(RECS[112 * 64:112 * 65])))
    return (proofs + cts).hex() + base64.b64decode(single["proof"]["proofJson"]).hex()


def verdicts(vk, recs, proofs, cts, n):
    """gsc_verify_raw under vk for n proofs of 164 bytes in 196-byte slots"""
    assert g.verify_init(0, vk)
    sig = b"".join(bench.signals_of("chacha20", recs[112 * k:112 * (k + 1)], cts[64 * k:64 * k + 64]) for k in range(n))
    return g.verify_raw(0, proofs, [164] * n, sig, n)


def facts_now():
    m = g.memory_info(0)
    return {"gen": g.key_generation(0), "key": g.key_id(0), "provers": m["provers"], "verifiers": m["verifiers"], "free": m["free"]}


class Callers:
    """eight closed-loop JSON Prove callers and one gsc_prove_raw caller of 65 statements; every call is logged with its start and end"""

    def __init__(self):
        self.stop = False
        self.logs = [[] for _ in range(9)]
        self.recs = [bench.xoshiro_records(64, (0x2000 + t) << 20) for t in range(8)]
        self.threads = [threading.Thread(target=self.json_loop, args=(t,)) for t in range(8)] + [threading.Thread(target=self.raw_loop)]

    def json_loop(self, t):
        k = 0
        while not self.stop:
            rec = self.recs[t][112 * (k % 64):112 * (k % 64 + 1)]
            t0 = time.monotonic(); out = g.prove(params(rec)); t1 = time.monotonic()
            self.logs[t].append((t0, t1, rec, out))
            k += 1

    def raw_loop(self):
        while not self.stop:
            t0 = time.monotonic(); out = g.prove_raw(0, RECS, N); t1 = time.monotonic()
            self.logs[8].append((t0, t1, RECS, out))

    def start(self):
        for th in self.threads:
            th.start()

    def finish(self):
        self.stop = True
        for th in self.threads:
            th.join()

    def judged(self, windows, after):
        """per thread: calls in all, calls inside each (t0, t1) window, and what the calls were: a proof valid under A / under B / under both or
        neither, the not-initialised answer, anything else; `after`: the calls that started later than that must be A's"""
        recs, proofs, cts, owner = [], [], [], []
        per = [{"calls": len(log), "inside": [sum(1 for c in log if c[0] >= w0 and c[1] <= w1) for w0, w1 in windows], "not_init": 0, "other": 0, "late_not_a": 0} for log in self.logs]
        for d in per:
            d.update(a=0, b=0, both=0, neither=0)
        for t, log in enumerate(self.logs):
            for ci, (t0, t1, rec, out) in enumerate(log):
                if t < 8:
                    if out == NOT_INIT:
                        per[t]["not_init"] += 1; continue
                    try:
                        o = json.loads(out); p = base64.b64decode(o["proof"]["proofJson"]); ct = base64.b64decode(o["publicSignals"])
                        assert len(p) == 164 and len(ct) == 64
                    except Exception:
                        per[t]["other"] += 1; continue
                    recs.append(rec); proofs.append(p + bytes(32)); cts.append(ct); owner.append((t, ci))
                else:
                    ok, pr, lens, ct = out
                    if ok == -1:
                        per[t]["not_init"] += 1; continue
                    if ok != N or set(lens) != {164}:
                        per[t]["other"] += 1; continue
                    for k in range(N):
                        recs.append(rec[112 * k:112 * (k + 1)]); proofs.append(pr[196 * k:196 * (k + 1)]); cts.append(ct[64 * k:64 * (k + 1)]); owner.append((t, ci))
        n = len(proofs)
        if not n:
            return per, 0
        va = verdicts(VK_A, b"".join(recs), b"".join(proofs), b"".join(cts), n)
        vb = verdicts(key_b()[1], b"".join(recs), b"".join(proofs), b"".join(cts), n)
        for (t, ci), a, b in zip(owner, va, vb):
            per[t]["a" if a and not b else "b" if b and not a else "both" if a else "neither"] += 1
            if self.logs[t][ci][0] > after and not (a and not b):
                per[t]["late_not_a"] += 1
        return per, n


def case_setup():
    pk, vk = g.setup(R1CS, bytes([0xB] * 32))
    open(os.path.join(KEYS, "pk.b"), "wb").write(pk); open(os.path.join(KEYS, "vk.b"), "wb").write(vk)
    return {"pk": len(pk), "vk": len(vk)}


def case_fresh_b():
    assert g.init_algorithm(0, key_b()[0], R1CS)
    return {"proofs": prove_all(), **facts_now()}


def case_release():
    out = {"start": g.memory_info(0), "cycles": []}
    assert g.init_algorithm(0, PK_A, R1CS)
    out["init"] = facts_now(); out["describe"] = g.describe(0); out["pa"] = prove_all()
    for _ in range(3):
        c = {"scan_before": g.debug_secret_scan(0)[0]}
        c["release"] = g.release_algorithm(0)
        c["after"] = facts_now(); c["describe"] = g.describe(0)
        c["prove"] = g.prove(params(RECS[:112])).decode(); c["raw"] = g.prove_raw(0, RECS, N)[0]
        c["release_again"] = g.release_algorithm(0)
        c["init"] = g.init_algorithm(0, PK_A, R1CS)
        c["scan_after_init"] = g.debug_secret_scan(0)[0]
        c["again"] = facts_now(); c["same_proofs"] = prove_all() == out["pa"]
        out["cycles"].append(c)
    return out


def case_replace():
    pk_b, vk_b = key_b()
    assert g.init_algorithm(0, PK_A, R1CS)
    out = {"before": facts_now(), "describe_before": g.describe(0), "pa": prove_all()}
    out["rc"] = g.replace_algorithm(0, pk_b, R1CS, vk_b)
    out["after"] = facts_now(); out["describe"] = g.describe(0)
    out["stats0"] = g.prove_check_stats(0)
    out["pb"] = prove_all(); out["stats1"] = g.prove_check_stats(0)
    blob = bytes.fromhex(out["pb"]); proofs, cts = blob[:196 * N], blob[196 * N:260 * N]
    out["under_b"] = verdicts(vk_b, RECS, proofs, cts, N); out["under_a"] = verdicts(VK_A, RECS, proofs, cts, N)
    out["not_initialised"] = g.replace_algorithm(1, pk_b, R1CS)
    return out


def case_refused():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import keyraw
    pk_b, vk_b = key_b()
    bad = keyraw.rewrite_pk(pk_b, replace={("g2.B", 5): keyraw.enc_g2(keyraw.twist_point_outside_g2(), False)})
    assert g.init_algorithm(0, PK_A, R1CS)
    out = {"pa": prove_all(), "before": facts_now()}
    print("REPLACE-BEGIN", flush=True)
    out["rc"] = g.replace_algorithm(0, bad, R1CS, vk_b)
    print("REPLACE-END", flush=True)
    out["after"] = facts_now(); out["same_proofs"] = prove_all() == out["pa"]
    out["rc_bad_vk"] = g.replace_algorithm(0, pk_b, R1CS, vk_b[:100])      # a verifying key that does not parse: a refused replacement
    out["after_bad_vk"] = facts_now(); out["describe"] = g.describe(0)
    return out


def case_swaps():
    pk_b, vk_b = key_b()
    assert g.init_algorithm(0, PK_A, R1CS)
    cs = Callers(); cs.start()
    time.sleep(0.3); t_idle0 = time.monotonic(); time.sleep(0.4); t_idle1 = time.monotonic()
    w = []
    t0 = time.monotonic(); rc1 = g.replace_algorithm(0, pk_b, R1CS); w.append((t0, time.monotonic()))
    gen1 = g.key_generation(0)
    time.sleep(0.2)
    t0 = time.monotonic(); rc2 = g.replace_algorithm(0, PK_A, R1CS); w.append((t0, time.monotonic()))
    time.sleep(0.3)
    cs.finish()
    per, n = cs.judged(w + [(t_idle0, t_idle1)], w[1][1])
    return {"rc": [rc1, rc2], "gens": [gen1, g.key_generation(0)], "replace_s": [b - a for a, b in w], "idle_s": t_idle1 - t_idle0, "per": per, "proofs": n, "end": facts_now()}


def case_release_load():
    assert g.init_algorithm(0, PK_A, R1CS)
    pa = prove_all()
    cs = Callers(); cs.start()
    time.sleep(0.4)
    t0 = time.monotonic(); rc = g.release_algorithm(0); t1 = time.monotonic()
    time.sleep(0.1)
    cs.finish()
    after = facts_now()
    per, n = cs.judged([(t0, t1)], float("inf"))
    ok = g.init_algorithm(0, PK_A, R1CS)
    return {"rc": rc, "release_s": t1 - t0, "after": after, "per": per, "proofs": n, "init": ok, "same_proofs": prove_all() == pa}


def case_replicas():
    pk_b, vk_b = key_b()
    assert g.init_algorithm(0, PK_A, R1CS)
    out = {"describe0": g.describe(0)}
    prove_all(); out["served_a"] = g.served(0); out["before"] = facts_now()
    out["rc"] = g.replace_algorithm(0, pk_b, R1CS, vk_b)
    out["served_swapped"] = g.served(0); out["after"] = facts_now(); out["describe1"] = g.describe(0)
    out["pb"] = prove_all(); out["served_b"] = g.served(0)
    out["release"] = g.release_algorithm(0); out["end"] = facts_now()
    return out


if __name__ == "__main__":
    if CASE != "setup":
        g.set_deterministic_randomness(R, S, 0)
    facts = globals()["case_" + CASE]()
    json.dump(facts, open(OUT, "w"))
    print("CHILD-OK", flush=True)
