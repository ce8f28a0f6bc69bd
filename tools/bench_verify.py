"""Times the GPU verifier (gsc_verify_raw in libprove.so) against libverify.so's Verify on up to 16 host threads.

Proofs come from gsc_prove_raw.  One JSON line per configuration: ChaCha20 at n = 1024, 8192, 65536 and AES-128 at 8192.  Every GPU
verdict is checked (all proofs valid must be accepted; the same proofs with the signals of the next statement must be rejected), and
the CPU rate is measured on a sample of the same proofs with the same check.

    python tools/bench_verify.py [--sizes 1024,8192,65536] [--aes 8192] [--cpu-sample 2048] [--out FILE]

--batched times gsc_verify_raw_batched (one final exponentiation per chunk) against gsc_verify_raw on the same all-valid proofs
instead, each the median of --repeat calls, and checks that the verdicts are equal.  One more ChaCha20 line at the largest size has a
single bad proof (signals of another statement): the price of the proof-by-proof pass that follows a failing chunk.

--latency times single calls from one proof upwards: for ChaCha20 and AES-128 and every size of --sizes (honoured down to 1, e.g.
1,8,64,512,4096,8192,32768,65536), the median of --repeat (at least 5) calls of gsc_verify_raw, and of gsc_verify_raw_batched and
gsc_verify_all too with --batched, in milliseconds and proofs/s, with libverify.so's single-thread milliseconds per proof beside n = 1.  --path thread / few forces the
per-thread or the few-proof kernels through gsc_debug_verify_path (auto: the library routes by GSC_VERIFY_FEW_MAX; a comma-separated
list measures one after the other on the same proofs); --label names
the build in every line, and --lib-root measures the library of another checkout (the parent commit) with this tool.

    python tools/bench_verify.py --latency --sizes 1,8,64,512,4096,8192 --path few [--batched] [--label change] [--out FILE]

--claims S[,S...] times gsc_verify_claims (one equation and one final exponentiation per claim) against gsc_verify_raw and
gsc_verify_raw_batched on the same items: for ChaCha20 at every size of --sizes (default 8192,65536) and AES-128 at --aes, the items cut
into claims of S proofs, once all valid and once with one bad proof (signals of another statement) in 1 % of the claims; ms per call,
the median of --repeat (at least 5) calls after 2.  Measured on one MI355X (profiles/r09_bench_verify_claims.jsonl, DESIGN.md
§10): at 65 536 ChaCha20 proofs per call gsc_verify_claims beats gsc_verify_raw from claims of 8 proofs (1.17x; 64: 1.26x; sizes
between 1 and 8 were not measured) and is slower for claims of one proof (0.66x); at 8192 per call it is slower for ChaCha20 at every
measured size and level with gsc_verify_raw for AES-128 from 8.

    python tools/bench_verify.py --claims 1,8,64 [--sizes 8192,65536] [--aes 8192] [--out FILE]
"""
import argparse
import json
import os
import random
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import golden_bytes  # noqa: E402

NAMES = {0: "chacha20", 1: "aes-128-ctr"}
THREADS = 16
SIZES_DEFAULT = "1024,8192,65536"


def make_items(g, algo, n, seed):
    rnd = random.Random(seed)
    recs = b"".join(rnd.randbytes(32) + rnd.randbytes(12) + rnd.getrandbits(31).to_bytes(4, "little") + rnd.randbytes(64) for _ in range(n))
    proofs, lens, cts = g.raw_buffers(n)
    done = 0
    while done < n:                                   # prove in calls of at most 16384 statements
        m = min(16384, n - done)
        sub = g.raw_buffers(m)
        assert g.prove_raw_into(algo, recs[112 * done:112 * (done + m)], m, *sub) == m
        proofs[196 * done:196 * (done + m)] = sub[0].raw
        for k in range(m):
            lens[done + k] = sub[1][k]
        cts[64 * done:64 * (done + m)] = sub[2].raw
        done += m
    sig = bytearray()
    for k in range(n):
        rec = recs[112 * k:112 * k + 112]
        ctr = rec[44:48] if algo == 0 else rec[44:48][::-1]
        sig += cts.raw[64 * k:64 * k + 64] + rec[32:44] + ctr + rec[48:]
    return proofs.raw, list(lens), bytes(sig)


def run(g, algo, n, cpu_sample, seed):
    proofs, lens, sig = make_items(g, algo, n, seed)
    g.verify_raw(algo, proofs[:196 * 64], lens[:64], sig[:144 * 64])          # warm-up (kernel load)
    t0 = time.perf_counter()
    v = g.verify_raw(algo, proofs, lens, sig)
    gpu_s = time.perf_counter() - t0
    shifted = sig[144:] + sig[:144]
    w = g.verify_raw(algo, proofs, lens, shifted)
    ok = v == [1] * n and w == [0] * n
    m = min(cpu_sample, n)
    items = [{"cipher": NAMES[algo], "proof": list(proofs[196 * k:196 * k + lens[k]]), "publicSignals": list(sig[144 * k:144 * k + 144])} for k in range(m)]
    enc = [json.dumps(it).encode() for it in items]
    t0 = time.perf_counter()
    with ThreadPoolExecutor(THREADS) as ex:
        cpu = list(ex.map(g.verify, enc))
    cpu_s = time.perf_counter() - t0
    ok = ok and all(cpu)
    return {"tool": "bench_verify", "cipher": NAMES[algo], "n": n, "gpu_s": round(gpu_s, 4), "gpu_proofs_per_s": round(n / gpu_s, 1),
            "cpu_threads": THREADS, "cpu_sample": m, "cpu_proofs_per_s": round(m / cpu_s, 1), "speedup": round((n / gpu_s) / (m / cpu_s), 1),
            "verdicts_ok": ok, "device": os.environ.get("GSC_DEVICE", "0")}


def _median_call(fn, repeat):
    times, out = [], None
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return sorted(times)[len(times) // 2], out


def run_batched(g, algo, n, seed, repeat, bad=None):
    proofs, lens, sig = make_items(g, algo, n, seed)
    if bad is not None:                               # item `bad` gets the signals of the next statement
        sig = sig[:144 * bad] + sig[144 * (bad + 1):144 * (bad + 2)] + sig[144 * (bad + 1):]
    g.verify_raw(algo, proofs[:196 * 64], lens[:64], sig[:144 * 64])          # warm-up (kernel load)
    g.verify_raw_batched(algo, proofs[:196 * 64], lens[:64], sig[:144 * 64])
    plain_s, want = _median_call(lambda: g.verify_raw(algo, proofs, lens, sig), repeat)
    batched_s, got = _median_call(lambda: g.verify_raw_batched(algo, proofs, lens, sig), repeat)
    expect = [1] * n
    if bad is not None:
        expect[bad] = 0
    ok = got == want == expect and g.verify_all(algo, proofs, lens, sig) == (1 if bad is None else 0)
    return {"tool": "bench_verify", "mode": "batched", "cipher": NAMES[algo], "n": n, "bad": 0 if bad is None else 1,
            "plain_s": round(plain_s, 4), "plain_proofs_per_s": round(n / plain_s, 1), "batched_s": round(batched_s, 4),
            "batched_proofs_per_s": round(n / batched_s, 1), "speedup": round(plain_s / batched_s, 2), "repeat": repeat,
            "verdicts_ok": ok, "device": os.environ.get("GSC_DEVICE", "0")}


def run_latency(g, algo, items, n, repeat, entry, path, label):
    proofs, lens, sig = items[0][:196 * n], items[1][:n], items[2][:144 * n]
    batched = entry == "gsc_verify_all"
    fn = {"gsc_verify_raw": g.verify_raw, "gsc_verify_raw_batched": g.verify_raw_batched, "gsc_verify_all": g.verify_all}[entry]
    call = lambda: fn(algo, proofs, lens, sig)
    call(); call()                                    # warm-up: kernel load, clocks
    med, out = _median_call(call, repeat)
    line = {"tool": "bench_verify", "mode": "latency", "build": label, "entry": entry,
            "cipher": NAMES[algo], "n": n, "path": path, "ms": round(1e3 * med, 3), "proofs_per_s": round(n / med, 1), "repeat": repeat,
            "verdicts_ok": out == (1 if batched else [1] * n), "device": os.environ.get("GSC_DEVICE", "0")}
    if hasattr(g, "verify_last_path"):
        line["last_path"] = g.verify_last_path(algo)
    if n == 1:
        enc = json.dumps({"cipher": NAMES[algo], "proof": list(proofs[:lens[0]]), "publicSignals": list(sig)}).encode()
        cpu, ok = _median_call(lambda: g.verify(enc), repeat)
        line["cpu_1thread_ms"] = round(1e3 * cpu, 3)
        line["verdicts_ok"] = line["verdicts_ok"] and bool(ok)
    return line


def run_claims(g, algo, items, n, size, bad, repeat, label):
    proofs, lens, sig = items[0][:196 * n], items[1][:n], items[2][:144 * n]
    ends = list(range(size, n, size)) + [n]
    m = len(ends)
    want = [1] * n
    if bad:                                           # in 1 % of the claims one item gets the signals of the next statement
        rnd = random.Random(size)
        sigb = bytearray(sig)
        for c in rnd.sample(range(m), max(1, m // 100)):
            lo = ends[c - 1] if c else 0
            i = rnd.randrange(lo, ends[c])
            j = (i + 1) % n
            sigb[144 * i:144 * i + 144] = sig[144 * j:144 * j + 144]
            want[i] = 0
        sig = bytes(sigb)
    want_claims = [int(all(want[a:b])) for a, b in zip([0] + ends[:-1], ends)]
    line = {"tool": "bench_verify", "mode": "claims", "build": label, "cipher": NAMES[algo], "n": n, "claim_size": size, "claims": m,
            "bad_claims": m - sum(want_claims), "repeat": repeat, "device": os.environ.get("GSC_DEVICE", "0")}
    ok = True
    for entry, fn, expect in (("claims", lambda: g.verify_claims(algo, proofs, lens, sig, ends), want_claims),
                              ("raw", lambda: g.verify_raw(algo, proofs, lens, sig), want),
                              ("batched", lambda: g.verify_raw_batched(algo, proofs, lens, sig), want)):
        fn(); fn()                                    # warm-up: kernel load, buffers, clocks
        med, out = _median_call(fn, repeat)
        line[entry + "_ms"] = round(1e3 * med, 3)
        ok = ok and out == expect
    line["claims_vs_raw"] = round(line["raw_ms"] / line["claims_ms"], 2)
    line["claims_vs_batched"] = round(line["batched_ms"] / line["claims_ms"], 2)
    line["last_path"] = g.verify_last_path(algo)
    line["verdicts_ok"] = ok
    return line


def main_claims(g, a):
    claim_sizes = [int(x) for x in a.claims.split(",") if x]
    sizes = sorted(int(x) for x in (a.sizes if a.sizes != SIZES_DEFAULT else "8192,65536").split(",") if x)
    lines = []
    for algo in (0, 1):
        if algo == 0:
            pk, r1cs, vk = golden_bytes("pk.chacha20"), golden_bytes("r1cs.chacha20"), golden_bytes("vk.chacha20")
            ns = sizes
        elif a.aes:
            pk, r1cs, vk = aes128_keys()
            ns = [a.aes]
        else:
            continue
        assert g.init_algorithm(algo, pk, r1cs) and g.verify_init(algo, vk)
        items = make_items(g, algo, max(ns), 11 + algo)         # one set of proofs; size n takes the first n
        for n in ns:
            for size in claim_sizes:
                for bad in (False, True):
                    lines.append(run_claims(g, algo, items, n, size, bad, max(5, a.repeat), a.label)); print(json.dumps(lines[-1]), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")
    return 0 if all(l["verdicts_ok"] for l in lines) else 1


def aes128_keys():
    cache = os.path.join(ROOT, "build", "keys")
    pkp, vkp = os.path.join(cache, "pk.aes128"), os.path.join(cache, "vk.aes128")
    r1cs = golden_bytes("r1cs.aes128")
    if not (os.path.exists(pkp) and os.path.exists(vkp)):       # the test suite's AES-128 test keys (same seed, same cache)
        from oracle import oracle as O
        os.makedirs(cache, exist_ok=True)
        pk, vkb = O.setup(O.R1CS(r1cs), bytes([1] * 32))
        open(pkp, "wb").write(pk); open(vkp, "wb").write(vkb)
    return open(pkp, "rb").read(), r1cs, open(vkp, "rb").read()


def main_latency(g, a):
    sizes = sorted(int(x) for x in a.sizes.split(",") if x)
    modes = {"auto": 0, "thread": 1, "few": 2}
    paths = [p for p in a.path.split(",") if p]
    for p in paths:
        if p not in modes or (modes[p] and (not hasattr(g, "debug_verify_path") or g.debug_verify_path(0) != 0)):
            raise SystemExit("--path %s needs gsc_debug_verify_path (test hooks on, a build that has it)" % p)
    lines = []
    for algo in (0, 1):
        if algo == 0:
            pk, r1cs, vk = golden_bytes("pk.chacha20"), golden_bytes("r1cs.chacha20"), golden_bytes("vk.chacha20")
        elif a.aes:
            pk, r1cs, vk = aes128_keys()
        else:
            continue
        assert g.init_algorithm(algo, pk, r1cs) and g.verify_init(algo, vk) and g.init_verifier(algo, vk)
        items = make_items(g, algo, max(sizes), 11 + algo)      # one set of proofs; size n takes the first n
        for p in paths:
            if modes[p] or len(paths) > 1:
                g.debug_verify_path(modes[p])
            for entry in (["gsc_verify_raw", "gsc_verify_raw_batched", "gsc_verify_all"] if a.batched else ["gsc_verify_raw"]):
                for n in sizes:
                    lines.append(run_latency(g, algo, items, n, max(5, a.repeat), entry, p, a.label)); print(json.dumps(lines[-1]), flush=True)
        if hasattr(g, "debug_verify_path"):
            g.debug_verify_path(0)
    if a.out:
        with open(a.out, "a") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")
    return 0 if all(l["verdicts_ok"] for l in lines) else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=SIZES_DEFAULT)
    ap.add_argument("--aes", type=int, default=8192, help="AES-128 batch (0: skip)")
    ap.add_argument("--cpu-sample", type=int, default=2048)
    ap.add_argument("--out", default=None)
    ap.add_argument("--batched", action="store_true", help="gsc_verify_raw_batched against gsc_verify_raw")
    ap.add_argument("--repeat", type=int, default=3, help="--batched: calls per timing (median)")
    ap.add_argument("--latency", action="store_true", help="per-call milliseconds from n = 1 upwards (with --batched: gsc_verify_raw_batched and gsc_verify_all too)")
    ap.add_argument("--path", default="auto", help="--latency: auto, thread, few or several, e.g. auto,thread,few: force the verifier's kernels (test hook)")
    ap.add_argument("--claims", default=None, help="claim sizes, e.g. 1,8,64: gsc_verify_claims against gsc_verify_raw and gsc_verify_raw_batched")
    ap.add_argument("--label", default="change", help="--latency: name of the measured build in every line")
    ap.add_argument("--lib-root", default=ROOT, help="checkout whose library is measured (default: this one)")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.lib_root))
    import gsc_loader
    g = gsc_loader.load()
    if a.latency:
        return main_latency(g, a)
    if a.claims:
        return main_claims(g, a)
    lines = []
    assert g.init_algorithm(0, golden_bytes("pk.chacha20"), golden_bytes("r1cs.chacha20"))
    vk = golden_bytes("vk.chacha20")
    assert g.verify_init(0, vk) and g.init_verifier(0, vk)
    sizes = [int(x) for x in a.sizes.split(",") if x]
    for n in sizes:
        lines.append(run_batched(g, 0, n, n, a.repeat) if a.batched else run(g, 0, n, a.cpu_sample, n)); print(json.dumps(lines[-1]), flush=True)
    if a.batched and sizes:
        n = max(sizes)
        lines.append(run_batched(g, 0, n, n, a.repeat, bad=n // 2)); print(json.dumps(lines[-1]), flush=True)
    if a.aes:
        cache = os.path.join(ROOT, "build", "keys")
        pkp, vkp = os.path.join(cache, "pk.aes128"), os.path.join(cache, "vk.aes128")
        r1cs = golden_bytes("r1cs.aes128")
        if not (os.path.exists(pkp) and os.path.exists(vkp)):       # the test suite's AES-128 test keys (same seed, same cache)
            from oracle import oracle as O
            os.makedirs(cache, exist_ok=True)
            pk, vkb = O.setup(O.R1CS(r1cs), bytes([1] * 32))
            open(pkp, "wb").write(pk); open(vkp, "wb").write(vkb)
        pk, vkb = open(pkp, "rb").read(), open(vkp, "rb").read()
        assert g.init_algorithm(1, pk, r1cs) and g.verify_init(1, vkb) and g.init_verifier(1, vkb)
        lines.append(run_batched(g, 1, a.aes, 7, a.repeat) if a.batched else run(g, 1, a.aes, min(a.cpu_sample, 1024), 7)); print(json.dumps(lines[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")
    return 0 if all(l["verdicts_ok"] for l in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
