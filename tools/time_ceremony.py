#!/usr/bin/env python3
"""Wall times of one contribution and one verification of the key ceremony's second phase (gsc_setup_contribute,
gsc_setup_verify_contribution) on the ChaCha20 pair of tests/golden and on an AES-256 pair from the oracle's Setup.

  python tools/time_ceremony.py [repeats]        (needs a GPU)
  python tools/time_ceremony.py [repeats] --sigma
      the sigma calls instead on AES-128 and AES-256 pairs: gsc_setup_contribute_sigma, gsc_setup_verify_sigma_contribution,
      gsc_pedersen_verify and, on a production pair from an L = 17 powers file (gsc_debug_srs_generate: test hooks), gsc_setup_verify_from_srs
The first call of a process pays the runtime's start and the code-object load; it is reported apart from the repeats that follow."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench          # noqa: E402
import gsc_loader     # noqa: E402


def pairs():
    from oracle import oracle as O
    yield "chacha20", bench.golden("pk.chacha20"), bench.golden("vk.chacha20")
    pk, vk = O.setup(O.R1CS(bench.golden("r1cs.aes256")), bytes([2] * 32))
    yield "aes-256-ctr", pk, vk


def timed(reps, call):
    """wall times of reps + 1 calls: the first, then the others"""
    t = []
    for _ in range(reps + 1):
        t0 = time.perf_counter(); out = call(); t.append(time.perf_counter() - t0)
        assert out
    return t, out


def line(what, t, reps):
    ms = lambda v: "%.1f" % (1e3 * v)
    print("  %-16s first %s ms, then min %s / median %s / max %s ms over %d" % (what, ms(t[0]), ms(min(t[1:])), ms(sorted(t[1:])[reps // 2]), ms(max(t[1:])), reps))


def sigma(reps):
    os.environ.setdefault("GSC_ENABLE_TEST_HOOKS", "1")      # the powers file of the last figure comes from a test hook
    from oracle import oracle as O
    g = gsc_loader.load()
    srs = g.debug_srs_generate(17, bytes([61] * 32))
    for name, tag, algo in (("aes-128-ctr", "aes128", 1), ("aes-256-ctr", "aes256", 2)):
        r1cs = bench.golden("r1cs." + tag)
        pk, vk = O.setup(O.R1CS(r1cs), bytes([algo] * 32))
        print("%s: pk %d bytes, vk %d bytes" % (name, len(pk), len(vk)))
        tc, step = timed(reps, lambda: g.setup_contribute_sigma(pk, vk))
        line("contribute", tc, reps)
        line("verify link", timed(reps, lambda: g.setup_verify_sigma_contribution(pk, vk, *step))[0], reps)
        line("pedersen_verify", timed(reps, lambda: g.pedersen_verify(step[0], step[1]))[0], reps)
        ppk, pvk = g.setup_from_srs(r1cs, srs)
        line("verify_from_srs", timed(reps, lambda: g.setup_verify_from_srs(r1cs, srs, ppk, pvk))[0], reps)


def main():
    args = [a for a in sys.argv[1:] if a != "--sigma"]
    reps = int(args[0]) if args else 5
    if "--sigma" in sys.argv[1:]:
        return sigma(reps)
    g = gsc_loader.load()
    for name, pk, vk in pairs():
        tc, tv = [], []
        for _ in range(reps + 1):
            t0 = time.perf_counter(); pk2, vk2, rec = g.setup_contribute(pk, vk); t1 = time.perf_counter()
            ok = g.setup_verify_contribution(pk, vk, pk2, vk2, rec); t2 = time.perf_counter()
            assert ok
            tc.append(t1 - t0); tv.append(t2 - t1)
        ms = lambda v: "%.1f" % (1e3 * v)
        print("%s: pk %d bytes, vk %d bytes" % (name, len(pk), len(vk)))
        print("  contribute  first %s ms, then min %s / median %s / max %s ms over %d" % (ms(tc[0]), ms(min(tc[1:])), ms(sorted(tc[1:])[reps // 2]), ms(max(tc[1:])), reps))
        print("  verify      first %s ms, then min %s / median %s / max %s ms over %d" % (ms(tv[0]), ms(min(tv[1:])), ms(sorted(tv[1:])[reps // 2]), ms(max(tv[1:])), reps))


if __name__ == "__main__":
    main()
