#!/usr/bin/env python3
"""Wall times of one contribution and one verification of the key ceremony's second phase (gsc_setup_contribute,
gsc_setup_verify_contribution) on the ChaCha20 pair of tests/golden and on an AES-256 pair from the oracle's Setup.

  python tools/time_ceremony.py [repeats]        (needs a GPU)
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


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
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
