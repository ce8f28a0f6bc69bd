#!/usr/bin/env python3
"""Wall times of gsc_srs_verify and gsc_setup_from_srs beside gsc_setup, for the three circuits, on powers files from the
test hook (L = 15 for ChaCha20-V3, 17 for the AES circuits): medians of 5 after the first call of the process.  GSC_SETUP_TRACE=1 makes
gsc_setup_from_srs print its stages (file check, transforms, column sums, the rest) and the column histogram of each matrix.
  GSC_ENABLE_TEST_HOOKS=1 python tools/time_srs_setup.py [out.txt]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GSC_ENABLE_TEST_HOOKS", "1")
import bench          # noqa: E402
import gsc_loader     # noqa: E402


def timed(f, reps=5):
    f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    g = gsc_loader.load()
    seed = bytes([9] * 32)
    lines = []
    for name, L in (("chacha20", 15), ("aes128", 17), ("aes256", 17)):
        r1cs = bench.golden("r1cs." + name)
        srs = g.debug_srs_generate(L, seed)
        lines.append("%-9s L=%d file %.1f MB: gsc_srs_verify %.0f ms, gsc_setup_from_srs (production) %.0f ms, (seeded) %.0f ms, gsc_setup (seeded) %.0f ms"
                     % (name, L, len(srs) / 1e6, timed(lambda: g.srs_verify(srs)), timed(lambda: g.setup_from_srs(r1cs, srs)),
                        timed(lambda: g.setup_from_srs(r1cs, srs, seed)), timed(lambda: g.setup(r1cs, seed))))
        print(lines[-1], flush=True)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
