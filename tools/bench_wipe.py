"""Fill rate of k_wipe alone: one descriptor over a whole buffer through the test hook gsc_debug_wipe (device time of the launch, HIP events),
then the column form of a latency-path call.  usage: GSC_ENABLE_TEST_HOOKS=1 python tools/bench_wipe.py [GiB] [repeats]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gsc_loader

g = gsc_loader.load()
gib = int(sys.argv[1]) if len(sys.argv) > 1 else 4
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
n = gib << 30
for k in range(reps):
    _, counts, ms = g.debug_wipe(n, 0xA5, [(0, 1, n, n)], windows=[(0, 1, n, n)], want_buffer=False)
    assert counts == [0]
    print("fill %d GiB: %.3f ms  %.0f GB/s" % (gib, ms, n / ms / 1e6), flush=True)
# 61 000 + 3 x 32 768 rows of 2 KiB, columns < n: what one Prove clears of W, a, b, c when it wrote its own columns only
rows = 61000 + 3 * 32768
for cols in (1, 5, 32, 64):
    _, counts, ms = g.debug_wipe(rows * 2048, 0xA5, [(0, rows, 2048, 32 * cols)], windows=[(0, rows, 2048, 32 * cols)], want_buffer=False)
    assert counts == [0]
    print("columns < %2d of %d rows of 2 KiB: %.3f ms" % (cols, rows, ms), flush=True)
