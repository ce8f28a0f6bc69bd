#!/usr/bin/env python3
"""Wall times of gsc_srs_contribute and gsc_srs_verify_contribution at L = 15 and L = 17 on gsc_srs_initial's files, with the
split of a contribution between decode, powers, G1 ladders, G2 ladders and download (GSC_SRS_TRACE=1 makes the library print it; every stage
then waits for the stream, so the traced total is measured apart from the untraced one); and the per-point ladder against the uniform
k_scale_points on the same n = 131 071 G1 points (gsc_debug_scale_powers against gsc_debug_scale_points: the hooks' host work — decode and
download — is the same in both).  Medians of 5 after the first call of the process.
  GSC_ENABLE_TEST_HOOKS=1 python tools/time_srs_contribute.py [out.txt]"""
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GSC_ENABLE_TEST_HOOKS", "1")
import gsc_loader     # noqa: E402

STAGES = ("decode", "powers", "G1 ladders", "G2 ladders", "download")


def timed(f, reps=5):
    f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def traced(L):
    """the stage lines of six contributions in a child with the trace on -> the median of the last five per stage"""
    code = ("import sys; sys.path.insert(0, %r); import gsc_loader; g = gsc_loader.load(); s = g.srs_initial(%d)\n"
            "for _ in range(6): g.srs_contribute(s)\n" % (ROOT, L))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, GSC_SRS_TRACE="1"), capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        raise SystemExit("the traced child failed: %d\n%s" % (out.returncode, (out.stdout + out.stderr)[-2000:]))
    rows = [[float(v) for v in re.findall(r"([0-9.]+) ms", l)] for l in out.stdout.splitlines() if l.startswith("gsc_srs_contribute: decode ")]
    assert len(rows) == 6 and all(len(r) == len(STAGES) for r in rows), out.stdout[-2000:]
    return [statistics.median(r[i] for r in rows[1:]) for i in range(len(STAGES))]


def ladder_points(g):
    """the 4N - 1 = 131 071 G1 elements of the generator hook's L = 15 file for a fixed seed, and a fixed full-width scalar: the same inputs
    in whichever tree this runs"""
    N = 1 << 15
    f = g.debug_srs_generate(15, bytes([9] * 32))
    tau1, alpha1 = 12, 12 + 64 * (2 * N - 1) + 128 * N
    pts = f[tau1:tau1 + 64 * (2 * N - 1)] + f[alpha1:alpha1 + 64 * 2 * N]      # tauG1 | alphaG1 | betaG1
    assert len(pts) == 64 * (4 * N - 1)
    return pts, 4 * N - 1, 0x2b3a5c7d9e1f20416385a7c9ebfd0f2143658799bbddff0123456789abcdef01


def main():
    g = gsc_loader.load()
    lines = []
    for L in (15, 17):
        start = g.srs_initial(L)
        nxt, rec = g.srs_contribute(start)
        t_c = timed(lambda: g.srs_contribute(start))
        t_v = timed(lambda: g.srs_verify_contribution(start, nxt, rec))
        st = traced(L)
        lines.append("L=%d file %.1f MB: gsc_srs_contribute %.0f ms, gsc_srs_verify_contribution %.0f ms; traced contribution: %s"
                     % (L, len(start) / 1e6, t_c, t_v, ", ".join("%s %.1f ms" % p for p in zip(STAGES, st))))
        print(lines[-1], flush=True)
    pts, n, k = ladder_points(g)
    inf = bytes(n)
    t_u = timed(lambda: g.debug_scale_points(0, pts, inf, k))
    t_p = timed(lambda: g.debug_scale_powers(0, pts, inf, k, 1, 0))
    lines.append("n=%d G1 points, hooks' wall time (decode, ladder, download): uniform k_scale_points %.1f ms, k_fr_powers + per-point ladder %.1f ms (%.3f x)"
                 % (n, t_u, t_p, t_p / t_u))
    print(lines[-1], flush=True)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
