"""The quotient fold on the device (k_quot_bases.hip): GSC_QUOTIENT_FOLD=1 drops the n - m + 1 = 9 152 Z bases that the
domain's zero padding makes redundant and folds them into U and the live V — by the three group transforms of launch_quot_fold_dft, the
fold's only route — and the sums, hence the proof bytes, must not change.

Two prover processes on the golden ChaCha20 key, fold on and off, small tables (c = 8), (r, s) fixed; each proves the same 64 statements and
evaluates the quotient sum of 64 columns of caller-supplied a, b with entries +-1 on every row < m (gsc_debug_z_sum): proofs never multiply
a U'_i by anything but the c_i of a real witness, three quarters of which are zero — here every c_i is +-1, so every folded base is weighed.
Both comparisons are exact equality."""
import base64
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, golden_bytes

pytestmark = pytest.mark.gpu

N, M_ROWS, DOMAIN = 64, 23617, 32768
R_MOD = 21888242871839275222246405745257275088548364400416034343698204186575808495617

_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import bench, gsc_loader
g = gsc_loader.load()
assert g.init_algorithm(0, bench.golden("pk.chacha20"), bench.golden("r1cs.chacha20"))
print("DESCRIBE", g.describe(0))
n = 64
recs = bench.xoshiro_records(n, 0xF01D << 20)
g.set_deterministic_randomness(int(sys.argv[3]), int(sys.argv[4]), 0)
ok, proofs, lens, cts = g.prove_raw(0, recs, n)
assert ok == n and set(lens) == {164}, (ok, set(lens))
name, ms, stmts, cols, nb = g.last_dominant_kernel(0)
assert name.startswith("k_msm_win") and nb == 32768, (name, nb)      # the set's n positions, folded or not
abc = open(sys.argv[5], "rb").read()
pts, flags = g.debug_z_sum(0, abc, len(abc) // (3 * 64 * 32))
open(sys.argv[2], "wb").write(recs + proofs + cts + pts + flags)
print("CHILD-OK")
"""


def _signed_rows(rng):
    """a, b, c = a b: [m][64] big-endian field elements, every entry +-1"""
    one = np.frombuffer((1).to_bytes(32, "big"), np.uint8)
    minus = np.frombuffer((R_MOD - 1).to_bytes(32, "big"), np.uint8)
    sa, sb = rng.integers(0, 2, (M_ROWS, 64), dtype=np.uint8), rng.integers(0, 2, (M_ROWS, 64), dtype=np.uint8)
    mats = [np.where(s[:, :, None] == 1, minus, one) for s in (sa, sb, sa ^ sb)]
    return np.stack(mats).astype(np.uint8).tobytes()


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    sys.path.insert(0, ROOT)
    tmp = tmp_path_factory.mktemp("fold")
    abc_path = str(tmp / "abc.bin")
    open(abc_path, "wb").write(_signed_rows(np.random.default_rng(0xF01D)))
    r, s = 0x1234567, 0xabcdef0123456789abcdef
    out = {}
    for fold in ("1", "0"):
        env = {k: v for k, v in os.environ.items() if not k.startswith("GSC_")}
        env.update({"GSC_MAX_BATCH": "64", "GSC_WINDOW_Z": "8", "GSC_W_TABLE_GB": "8", "GSC_ENABLE_TEST_HOOKS": "1", "GSC_QUOTIENT_FOLD": fold})
        path = str(tmp / ("out%s.bin" % fold))
        p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, path, str(r), str(s), abc_path], env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0 and "CHILD-OK" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
        blob = open(path, "rb").read()
        cut = [112 * N, 196 * N, 64 * N, 64 * 64, 64]
        assert len(blob) == sum(cut)
        parts, at = [], 0
        for c in cut:
            parts.append(blob[at:at + c]); at += c
        out[fold] = dict(zip(("recs", "proofs", "cts", "pts", "flags"), parts), describe=[l for l in p.stdout.splitlines() if l.startswith("DESCRIBE")][0])
    return out


def test_folded_and_unfolded_sets_give_the_same_proof_bytes(gsc, runs):
    sys.path.insert(0, ROOT)
    import bench
    on, off = runs["1"], runs["0"]
    assert " Z=32768 " in on["describe"] and "Zlive=23616" in on["describe"], on["describe"]
    assert " Z=32768 " in off["describe"] and "Zlive" not in off["describe"] and "Zfold=off(GSC_QUOTIENT_FOLD=0)" in off["describe"], off["describe"]
    assert on["recs"] == off["recs"] and on["cts"] == off["cts"]
    assert on["proofs"] == off["proofs"]
    assert len({on["proofs"][196 * k:196 * k + 164] for k in range(N)}) == N
    assert gsc.init_verifier(0, golden_bytes("vk.chacha20"))
    for k in range(N):
        rec = on["recs"][112 * k:112 * (k + 1)]
        assert gsc.verify({"cipher": "chacha20", "proof": base64.b64encode(on["proofs"][196 * k:196 * k + 164]).decode(),
                           "publicSignals": base64.b64encode(bench.signals_of("chacha20", rec, on["cts"][64 * k:64 * k + 64])).decode()}), k


def test_folded_and_unfolded_quotient_sums_agree_when_every_c_is_signed_one(runs):
    on, off = runs["1"], runs["0"]
    assert on["flags"] == off["flags"] == bytes(64)                     # no column sums to the point at infinity
    assert on["pts"] == off["pts"]
    assert len({on["pts"][64 * k:64 * k + 64] for k in range(64)}) == 64      # 64 different columns, 64 different points
