"""The quotient's live tiles on the device (k_ntt.hip launch_quotient): with folded sets the last quotient kernel runs only the
tiles that hold live table positions (ChaCha20-V3: 93 of 128, the 93rd with 64 live positions of 256) and the kernel before it stores only what
those tiles load; GSC_QUOTIENT_LIVE_TILES=0 runs and stores everything.  Proof bytes must not depend on it.

Prover processes on the golden ChaCha20 key, small tables (c = 8, batches of 64), (r, s) fixed, the other settings those of
test_gpu_quot_fold.py.  Each proves the same 64 statements; some prove 64 OTHER statements first, so that the words the kernels no longer write
hold that batch's leftovers when the batch under test runs: the proofs must equal those of a process that proved the batch alone.  The unfused
digit route (the last kernel writes d, a recoding pass follows) is selected by GSC_FUSE_Z_DIGITS=0.  Every comparison is exact equality."""
import base64
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, golden_bytes

pytestmark = pytest.mark.gpu
sys.path.insert(0, ROOT)      # bench.py: statements and public signals

N = 64
R_MOD = 21888242871839275222246405745257275088548364400416034343698204186575808495617

_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import bench, gsc_loader
g = gsc_loader.load()
algo, rows, before = int(sys.argv[6]), int(sys.argv[8]), int(sys.argv[9])
name = ["chacha20", "aes-128-ctr"][algo]
pk = open(sys.argv[7], "rb").read() if algo else bench.golden("pk.chacha20")
assert g.init_algorithm(algo, pk, bench.golden(["r1cs.chacha20", "r1cs.aes128"][algo]))
print("DESCRIBE", g.describe(algo))
n = 64
if before:      # another batch first: what the kernels do not write keeps ITS values
    other = bench.provable(bench.xoshiro_records(n, 0xBEF0 << 20), name)
    g.set_deterministic_randomness(0x7654321, 0x1357, 0x3333)
    ok, proofs, lens, cts = g.prove_raw(algo, other, n)
    assert ok == n, ok
recs = bench.provable(bench.xoshiro_records(n, 0x711E << 20), name)
g.set_deterministic_randomness(int(sys.argv[3]), int(sys.argv[4]), 0x5555)
ok, proofs, lens, cts = g.prove_raw(algo, recs, n)
assert ok == n and set(lens) == {196 if algo else 164}, (ok, set(lens))
kname, ms, stmts, cols, nb = g.last_dominant_kernel(algo)
assert kname.startswith("k_msm_win") and nb == [32768, 131072][algo], (kname, nb)      # the set's n positions, whatever is skipped
pts, flags = bytes(64 * 64), bytes(64)
if rows:
    abc = open(sys.argv[5], "rb").read()
    assert len(abc) == 3 * rows * 64 * 32
    pts, flags = g.debug_z_sum(algo, abc, rows)
open(sys.argv[2], "wb").write(recs + proofs + cts + pts + flags)
print("CHILD-OK")
"""


def _signed_rows(rng, rows):
    """a, b, c = a b: [rows][64] big-endian field elements, every entry +-1 (test_gpu_quot_fold.py's inputs)"""
    one = np.frombuffer((1).to_bytes(32, "big"), np.uint8)
    minus = np.frombuffer((R_MOD - 1).to_bytes(32, "big"), np.uint8)
    sa, sb = rng.integers(0, 2, (rows, 64), dtype=np.uint8), rng.integers(0, 2, (rows, 64), dtype=np.uint8)
    mats = [np.where(s[:, :, None] == 1, minus, one) for s in (sa, sb, sa ^ sb)]
    return np.stack(mats).astype(np.uint8).tobytes()


def _child(tmp, tag, env_extra, algo=0, pk_path="-", rows=0, before=0, abc_path="-"):
    env = {k: v for k, v in os.environ.items() if not k.startswith("GSC_")}
    env.update({"GSC_MAX_BATCH": "64", "GSC_WINDOW_Z": "8", "GSC_W_TABLE_GB": "8", "GSC_ENABLE_TEST_HOOKS": "1"})
    env.update(env_extra)
    r, s = 0x1234567, 0xabcdef0123456789abcdef
    path = str(tmp / ("out_%s.bin" % tag))
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, path, str(r), str(s), abc_path, str(algo), pk_path, str(rows), str(before)], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0 and "CHILD-OK" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
    blob = open(path, "rb").read()
    cut = [112 * N, 196 * N, 64 * N, 64 * 64, 64]
    assert len(blob) == sum(cut)
    parts, at = [], 0
    for c in cut:
        parts.append(blob[at:at + c]); at += c
    return dict(zip(("recs", "proofs", "cts", "pts", "flags"), parts), describe=[l for l in p.stdout.splitlines() if l.startswith("DESCRIBE")][0])


def _field(describe, key):
    return [w for w in describe.split() if w.startswith(key + "=")][0].split("=", 1)[1]


def _same_proofs(a, b, proof_len):
    assert a["recs"] == b["recs"] and a["cts"] == b["cts"]
    assert a["proofs"] == b["proofs"]
    assert len({a["proofs"][196 * k:196 * k + proof_len] for k in range(N)}) == N


# ---- ChaCha20-V3: L = 15, tiles of 256, 93 of 128 live -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chacha(tmp_path_factory):
    """knob on and off, each with the quotient sums of the +-1 inputs (every c_i non-zero: every live base is weighed, the 64 live positions of
    the partly live tile 92 among them)"""
    tmp = tmp_path_factory.mktemp("live_tiles")
    abc_path = str(tmp / "abc.bin")
    open(abc_path, "wb").write(_signed_rows(np.random.default_rng(0xF01D), 23617))
    return {knob: _child(tmp, "knob" + knob, {"GSC_QUOTIENT_LIVE_TILES": knob}, rows=23617, abc_path=abc_path) for knob in ("1", "0")}, tmp


def test_the_knob_changes_what_is_launched_and_says_so(chacha):
    runs, _ = chacha
    on, off = runs["1"], runs["0"]
    for r in (on, off):
        assert _field(r["describe"], "Z") == "32768" and _field(r["describe"], "Zlive") == "23616" and _field(r["describe"], "Zfold") == "dft", r["describe"]
    assert _field(on["describe"], "Qtiles") == "93/128", on["describe"]
    assert _field(off["describe"], "Qtiles") == "128/128", off["describe"]


def test_live_tiles_and_all_tiles_give_the_same_proof_bytes_and_they_verify(gsc, chacha):
    import bench
    runs, _ = chacha
    on, off = runs["1"], runs["0"]
    _same_proofs(on, off, 164)
    assert gsc.init_verifier(0, golden_bytes("vk.chacha20"))
    for k in range(N):
        rec = on["recs"][112 * k:112 * (k + 1)]
        assert gsc.verify({"cipher": "chacha20", "proof": base64.b64encode(on["proofs"][196 * k:196 * k + 164]).decode(),
                           "publicSignals": base64.b64encode(bench.signals_of("chacha20", rec, on["cts"][64 * k:64 * k + 64])).decode()}), k


def test_live_tiles_and_all_tiles_give_the_same_quotient_sums_when_every_c_is_signed_one(chacha):
    runs, _ = chacha
    on, off = runs["1"], runs["0"]
    assert on["flags"] == off["flags"] == bytes(64)                     # no column sums to the point at infinity
    assert on["pts"] == off["pts"]
    assert len({on["pts"][64 * k:64 * k + 64] for k in range(64)}) == 64      # 64 different columns, 64 different points


@pytest.mark.parametrize("route", ["fused", "unfused"])
def test_words_left_by_an_earlier_batch_are_never_read(chacha, route):
    """fused: the last kernel writes the Z digits itself (the default); unfused: GSC_FUSE_Z_DIGITS=0, it writes d and k_recode reads the live rows"""
    runs, tmp = chacha
    env = {"GSC_QUOTIENT_LIVE_TILES": "1"}
    if route == "unfused":
        env["GSC_FUSE_Z_DIGITS"] = "0"
    alone = runs["1"] if route == "fused" else _child(tmp, "alone_" + route, env)
    after = _child(tmp, "after_" + route, env, before=1)
    for r in (alone, after):
        assert _field(r["describe"], "Qtiles") == "93/128", r["describe"]
        assert ("+digits" in r["describe"]) == (route == "fused"), r["describe"]
    _same_proofs(alone, after, 164)
    _same_proofs(alone, runs["0"], 164)


def test_without_the_fold_every_tile_runs(chacha):
    runs, tmp = chacha
    plain = _child(tmp, "nofold", {"GSC_QUOTIENT_FOLD": "0", "GSC_QUOTIENT_LIVE_TILES": "1"})
    assert "Zfold=off(GSC_QUOTIENT_FOLD=0)" in plain["describe"] and _field(plain["describe"], "Qtiles") == "128/128", plain["describe"]
    _same_proofs(plain, runs["1"], 164)


# ---- AES-128-V2: L = 17, an odd Lhi, 72 KiB tiles of 512, 147 of 256 live ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def aes(aes_keys, tmp_path_factory):
    pk_path = os.path.join(ROOT, "build", "keys", "pk.aes128")
    assert os.path.exists(pk_path)
    tmp = tmp_path_factory.mktemp("live_tiles_aes")
    # (no latency layouts: these children prove one batch of 64 and share the device with the session's own algorithms)
    return {knob: _child(tmp, "aes_knob" + knob, {"GSC_QUOTIENT_LIVE_TILES": knob, "GSC_FEW_Z_GB": "0", "GSC_FEW_WIDE": "0"}, algo=1, pk_path=pk_path) for knob in ("1", "0")}


def test_aes128_live_tiles_and_all_tiles_give_the_same_proofs_and_they_verify(gsc, aes, aes_keys):
    import bench
    on, off = aes["1"], aes["0"]
    assert _field(on["describe"], "domain") == "2^17" and _field(on["describe"], "Zlive") == "74898", on["describe"]
    assert _field(on["describe"], "Qtiles") == "147/256", on["describe"]
    assert _field(off["describe"], "Qtiles") == "256/256", off["describe"]
    _same_proofs(on, off, 196)
    assert gsc.init_verifier(1, aes_keys["aes128"][2])
    items = [("aes-128-ctr", on["proofs"][196 * k:196 * k + 196], bench.signals_of("aes-128-ctr", on["recs"][112 * k:112 * (k + 1)], on["cts"][64 * k:64 * k + 64])) for k in range(N)]
    assert bench.verify_items(gsc, items) == [True] * N
