"""A finished call leaves NOTHING key-derived in device memory.  tests/test_gpu_secrets.py looks where the old wipe wrote (the key wires, r, s,
the input records); the witness of these circuits is a cipher key and every buffer behind it gives it away (ChaCha20's first add32 bits are a
key word plus a constant, the AES S-box inputs key XOR public data): the other rows of W and the byte planes, a / b / c, the quotient's
intermediates, the signed digits, the partial sums.  The engine brings every secret region of a lane (csrc/wipe_plan.hpp: every device
allocation but results, verdicts and timing words) back to its idle image — phase A beside the Z sum, phase B behind the assembly, everything
over the whole allocation when a call leaves by an exception — and gsc_debug_secret_scan counts, on the device and over the whole allocations,
the bytes that differ from it.  One child process per configuration (the knobs are read once per process), small tables."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

PUBLIC = ["out", "flags", "status", "cpts", "clk", "fsync", "wsflag"]

_CHILD = r"""
import base64, json, sys
sys.path.insert(0, sys.argv[1])
import bench, gsc_loader
g = gsc_loader.load()
algo, name, mode = int(sys.argv[2]), sys.argv[3], sys.argv[4]
if algo == 0:
    pk, vk = bench.golden("pk.chacha20"), bench.golden("vk.chacha20")
else:
    pk, vk = g.setup(bench.golden("r1cs." + name), bench.SETUP_SEEDS[name])
assert g.init_algorithm(algo, pk, bench.golden("r1cs." + name))
print("DESCRIBE", g.describe(algo))
cipher, kl = bench.ALGOS[name][1], bench.ALGOS[name][2]
scans = []
def scan(what):
    total, dirty, info = g.debug_secret_scan(algo)
    scans.append([what, total, dirty, info])
    return total
def records(n):
    return bench.provable(bench.xoshiro_records(n, (0x5EC << 20) + n), name)
def verified(recs, proofs, lens, cts, n):
    assert g.init_verifier(algo, vk)
    for k in range(n):
        item = {"cipher": cipher, "proof": base64.b64encode(proofs[196 * k:196 * k + lens[k]]).decode(),
                "publicSignals": base64.b64encode(bench.signals_of(name, recs[112 * k:112 * k + 112], cts[64 * k:64 * k + 64])).decode()}
        if not g.verify(item):
            return False
    return True
def prove_json(rec):
    out = g.prove({"cipher": cipher, "key": list(rec[:kl]), "nonce": list(rec[32:44]), "counter": int.from_bytes(rec[44:48], "little"), "input": list(rec[48:112])})
    return out if isinstance(out, bytes) else out.encode()

scan("init")
if mode == "plain":
    for n in (1, 5, 64, 200, 300, 200, 1):      # ... 300: two chunks with different row strides on one lane; 200 then 1: a smaller call after a larger one
        recs = records(n)
        ok, proofs, lens, cts = g.prove_raw(algo, recs, n)
        assert ok == n, (n, ok)
        scan("raw %d" % n)
    assert b"proofJson" in prove_json(recs[:112])
    scan("json")
    print("LEGACY", g.debug_secret_residue(algo))
elif mode == "fixed":      # 64 fixed statements, fixed randomness: the proofs, and whether libverify.so accepts them
    recs = records(64)
    g.set_deterministic_randomness(0x1234567, 0xabcdef0123456789abcdef, 0x77)
    ok, proofs, lens, cts = g.prove_raw(algo, recs, 64)
    g.set_deterministic_randomness(None)
    assert ok == 64
    scan("raw 64")
    print("LEGACY", g.debug_secret_residue(algo))
    print("PROOFS", proofs.hex())
    print("VERIFIED", verified(recs, proofs, lens, cts, 64))
elif mode == "batch":      # one batch call, then the scan (GSC_KEEP_SECRETS: what the wipe would have removed)
    recs = records(200)
    ok, proofs, lens, cts = g.prove_raw(algo, recs, 200)
    assert ok == 200
    scan("raw 200")
elif mode == "fail":       # GSC_FAIL_AFTER_STAGE: every call fails, in the shape failures have, and leaves nothing
    for n in (70, 3):
        recs = records(n)
        ok, proofs, lens, cts = g.prove_raw(algo, recs, n)
        print("RAW", n, ok)
        scan("failed raw %d" % n)
    out = prove_json(recs[:112])
    print("JSONFAIL", b"proofJson" not in out, out[:200])
    scan("failed json")
elif mode == "after":      # the knob cleared: the same calls prove and verify
    for n in (70, 3):
        recs = records(n)
        ok, proofs, lens, cts = g.prove_raw(algo, recs, n)
        assert ok == n
        print("VERIFIED", n, verified(recs, proofs, lens, cts, n))
        scan("raw %d" % n)
print("DESCRIBE_END", g.describe(algo))
print("SCANS", json.dumps(scans))
print("CHILD-OK")
"""


def _run(algo, name, mode, extra=None):
    env = {k: v for k, v in os.environ.items() if not k.startswith("GSC_")}
    env.update({"GSC_ENABLE_TEST_HOOKS": "1", "GSC_MAX_BATCH": "256", "GSC_WINDOW_Z": "8", "GSC_WINDOW_W": "8", "GSC_W_TABLE_GB": "8", "GSC_FEW_Z_GB": "3", "GSC_FEW_WIDE": "0"})
    env.update(extra or {})
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(algo), name, mode], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0 and "CHILD-OK" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
    out = {"stdout": p.stdout}
    for line in p.stdout.splitlines():
        key, _, rest = line.partition(" ")
        if key == "SCANS":
            import json
            out["scans"] = json.loads(rest)
        elif key in ("DESCRIBE", "DESCRIBE_END", "LEGACY", "PROOFS"):
            out[key.lower()] = rest
        elif key in ("VERIFIED", "RAW", "JSONFAIL"):
            out.setdefault(key.lower(), []).append(rest)
    return out


def _assert_clean(run):
    for what, total, dirty, info in run["scans"]:
        print(what, total, dirty)
        assert total == 0 and dirty == {}, (what, total, dirty)
        assert info["registered"] == info["allocated"] > 0, (what, info)
        assert info["public"] == PUBLIC, info


PLAIN = [(0, "chacha20", {}),
         (0, "chacha20", {"GSC_SMALL_WITNESS": "0", "GSC_QUOTIENT_EVAL": "0"}),
         (0, "chacha20", {"GSC_SMALL_WITNESS": "2"}),      # every chunk falls back in-call: both attempts wipe what they wrote
         (0, "chacha20", {"GSC_FUSE_Z_DIGITS": "0"}),
         (1, "aes128", {})]


@pytest.mark.parametrize("algo,name,extra", PLAIN, ids=["chacha20", "chacha20-generic-coefficient", "chacha20-fallback", "chacha20-unfused", "aes128"])
def test_every_secret_region_is_idle_after_init_and_after_every_call(algo, name, extra):
    run = _run(algo, name, "plain", extra)
    assert " wipe=full " in run["describe"], run["describe"]
    assert [s[0] for s in run["scans"]] == ["init", "raw 1", "raw 5", "raw 64", "raw 200", "raw 300", "raw 200", "raw 1", "json"]
    _assert_clean(run)
    assert run["legacy"] == "0"
    if extra.get("GSC_SMALL_WITNESS") == "2":      # the fallback was really taken
        assert "fallbacks 0)" in run["describe"] and "fallbacks 0)" not in run["describe_end"], run["describe_end"]


def test_the_scan_sees_what_the_wipe_removes():
    run = _run(0, "chacha20", "batch", {"GSC_KEEP_SECRETS": "1"})
    assert " wipe=off " in run["describe"]
    what, total, dirty, info = run["scans"][-1]
    names = {k.split(".", 1)[1] for k in dirty}
    print(total, dirty)
    assert {"W", "A", "B", "digits", "W8", "A8", "B8", "C8"} <= names, names
    assert names & {"part1a", "part1b", "part2a", "part2b"}, names
    assert total > 1_000_000
    assert run["scans"][0][1] == 0      # ... and nothing before the first call


def test_old_wipe_leaves_the_key_recoverable_and_proofs_do_not_depend_on_the_wipe():
    old = _run(0, "chacha20", "fixed", {"GSC_WIPE": "0"})
    new = _run(0, "chacha20", "fixed", {"GSC_WIPE": "1"})
    assert " wipe=inputs " in old["describe"] and " wipe=full " in new["describe"]
    # the old wipe: its own hook reads clean while the scan finds the derived buffers
    assert old["legacy"] == "0" and old["scans"][-1][1] > 1_000_000, old["scans"][-1][:3]
    assert {k.split(".", 1)[1] for k in old["scans"][-1][2]} >= {"A", "B", "digits"}
    _assert_clean(new)
    assert old["proofs"] == new["proofs"] and len(new["proofs"]) == 2 * 196 * 64
    assert old["verified"] == ["True"] and new["verified"] == ["True"]


@pytest.mark.parametrize("algo,name,stage", [(0, "chacha20", 2), (0, "chacha20", 4), (0, "chacha20", 5), (1, "aes128", 3)])
def test_a_call_that_leaves_by_an_exception_leaves_nothing_behind(algo, name, stage):
    run = _run(algo, name, "fail", {"GSC_FAIL_AFTER_STAGE": str(stage)})
    assert run["raw"] == ["70 -1", "3 -1"], run["raw"]                 # gsc_prove_raw's failure
    assert run["jsonfail"][0].startswith("True"), run["jsonfail"]     # Prove's: a JSON error string, no proof
    assert [s[0] for s in run["scans"]] == ["init", "failed raw 70", "failed raw 3", "failed json"]
    _assert_clean(run)
    # the knob is read once per process: a fresh one, knob cleared, proves and verifies the same statements
    after = _run(algo, name, "after")
    assert after["verified"] == ["70 True", "3 True"], after["verified"]
    _assert_clean(after)
