"""The reference and the case table tests/test_gpu_assemble.py holds the proof assembly kernels against, proven on a CPU first: the Python split
against glv.hpp built for the host (tests/native/glv_split_check.cpp), the lane-by-lane model of k_fin_scalarmul_few against the plain product and
against affine arithmetic with phi(x, y) = (beta x, y), the expected bytes against an independent ec_add / ec_mul composition, the challenge
against the oracle's expand_message_xmd; then what the table reaches, as conditions on the splits glv_split REALLY returns for its scalars, and
that each of a list of wrong kernels would change an expected byte or flag.  glv_split's floors leave k1 >= 0 and both magnitudes below 2^128 for
EVERY scalar (and k1 = 0 for k = 0 alone), so a negative k1, a zero k1 beside a non-zero k2, bits 128 and 129 of the top chunk and the fifth word reach k_fin_scalarmul_few only through the hook's glv_in:
the second table (devref.assemble_halves), held to the same conditions.  Last last the hook's boundary: exported, declared, wrapped, refusing
malformed calls before a device is asked for (hooks disabled: test_host_boundary.py)."""
import ctypes as C
import os
import random
import re
import struct
import subprocess
import sys

import pytest

import devref as D
from conftest import ROOT

R, P = D.R, D.P


@pytest.fixture(scope="module")
def table():
    return D.assemble_table()


@pytest.fixture(scope="module")
def real_splits():
    """scalar -> (k1 words, k2 words, neg) from glv.hpp itself, for every scalar of the tables and a few more"""
    exe = D.native_exe("glv_split_check")
    rnd = random.Random(5)
    ks = sorted(set(D.assemble_table().scalars() + D.assemble_table(67).scalars() + [rnd.randrange(R) for _ in range(500)] + [rnd.getrandbits(b) for b in (1, 31, 32, 33, 64, 127, 128, 129, 250)]))
    out = subprocess.run([exe], input=struct.pack("<i", len(ks)) + b"".join(k.to_bytes(32, "little") for k in ks), capture_output=True, timeout=60, check=True).stdout
    assert len(out) == 48 * len(ks)
    res = {}
    for i, k in enumerate(ks):
        w = struct.unpack_from("<12I", out, 48 * i)
        assert w[11] == 1, hex(k)
        res[k] = (w[:5], w[5:10], w[10])
    return res


def test_split_model_is_glv_hpp(real_splits):
    for k, rec in real_splits.items():
        assert D.glv_words(k) == rec, hex(k)
        k1, k2 = D.glv_halves(k)
        assert (k1 + k2 * D.GLV_LAMBDA - k) % R == 0 and 0 <= k1 < 1 << 128 and abs(k2) < 1 << 128
    # why k1 is never negative: c_i = floor(k g_i / 2^384) with g_i = floor(2^384 beta_i / r) never exceeds the real coefficient k beta_i / r of
    # (k, 0) in the basis, and k1 is the sum of the two non-negative remainders times a1, a2 > 0
    assert D.GLV_A1 > 0 and D.GLV_A2 > 0 and D.GLV_G1 * R <= D.GLV_A1 << 384 and D.GLV_G2 * R <= D.GLV_B1_ABS << 384
    assert D.GLV_A1 * D.GLV_A1 + D.GLV_A2 * D.GLV_B1_ABS == R                  # the basis' determinant


def test_lane_model_agrees_with_the_plain_product(table, real_splits):
    """every scalar of the table, under the split glv_split really returns, on several points"""
    rnd = random.Random(6)
    points = [1, 2, R - 1, D.GLV_LAMBDA] + [rnd.randrange(1, R) for _ in range(3)]
    for k in table.scalars():
        assert D.glv_words(k) == real_splits[k]
        for a in points:
            assert D.latency_product(k, a) == k * a % R == D.batch_product(k, a), (hex(k), hex(a))


def _lanes_on_points(rec, pt):
    """k_fin_scalarmul_few in affine arithmetic: one doubling chain, lanes keep 2^(5q) P, the k2 lanes apply phi, each multiplies by its chunk"""
    k1w, k2w, neg = rec
    chain, kept = pt, []
    for i in range(126):
        if i % 5 == 0:
            kept.append(chain)
        chain = D.ec_add(chain, chain)
    assert len(kept) == 26
    acc = None
    for second, words in ((False, k1w), (True, k2w)):
        for q, chunk in enumerate(D.glv_chunks(words)):
            mine = kept[q]
            if second:
                mine = ((mine[0][0] * D.GLV_BETA % P,), mine[1])
            if (neg >> (1 if second else 0)) & 1:
                mine = D.ec_neg(mine)
            acc = D.ec_add(acc, D.ec_mul(chunk, mine) if chunk else None)
    return acc


def test_lane_model_on_points(table):
    by_neg = {}
    for k in table.scalars():
        by_neg.setdefault(D.glv_words(k)[2], k)
    assert sorted(by_neg) == [0, 2]
    pt = D.ec_mul(0x1234567, D.G1_GEN)
    for k in list(by_neg.values()) + [R - 1, 1 << 253, D.glv_compose((1 << 125) - 1, (1 << 125) - 1)]:
        assert _lanes_on_points(D.glv_words(k), pt) == D.ec_mul(k, pt), hex(k)
    top = (1 << 130) - 1
    for rec, k in [D.glv_chosen(top, top, neg) for neg in range(4)] + [D.glv_chosen(31 << 125, 0, 1), D.glv_chosen(0, 31 << 125, 2)]:
        assert _lanes_on_points(rec, pt) == D.ec_mul(k, pt) and D.latency_product(0, 0x1234567, rec=rec) == k * 0x1234567 % R


@pytest.mark.parametrize("has_c", [True, False], ids=["with_c", "without_c"])
def test_expected_bytes_against_affine_composition(table, has_c):
    """ec_mul / ec_add on the points themselves, no discrete logarithm carried along"""
    exp = table.expected(has_c=has_c)
    le = lambda pt: D.pack_point(1, pt)
    for p in (0, 1, 2, 3, 4, 6, 7, 9, 15, 17, 26, 30, 31, 40, 63):
        col = table.cols[p]
        pt = {key: None if col[key] is None else D.ec_mul(col[key], D.G1_GEN) for key in ("a", "b1", "k", "z", "c")}
        t0 = None if pt["a"] is None or col["s"] == 0 else D.ec_mul(col["s"], pt["a"])
        t1 = None if pt["b1"] is None or col["r"] == 0 else D.ec_mul(col["r"], pt["b1"])
        krs = D.ec_add(D.ec_add(pt["k"], pt["z"]), D.ec_add(t0, t1))
        if has_c:
            krs = D.ec_add(krs, pt["c"])
        fl = (1 if pt["a"] is None else 0) | (4 if krs is None else 0)
        assert exp["flags"][p] & 5 == fl, (p, col["name"])
        if pt["a"] is not None:
            assert exp["out"][256 * p:256 * p + 64] == le(pt["a"]), p
        if krs is not None:
            assert exp["out"][256 * p + 192:256 * p + 256] == le(krs), (p, col["name"])
        assert exp["tmp"][64 * p:64 * p + 64] == le(t0) and exp["tmp"][64 * (64 + p):64 * (64 + p) + 64] == le(t1), p
        assert exp["tmp_inf"][p] == (t0 is None) and exp["tmp_inf"][64 + p] == (t1 is None)
    for p in (1, 10, 15):
        col = table.cols[p]
        if col["b2"] is None:
            assert exp["flags"][p] & 2 and exp["out"][256 * p + 64:256 * p + 192] == bytes([0xA5]) * 128
        else:
            assert exp["out"][256 * p + 64:256 * p + 192] == D.pack_point(2, D.ec_mul(col["b2"], D.G2_GEN)) and not exp["flags"][p] & 2


def test_challenge_against_the_oracle(oracle, table):
    exp = table.expected()
    for p in (0, 1, 16, 63):      # 16: the 64 zero bytes of a commitment at infinity
        msg = exp["cpts"][64 * p:64 * p + 64]
        assert (p == 16) == (msg == bytes(64))
        o = C.create_string_buffer(48)
        oracle.lib().orc_expand_message_xmd(msg, 64, b"bsb22-commitment", 16, o, 48)
        assert o.raw == D.expand_message_xmd48(msg, b"bsb22-commitment")
        assert exp["commit"][32 * p:32 * p + 32] == (int.from_bytes(o.raw, "big") % R * D.FR_MONT % R).to_bytes(32, "little")


def test_table_reaches_what_the_kernels_can_get_wrong(table, real_splits):
    cols = table.cols
    assert len(cols) == 64 and len({c["name"] for c in cols}) >= 21
    splits = {key: [real_splits[c[key]] for c in cols] for key in ("r", "s")}
    every = splits["r"] + splits["s"]
    for key in ("r", "s"):      # both signs of k2 in each role; k1 < 0 is no output of glv_split (module docstring): test_chosen_halves_reach_the_rest
        assert {s[2] for s in splits[key]} == {0, 2}, key
    chunks = [(D.glv_chunks(s[0]), D.glv_chunks(s[1])) for s in every]
    for half in (0, 1):
        for q in range(26):
            assert any(c[half][q] for c in chunks), (half, q)
        assert any(31 in c[half] for c in chunks)
    # a zero half: k2 = 0 for every k < 2^64 or so; k1 = 0 only for k = 0 (the remainders of both floors would have to vanish): glv_in again
    assert any(not any(c[1]) and any(c[0]) for c in chunks) and any(not any(c[0]) and not any(c[1]) for c in chunks) and not any(any(c[1]) and not any(c[0]) for c in chunks)
    for half in (0, 1):
        for q in D.STRADDLES:      # ... with bits on both sides of the word boundary; the top chunk's upper side is bits 128, 129, which glv_split
            lo_bits = 32 - (5 * q & 31)      # never sets for a scalar below r (test_split_model_is_glv_hpp): there the chunk itself
            assert any(c[half][q] & ((1 << lo_bits) - 1) and (q == 25 or c[half][q] >> lo_bits) for c in chunks), (half, q)
    assert any(c["r"] >> 253 for c in cols) and any(c["s"] >> 253 for c in cols)
    fixed, _ = D.assemble_scalars()
    for v in fixed:
        assert any(c["r"] == v for c in cols) and any(c["s"] == v for c in cols), hex(v)
    # flags: every value the issue names, and every byte position of a flag word with a clean neighbour in the same word — in every mode
    seen = set()
    for has_c in (True, False):
        for has_commit in (True, False):
            fl = table.expected(has_c=has_c, has_commit=has_commit)["flags"]
            seen |= set(fl)
            for pos in range(4):
                assert any(fl[p] and not all(fl[p & ~3:(p & ~3) + 4][j] for j in range(4) if j != pos) for p in range(pos, 64, 4)), (has_c, has_commit, pos)
            assert sum(1 for f in fl if f) <= 16 and sum(1 for f in fl if not f) >= 48
    assert {1, 2, 4, 8, 16, 7, 31} <= seen
    # the latency kernel's runs (nproofs 1, 3, 32 on the table and on its second half) start with flagged and with clean columns
    assert cols[0]["a"] is None and cols[1]["a"] is not None and cols[32]["a"] is not None
    # the ragged batch: three columns in a word of their own, flagged differently
    fl = D.assemble_table(67).expected()["flags"]
    assert len(fl) == 67 and len(set(fl[64:])) == 3 and all(fl[64:])
    assert D.assemble_table(67).cols[:64] == cols
    # degenerate additions of k_fin_combine, as the integers say
    by = {c["name"]: c for c in cols}
    t = lambda c: (c["s"] * c["a"] % R, c["r"] * c["b1"] % R)
    assert by["K = Z"]["k"] == by["K = Z"]["z"] and (by["K = -Z"]["k"] + by["K = -Z"]["z"]) % R == 0
    assert t(by["sA = rB1"])[0] == t(by["sA = rB1"])[1] != 0 and sum(t(by["sA = -rB1"])) % R == 0 and t(by["sA = -rB1"])[0]
    c = by["K + Z = sA + rB1"]; assert (c["k"] + c["z"] - sum(t(c))) % R == 0 and sum(t(c)) % R
    c = by["K + Z = -(sA + rB1)"]; assert (c["k"] + c["z"] + sum(t(c))) % R == 0 and sum(t(c)) % R
    c = by["K + Z + sA + rB1 = C"]; assert (c["k"] + c["z"] + sum(t(c)) - c["c"]) % R == 0
    c = by["K + Z + sA + rB1 = -C"]; assert (c["k"] + c["z"] + sum(t(c)) + c["c"]) % R == 0
    for key in D.ASSEMBLE_SETS:
        alone = [c for c in cols if c[key] is None and sum(1 for k2 in D.ASSEMBLE_SETS if c[k2] is None) == 1]
        assert alone, key
    assert by["s = 0 with A finite"]["a"] is not None and by["r = 0"]["b1"] is not None and by["r = 0"]["r"] == 0
    # scales: 1, p - 1 and all limbs at their maximum reach every set
    sets = table.sets()
    for name in D.ASSEMBLE_SETS:
        w = 64 if name == "b2" else 32
        lams = {sets[name][2][w * p:w * p + w] for p in range(64)}
        for v in (1, P - 1, D.ALL_LIMBS):
            assert any(int.from_bytes(l[-32:], "big") == v or int.from_bytes(l[:32], "big") == v for l in lams), (name, hex(v))


def test_chosen_halves_reach_the_rest(table):
    """glv_in: all four values of neg, every chunk position at 31, the top chunk's bits 128 and 129 from the fifth word, a zero half under a set sign"""
    halves = D.assemble_halves()
    recs = [rec for col in halves for rec in col]
    assert len(halves) == 32 and {r[2] for r in recs} == {0, 1, 2, 3}
    for role in (0, 1):
        assert {col[role][2] for col in halves} == {0, 1, 2, 3}
    chunks = [(D.glv_chunks(r[0]), D.glv_chunks(r[1])) for r in recs]
    for half in (0, 1):
        for q in range(26):
            assert any(c[half][q] == 31 for c in chunks), (half, q)
            assert any(c[half][q] and sum(1 for v in c[0] + c[1] if v) == 1 for c in chunks), ("alone", half, q)
        assert any(r[half][4] == 3 for r in recs) and any(c[half][25] >> 3 for c in chunks)
        assert any(not any(r[half]) and any(r[1 - half]) and not r[2] for r in recs), "a zero half"
        assert any(not any(r[half]) and (r[2] >> half) & 1 for r in recs), "a zero half with its sign bit set"
    for variant in ("neg_exchanged", "straddle_ignored", "q25_ignored", "beta_on_first_half", "rs_exchanged"):
        for case in (table, table.rotated(32)):
            good, bad = case.expected(nproofs=32, halves=halves), case.expected(nproofs=32, halves=halves, variant=variant)
            assert good["out"] != bad["out"], variant
    # the top chunk alone decides a column: q25_ignored changes the columns whose only chunk is that one
    good, bad = table.rotated(32).expected(nproofs=32, halves=halves), table.rotated(32).expected(nproofs=32, halves=halves, variant="q25_ignored")
    assert [p for p in range(32) if good["tmp"][64 * p:64 * p + 64] != bad["tmp"][64 * p:64 * p + 64] or good["tmp"][64 * (64 + p):64 * (65 + p)] != bad["tmp"][64 * (64 + p):64 * (65 + p)]]


@pytest.mark.parametrize("variant", D.ASSEMBLE_VARIANTS)
def test_each_wrong_kernel_changes_an_expected_byte(table, variant):
    latency_only = variant in ("neg_exchanged", "straddle_ignored", "q25_ignored", "beta_on_first_half")
    runs = [(32, table), (32, table.rotated(32))] if latency_only else [(0, table)]
    if variant not in ("batch_from_bit_252",) and not latency_only:
        runs.append((32, table))
    for nproofs, case in runs:
        good, bad = case.expected(nproofs=nproofs), case.expected(nproofs=nproofs, variant=variant)
        differing = [p for p in range(64) if good["out"][256 * p:256 * p + 256] != bad["out"][256 * p:256 * p + 256] or good["flags"][p] != bad["flags"][p]]
        assert differing, (variant, nproofs)
    if variant == "c_ignored":      # ... and without C there is nothing to ignore
        assert table.expected(has_c=False) == table.expected(has_c=False, variant=variant)
    if latency_only:                # the batch kernel has no such step
        assert table.expected() == table.expected(variant=variant)


def test_latency_and_batch_models_give_the_same_columns(table):
    batch = table.expected()
    for nproofs, rot in ((1, 0), (3, 0), (32, 0), (32, 32)):
        case = table.rotated(rot)
        few, full = case.expected(nproofs=nproofs), case.expected()
        assert few["out"][:256 * nproofs] == full["out"][:256 * nproofs] and few["flags"][:nproofs] == full["flags"][:nproofs]
        for p in range(nproofs, 64):      # Ar and its flag untouched, tmp at infinity
            assert few["out"][256 * p:256 * p + 64] == bytes([0xA5]) * 64 and not few["flags"][p] & 1 and few["tmp_inf"][p] == 1 == few["tmp_inf"][64 + p]
    assert table.rotated(32).expected()["out"] == batch["out"][256 * 32:] + batch["out"][:256 * 32]


def test_symbol_is_exported_declared_and_wrapped():
    lib = os.path.join(ROOT, "gnark-symmetric-crypto_amd", "libprove.so")
    if not os.path.exists(lib):
        import __graft_entry__
        __graft_entry__.build()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    header = open(os.path.join(ROOT, "include", "libprove.h")).read()
    assert " T gsc_debug_assemble\n" in syms and "extern int gsc_debug_assemble(" in header and "struct gsc_debug_assemble_args {" in header
    import gsc_loader
    g = gsc_loader.load()
    assert "gsc_debug_assemble" in g.EXPORTS and callable(g.debug_assemble)
    fields = [f[0] for f in g.DebugAssembleArgs._fields_]      # the ctypes structure follows the header's field order
    body = header[header.index("struct gsc_debug_assemble_args {"):]
    body = body[:body.index("};")]
    assert re.findall(r"(\w+)\s*[,;]", body) == fields
    for txt in ("INTEGRATION.md", "DESIGN.md", "VERDICT.md"):
        assert "gsc_debug_assemble" in open(os.path.join(ROOT, txt)).read(), txt
    # the hook launches the production kernels and defines none of its own but the two conversions
    src = open(os.path.join(ROOT, "gnark-symmetric-crypto_amd", "csrc", "assemble_debug.hip")).read()
    assert re.findall(r"void (k_\w+)\(", src) == ["k_debug_assemble_in", "k_debug_assemble_out"]
    for launcher in ("launch_prep_rs", "launch_fin_scalarmul(", "launch_fin_scalarmul_few(", "launch_fin_combine", "launch_points_to_affine_be", "launch_challenge_from_point", "glv_split("):
        assert launcher in src, launcher


_MALFORMED = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import gsc_loader, devref as D
g = gsc_loader.load()
R, P = D.R, D.P
T = D.AssembleCase(D.assemble_table().cols[32:36])
def call(tag, batch=4, sets=None, rs=None, edit=None, **kw):
    s = dict(T.sets()) if sets is None else sets
    if edit:
        name, part, at, data = edit
        b = bytearray(s[name][part]); b[at:at + len(data)] = data
        s[name] = tuple(bytes(b) if i == part else x for i, x in enumerate(s[name]))
    res = g.debug_assemble(batch, s, T.rs() if rs is None else rs, **kw)
    print("CALL", tag, "accepted" if res["rc"] == 0 else "refused")
def without(*names):
    return {k: v for k, v in T.sets().items() if k not in names}
be = lambda v: int(v).to_bytes(32, "big")
call("batch0", batch=0); call("batch257", batch=257)
call("nproofs33", nproofs=33); call("nproofs5", nproofs=5)
call("wires", n_wires=4097); call("fill", fill=256)
call("r_is_r", rs=R.to_bytes(32, "little") + T.rs()[32:]); call("s_is_r", rs=T.rs()[:32] + R.to_bytes(32, "little") + T.rs()[64:])
call("mask", mask=bytes(32) * 3 + b"\xff" * 32)
call("lam0", edit=("k", 2, 32, bytes(32))); call("lam_p", edit=("z", 2, 0, be(P))); call("lam2_0", edit=("b2", 2, 64, bytes(64))); call("lam2_p", edit=("b2", 2, 32, be(P)))
call("no_a", sets=without("a")); call("no_b2", sets=without("b2")); call("d_alone", sets=without("pok")); call("pok_alone", sets=without("d"))
s = T.sets(); s["c"] = (s["c"][0], None, s["c"][2]); call("c_half", sets=s)
call("compressed", edit=("a", 0, 0, b"\x80")); call("zero_point", edit=("b1", 0, 64, bytes(64)))
call("glv_in_batch", glv_in=bytes(88 * 4))
call("glv_in_big", nproofs=2, glv_in=bytes(88) + bytes(16) + (4).to_bytes(4, "little") + bytes(68)); call("glv_in_neg", nproofs=1, glv_in=bytes(40) + (4).to_bytes(4, "little") + bytes(44))
call("no_device")
"""


def test_malformed_calls_are_refused_before_a_device_is_asked_for():
    """with every device hidden a well-formed call fails at the device; each malformed one must name ITS reason on stdout, not the device's"""
    env = dict(os.environ, GSC_ENABLE_TEST_HOOKS="1", HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", _MALFORMED, ROOT], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "accepted" not in out.stdout and out.stdout.count("refused") == 24
    reasons = [l for l in out.stdout.splitlines() if l.startswith("gsc_debug_assemble: ") or "no HIP device" in l]
    want = ["batch is 1 .. 256", "batch is 1 .. 256", "nproofs beyond", "nproofs beyond", "more than 4096 wires", "fill is one byte", "scalar that is not below r", "scalar that is not below r",
            "mask that is not below r", "scale that is zero: K", "scale that is not below p: Z", "scale that is zero: B2", "scale that is not below p: B2",
            "missing: A", "missing: B2", "D and Pok come together", "D and Pok come together", "missing: C", "not raw and finite: A", "not raw and finite: B1", "glv_in without nproofs", "magnitude of 2^130", "magnitude of 2^130", "no HIP device"]
    assert len(reasons) == len(want), out.stdout
    for line, w in zip(reasons, want):
        assert w in line, (w, line)
