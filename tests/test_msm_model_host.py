"""The references tests/test_gpu_msm.py holds the MSM kernels against, proven on a CPU first: the Jacobian fixed-window multiplication against the
affine ec_mul, the Python digit model against the device's own signed_digit_step built for the host (tests/native/msm_digits_check.cpp), the case
table's internal consistency (digits that stand for their scalars, gok / group_ok as the cases intend, every route of the issue present), and the
hook's boundary: exported, declared, refused without GSC_ENABLE_TEST_HOOKS (test_host_boundary.py) and refusing malformed calls before a device is
asked for."""
import os
import random
import re
import struct
import subprocess
import sys

import pytest

import devref as D
from conftest import ROOT

R = D.R


@pytest.mark.parametrize("group", [0, 1], ids=["g1", "g2"])
def test_jacobian_reference_against_affine_arithmetic(group):
    rnd = random.Random(77 + group)
    ks = [0, 1, 2, 3, 255, 256, 257, R - 1, R - 2, D.HALF_R, D.HALF_R + 1, 1 << 253] + [rnd.randrange(R) for _ in range(4)] + [rnd.getrandbits(64)]
    for k in ks:
        assert D.gen_mul(group, k) == (D.ec_mul(k, D.GEN[group]) if k else None), hex(k)
    assert D.gen_mul(group, R) is None and D.gen_mul(group, R + 5) == D.ec_mul(5, D.GEN[group])
    w = 1 if group == 0 else 2
    p = D.ec_mul(9, D.GEN[group])
    T = (p[0], p[1], D.f_small(w, 1))
    assert D.jac_to_affine(D.jac_madd(w, T, p)) == D.ec_add(p, p) and D.jac_madd(w, T, D.ec_neg(p)) is None      # the equal and the opposite operand


@pytest.fixture(scope="module")
def digits_exe():
    return D.native_exe("msm_digits_check")


@pytest.mark.parametrize("c", range(4, 18))
def test_digit_model_against_the_device_recoder(digits_exe, c):
    """signed_digits is the model behind win_digit_words and the window octets of flat_digit_words"""
    rnd = random.Random(c)
    nwin = D.msm_windows(c)
    vals = []
    for mont in (0, 1):
        for s in D.windowed_patterns(c, mont, rnd, 96):
            vals.append(D.sign_normalise(s) if mont else (s, False))
    payload = struct.pack("<2i", c, len(vals)) + bytes(n for _, n in vals) + b"".join(m.to_bytes(32, "little") for m, _ in vals)
    out = subprocess.run([digits_exe], input=payload, capture_output=True, timeout=60, check=True).stdout
    got = struct.unpack("<%di" % (len(vals) * nwin), out[:4 * len(vals) * nwin])
    for i, (m, n) in enumerate(vals):
        assert list(got[i * nwin:(i + 1) * nwin]) == D.signed_digits(m, c, nwin, n), (c, hex(m), n)
    assert not any(out[4 * len(vals) * nwin:])


def _i16(words, o, p, batch):
    return struct.unpack_from("<8h", words, 16 * (o * batch + p))


@pytest.mark.parametrize("group", [0, 1], ids=["g1", "g2"])
def test_case_table_is_consistent(group):
    """every digit word stands for its scalar, and the cases reach what the issue names"""
    table = D.msm_case_table(group)
    seen = set()
    for case in table.values():
        pl, B = case.plan, case.batch
        flat, gok = case.flat_model()
        win = case.win_model()
        gr = case.group_ok()
        cols = range(case.ncols)
        # windowed digits: sum_j e_j 2^(c j) = the scalar (mod r for sign-normalised ones), all digits in [-D, D - 1]
        wrows = case.digit_rows or [case.rows[k] for k in pl.wide]
        nwin, noct, words = D.msm_windows(case.c), (len(wrows) + 7) // 8, 2 if case.c > 16 else 1
        assert len(win) == (16 * words * nwin * noct * B if pl.wide else 0)
        for k, row in list(enumerate(wrows))[:12]:
            for p in (0, 1, 7, B - 1):
                ds = [struct.unpack_from("<8i" if words == 2 else "<8h", win, 16 * words * ((j * noct + k // 8) * B + p))[k % 8] for j in range(nwin)]
                assert sum(d << (case.c * j) for j, d in enumerate(ds)) % R == case.scalars[row * B + p] and (case.mont or sum(d << (case.c * j) for j, d in enumerate(ds)) >= 0)
                if any(d == -(1 << (case.c - 1)) for d in ds):
                    seen.add("digit -D at c=%d" % case.c)
        # flat digits, octet by octet, against the value each slot stands for
        for o in range(pl.nflat // 8):
            for p in cols:
                d = _i16(flat, o, p, B)
                vals = [case.value(r, p) for r in pl.frows[8 * o:8 * o + 8]]
                if pl.octwin[o] >= 0:
                    first = o - pl.octwin[o] // 8
                    ds = [x for oo in range(first, first + (D.msm_windows(pl.cv) + 7) // 8) for x in _i16(flat, oo, p, B)]
                    assert sum(x << (pl.cv * j) for j, x in enumerate(ds)) % R == vals[0] and not any(ds[D.msm_windows(pl.cv):])
                    continue
                g = 0 if o >= pl.nbit // 8 else gok[o * D.MSM_FEW_PROOFS + p] if case.nproofs else gok[o * (B // 64) + p // 64]
                if o < pl.nbit // 8 and g:
                    assert gr[o] == 1 and abs(d[0]) <= D.MSM_GROUP_ENTRIES and not any(d[1:])
                    t, v = [], d[0]
                    for _ in range(8):
                        r3 = (v + 1) % 3 - 1; t.append(r3); v = (v - r3) // 3
                    assert [x % R for x in t] == vals
                    seen.add("gok 1"); seen.add("v = %d" % d[0] if abs(d[0]) == 3280 else "gok 1")
                    continue
                if o < pl.nbit // 8:
                    seen.add("gok 0"); seen.add("group_ok 0" if not gr[o] else "gok 0")
                for i, (x, v) in enumerate(zip(d, vals)):
                    if x == D.MSM_FLAT_ESCAPE:
                        assert D.sign_normalise(v)[0] >= 1 << 15
                        seen.add("escape")
                    else:
                        assert x % R == v and abs(x) < 1 << 15
                        seen.add("beyond the row" if abs(x) > pl.len[8 * o + i] else "the row's last entry" if abs(x) == pl.len[8 * o + i] else "in the row")
        if case.name == "bits_one_wave_not_ternary":
            assert gok == bytes([1, 1, 1, 0]) and gr == b"\1\1"      # gok[o * 2 + wave]: group 1 of wave 1 holds the 2
        if case.name.startswith("bits_collision"):
            assert gr == b"\0\1" and gok == b"\0\1"
        exps = case.exponents()
        if "sum_is_infinity" in case.name:
            assert exps[0] == 0 and all(e == 0 for e in exps[1::2]) and all(exps[2::2])
        seen.add("c=%d" % case.c if pl.wide else "flat only")
        seen.add("latency" if case.nproofs else "batch")
        seen.add("digit_bases" if case.digit_rows else "batch")
        seen.add("plane" if case.plane else "batch")
        seen.add("addend" if pl.wide and pl.nflat else "batch")
    for what in ("gok 0", "gok 1", "group_ok 0", "v = 3280", "v = -3280", "escape", "beyond the row", "the row's last entry", "in the row", "digit -D at c=16", "digit -D at c=17",
                 "c=4", "c=6", "c=15", "c=16", "c=17", "latency", "digit_bases", "plane", "addend"):
        assert what in seen, what


def test_symbol_is_exported_declared_and_wrapped():
    lib = os.path.join(ROOT, "gnark-symmetric-crypto_amd", "libprove.so")
    if not os.path.exists(lib):
        import __graft_entry__
        __graft_entry__.build()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    header = open(os.path.join(ROOT, "include", "libprove.h")).read()
    assert " T gsc_debug_msm\n" in syms and "extern int gsc_debug_msm(" in header and "struct gsc_debug_msm_args {" in header
    import gsc_loader
    g = gsc_loader.load()
    assert "gsc_debug_msm" in g.EXPORTS and callable(g.debug_msm)
    # the ctypes structure follows the header's field order
    fields = [f[0] for f in g.DebugMsmArgs._fields_]
    body = header[header.index("struct gsc_debug_msm_args {"):]
    body = body[:body.index("};")]
    assert re.findall(r"(\w+)\s*[,;]", body) == fields
    for txt in ("INTEGRATION.md", "DESIGN.md"):
        assert "gsc_debug_msm" in open(os.path.join(ROOT, txt)).read(), txt


_MALFORMED = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import gsc_loader, devref as D
g = gsc_loader.load()
R = D.R
pt = [D.raw_point(gr, D.GEN[gr]) for gr in (0, 1)]
def call(tag, group=0, n=1, kind=None, rowlen=None, scal=None, points=None, **kw):
    kind = kind if kind is not None else [2] * n
    batch = kw.get("batch", 64)
    scal = scal if scal is not None else [1] * (n * batch) + [0] * batch
    a = dict(c=6, cv=0, mont=1, batch=64, nproofs=0, per_flat=0, per_win=0); a.update(kw)
    try:
        g.debug_msm(group, points if points is not None else pt[1 if group else 0] * n, kind, rowlen or [4] * n, list(range(n)), scal, n + 1, n, a["c"], a["cv"], a["mont"], a["batch"],
                    a["nproofs"], a["per_flat"], a["per_win"], kw.get("digit_rows"))
        print("CALL", tag, "accepted")
    except RuntimeError:
        print("CALL", tag, "refused")
call("group", group=2)
call("c3", c=3); call("c18", c=18); call("cv3", cv=3); call("cv16", cv=16)
call("batch96", batch=96, scal=[0] * (2 * 96)); call("batch0", batch=0, scal=[])
call("nproofs33", nproofs=33)
call("per_win12", per_win=12); call("per_flat12", per_flat=12, kind=[1]); call("per_flat520", per_flat=520, kind=[1])
call("scalar_r", scal=[R] + [1] * 63 + [0] * 64)
call("compressed", points=bytes([0x80]) + pt[0][1:]); call("infinity", points=bytes(64))
call("mont0_bit", mont=0, kind=[0]); call("mont0_narrow", mont=0, kind=[1])
call("kind3", kind=[3]); call("rowlen0", kind=[1], rowlen=[0])
call("digit_bases", digit_rows=[0])
call("no_device")
"""


def test_malformed_calls_are_refused_before_a_device_is_asked_for():
    """with every device hidden a well-formed call fails at the device; each malformed one must name ITS reason on stdout, not the device's"""
    env = dict(os.environ, GSC_ENABLE_TEST_HOOKS="1", HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", _MALFORMED, ROOT], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "accepted" not in out.stdout
    reasons = [l for l in out.stdout.splitlines() if l.startswith("gsc_debug_msm: ") or "no HIP device" in l]
    want = ["no such group", "c outside", "c outside", "cv outside", "cv outside", "batch is 64 or 128", "batch is 64 or 128", "nproofs beyond", "multiple of 8", "multiple of 8",
            "at most 512", "not below r", "not raw and finite", "not raw and finite", "canonical scalars", "canonical scalars", "no such kind", "narrow row of no length", "digit_bases must exceed",
            "no HIP device"]
    assert len(reasons) == len(want), out.stdout
    for line, w in zip(reasons, want):
        assert w in line, (w, line)
