"""CPU proof of the model behind tests/test_gpu_verify_g1.py (no GPU needed).  tests/native/verify_g1_check.cpp compiles the verifier's device
headers (verify_dev.hpp, verify_batch_dev.hpp, verify_claims_dev.hpp) for the host and walks the case table of tests/verifymodel.py the way the
kernels do, one item at a time, printing the fields gsc_debug_verify_g1 returns; here they must equal the model's bytes for EVERY case, in a plain
build and in one under AddressSanitizer and UBSan (a program of its own; nothing is loaded into Python under a sanitizer).  So a failure on the GPU
lies in the device mapping, not in the model.  The model's own pieces are checked too: the incremental window tables against their logarithms, the
public-input windows (through the native walk's L), every claim of the case table (verifymodel.reached), and the hook's boundary."""
import ctypes as C
import os
import random
import re
import struct
import subprocess

import pytest

import devref as D
import keyraw as KR
import verifymodel as M
from conftest import ROOT

CSRC = D.CSRC
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-static-libasan", "-static-libubsan"]
LARGE = ("chacha_plain", "large")      # 4097 Miller loops on one CPU thread: the one case walked without pairings, its flag is the GPU tests'


def _build(tag, extra):
    exe = os.path.join(ROOT, "build", "verify_g1_check_" + tag)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", CSRC] + extra + \
          ["-o", exe, os.path.join(ROOT, "tests", "native", "verify_g1_check.cpp"), os.path.join(CSRC, "verify_common.cpp"), os.path.join(CSRC, "json.cpp")]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return exe


@pytest.fixture(scope="module")
def plain():
    return _build("plain", [])


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    d = tmp_path_factory.mktemp("probe")
    (d / "probe.cpp").write_text("int main() { return 0; }\n")      # only a compiler without the runtime skips; the real build is asserted
    if subprocess.run(["g++"] + SAN + ["-o", str(d / "probe"), str(d / "probe.cpp")], capture_output=True).returncode != 0:
        pytest.skip("the compiler has no sanitizer runtime")
    return _build("san", SAN)


def _walk(exe, c, pairings=True, tables=False, fill=M.FILL, vk=None, algo=None):
    proofs, lens, sigs, rnd = c.inputs()
    vk = c.key.vk_bytes() if vk is None else vk
    inp = bytes([c.key.algo if algo is None else algo, (0 if pairings else 1) | (2 if tables else 0), fill]) + struct.pack("<I", len(vk)) + vk + struct.pack("<I", c.n)
    for i in range(c.n):
        inp += struct.pack("<I", lens[i]) + proofs[196 * i:196 * (i + 1)] + sigs[144 * i:144 * (i + 1)] + struct.pack("<8I", *rnd[8 * i:8 * i + 8])
    inp += struct.pack("<I", len(c.ends)) + b"".join(struct.pack("<I", e) for e in c.ends)
    out = subprocess.run([exe], input=inp, capture_output=True, timeout=900)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    lines = out.stdout.decode().splitlines()
    res = {"rc": int(lines[0].split()[1])}
    for l in lines[1:]:
        name, _, hx = l.partition(" ")
        res[name] = bytes.fromhex(hx)
    if "prho" in res:
        res["prho"] = [struct.unpack("<5I", res["prho"][20 * p:20 * p + 20]) for p in range(len(c.ends))]
    return res


def _flagless(want):
    return dict(want, flag=b"\2", pflag=bytes([2]) * len(want["pflag"]))


# ---- the model's own pieces ----
def test_window_tables_against_their_logarithms():
    """the incremental tables are the points of entry_log: every entry of the windows with collisions, a sample elsewhere"""
    rnd = random.Random(5)
    for name, key in M.keys().items():
        pts = key.table_points()
        special = range(9) if key.algo == 0 else (2, 12, 13, 14, 15)
        for w in list(special) + rnd.sample(range(M.NWIN), 3):
            for v in (range(256) if w in special else rnd.sample(range(256), 8)):
                assert pts[256 * w + v] == M.g1(key.entry_log(w, v)), (name, w, v)
        if key.has_commitment:
            cp = key.ctable_points()
            for j, v in [(0, 1), (0, 255), (31, 255), (17, 128)] + [(rnd.randrange(32), rnd.randrange(256)) for _ in range(8)]:
                assert cp[256 * j + v] == M.g1(key.centry_log(j, v)), (name, j, v)
    coll = M.keys()["chacha_coll"]
    pts = coll.table_points()
    assert pts[256 * 7 + 255] is None and pts[256 * 6 + 3] is None and pts[256 * 8 + 6] is None and pts[256 * 5 + 3] == M.g1(2 * coll.klog(41))
    assert all(p is None for p in M.keys()["aes_coll"].table_points()[512:768])
    assert coll.k[66] is None and coll.k[67] is None and 66 not in coll.raw and 67 in coll.raw, "infinity in both encodings"


def test_generator_multiples_and_encodings():
    for k in (1, 2, M.R - 1, 0x1234567 << 200):
        p = M.g1(k)
        assert p == KR.g1_mul((1, 2), k) and KR.decode_g1(KR.enc_g1(p, False)) == (0, p) and KR.decode_g1(KR.enc_g1(p, True)) == (0, p)
        q = M.g2(k)
        assert q == KR.g2_mul(KR.G2_GEN, k) and KR.decode_g2(KR.enc_g2(q, False)) == (0, q)
    assert M.g1(0) is None and M.g1(M.R) is None and M.g2(None) is None
    for name, key in M.keys().items():
        vk = key.vk_bytes()
        secs = dict((n, el) for n, _, _, el in KR.vk_sections(vk))      # keyraw's walk of the layout agrees with the writer
        assert len(secs["g1.K"]) == len(key.k) and ("ped.g" in secs) == key.has_commitment, name
        sizes = [sz for _, sz in secs["g1.K"]]
        assert [i for i, sz in enumerate(sizes) if sz == 64] == sorted(key.raw), name


def test_columns_are_what_they_say():
    for name in M.keys():
        cols = M.columns(name)
        assert all(p.verdict() == 1 for p in cols.valid), name
        assert all(p.verdict() == 0 for p in cols.bad) and len({p.name for p in cols.all()}) == len(cols.all())
        ys = {KR.enc_g1(M.g1(p.A), False)[0] & 0xC0 for p in cols.valid[:4] if p.A is not None}
        assert ys == {0x80, 0xC0}, "both signs of y"
        for p in cols.bad:      # the reference decoders refuse exactly the slot that was spoiled
            slot, length = p.slot()
            com = p.key.has_commitment
            parts = {"A": slot[:32], "C": slot[96:128], "PoK": slot[164:196] if com else slot[132:164]}
            if com:
                parts["D"] = slot[132:164]
            refused = [n for n, b in parts.items() if b[0] & 0xC0 == 0 or KR.decode_g1(b)[0] == 1] + (["B"] if KR.decode_g2(slot[32:96])[0] == 1 else [])
            shape = length == (196 if com else 164) and slot[128:132] == struct.pack(">I", 1 if com else 0)
            assert (len(refused) == 1 and refused[0] in p.slots and shape) or (not refused and not shape), (name, p.name)
        big = [p for p in cols.valid if p.a_point][0]
        assert all(KR.sqrt_fp(KR.g1_rhs(v)) is None for v in range(big.a_point[0] + 1, M.P)) and KR.decode_g1(big.slot()[0][:32]) == (0, big.a_point)


def test_every_case_reaches_what_it_claims():
    got = set()
    for key_name, shape in M.CASES:
        got |= M.reached(M.case(key_name, shape))
    assert got >= set(M.WHY), sorted(set(M.WHY) - got)
    with pytest.raises(AssertionError):      # a claim that does not hold is noticed
        c = M.case("chacha_plain", 64)
        M.reached(M.Case("x", c.key, c.proofs, c.rho, c.t, claims=[("block_tree", 1, 0, 32, "dbl")]))


# ---- the native walk against the model ----
@pytest.mark.parametrize("key_name", ("chacha_plain", "chacha_coll", "aes_coll"))
def test_native_tables_and_key_points(plain, key_name):
    """k_verify_tables' every entry (the other walks build only the entries their proofs read)"""
    c = M.case(key_name, 1)
    res = _walk(plain, c, tables=True)
    table, ctable = c.expected_tables()
    assert res["rc"] == 0 and res["key_status"] == c.key.key_status()
    assert not M.table_mismatches(res["table"], table)[:6] and not M.table_mismatches(res["ctable"], ctable)[:6]
    assert not M.mismatches(c, res, c.expected())[:6]


def _walk_case(exe, key_name, shape):
    """every field the hook returns, the chunk's and the parts' flags included"""
    c = M.case(key_name, shape)
    pairings = (key_name, shape) != LARGE
    want = c.expected() if pairings else _flagless(c.expected())
    res = _walk(exe, c, pairings=pairings)
    assert res["rc"] == 0 and not M.mismatches(c, res, want)[:6]


@pytest.mark.parametrize("key_name,shape", M.CASES, ids=lambda v: str(v))
def test_native_walk_equals_the_model(plain, key_name, shape):
    _walk_case(plain, key_name, shape)


@pytest.mark.parametrize("key_name,shape", M.CASES, ids=lambda v: str(v))
def test_native_walk_under_sanitizers(sanitized, key_name, shape):
    _walk_case(sanitized, key_name, shape)


def test_native_refusals(plain):
    c = M.case("chacha_plain", 1)
    vk = c.key.vk_bytes()
    assert _walk(plain, c, vk=vk[:-1])["rc"] == -2 and _walk(plain, c, algo=1)["rc"] == -3
    assert _walk(plain, c, vk=vk[:64] + bytes([0x80]) + KR.be(M._off_curve_x())[1:] + vk[96:])["rc"] == -2


# ---- the hook's boundary ----
def test_hook_is_declared_exported_wrapped_and_documented(gsc):
    header = open(os.path.join(ROOT, "include", "libprove.h")).read()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", gsc.LIB_PATH]).decode()
    assert " T gsc_debug_verify_g1\n" in syms and "extern int gsc_debug_verify_g1(" in header and "struct gsc_debug_verify_g1_args {" in header
    assert "gsc_debug_verify_g1" in gsc.EXPORTS and callable(gsc.debug_verify_g1)
    # the ctypes image against the compiler's: every field's name, offset and size, and the struct's size
    names = [n for n, _ in gsc.DebugVerifyG1Args._fields_]
    src = "#include <cstdio>\n#include <cstddef>\n#include \"libprove.h\"\nint main() { typedef gsc_debug_verify_g1_args A; A a;\n" + \
          "".join('printf("%s %%zu %%zu\\n", offsetof(A, %s), sizeof a.%s);\n' % (n, n, n) for n in names) + 'printf("size %zu 0\\n", sizeof(A)); return 0; }\n'
    exe = os.path.join(ROOT, "build", "verify_g1_args_layout")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-x", "c++", "-", "-o", exe], input=src, text=True, check=True)
    got = [l.split() for l in subprocess.check_output([exe], text=True).splitlines()]
    want = [[n, str(getattr(gsc.DebugVerifyG1Args, n).offset), str(getattr(gsc.DebugVerifyG1Args, n).size)] for n in names] + [["size", str(C.sizeof(gsc.DebugVerifyG1Args)), "0"]]
    assert got == want
    body = header[header.index("struct gsc_debug_verify_g1_args {"):]
    assert len(re.findall(r"[\w\]]\s*[,;]", body[body.index("{"):body.index("};") + 2])) == len(names)      # and the C struct has no field beyond them
    for txt in ("README.md", "DESIGN.md", "VERDICT.md"):
        assert "gsc_debug_verify_g1" in open(os.path.join(ROOT, txt)).read(), txt


def test_hook_refuses_without_the_opt_in_and_before_a_device(gsc):
    import sys
    code = ("import os, sys, ctypes as C\n%s"
            "sys.path.insert(0, %r); import gsc_loader; g = gsc_loader.load()\n"
            "print('rc=%%d' %% g.lib().gsc_debug_verify_g1(C.byref(g.DebugVerifyG1Args())))\n"
            "print('rc2=%%d' %% g.debug_verify_g1(0, b'x' * 40, bytes(196), [164], bytes(144), [1] * 8, path=7)['rc'])\n")
    env = {k: v for k, v in os.environ.items() if k != "GSC_ENABLE_TEST_HOOKS"}
    out = subprocess.run([sys.executable, "-c", code % ("os.environ.pop('GSC_ENABLE_TEST_HOOKS', None)\n", ROOT)], env=env, capture_output=True, text=True, timeout=120)
    assert "rc=-1" in out.stdout and "rc2=-1" in out.stdout and out.stdout.count("test hooks are disabled") == 2, out.stdout + out.stderr
    env = dict(os.environ, GSC_ENABLE_TEST_HOOKS="1", HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", code % ("", ROOT)], env=env, capture_output=True, text=True, timeout=120)
    assert "rc=-1" in out.stdout and "rc2=-1" in out.stdout and "path is 1 or 2" in out.stdout, out.stdout + out.stderr
