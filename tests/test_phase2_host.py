"""CPU tests of the key ceremony's host side (csrc/phase2.hpp: the key walk, the splice, the record).
tests/native/phase2_check.cpp is built with g++, once plainly and once under AddressSanitizer + UBSan (a stand-alone program run as its own
process: these are parsers of caller bytes), and driven with the golden pk.chacha20 / vk.chacha20: truncations, edited length fields, trailing
bytes, a key with raw elements.  What it prints is compared with Python's own walk (tests/keyraw.py) and hashlib.  Then the C-ABI: the new
symbols are exported, and a seeded contribution without the test hooks is refused before anything else happens."""
import hashlib
import os
import subprocess
import sys

import pytest

import keyraw
from conftest import ROOT, golden_bytes

CSRC = os.path.join(ROOT, "gnark-symmetric-crypto_amd", "csrc")
BUILD = os.path.join(ROOT, "build")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-static-libasan", "-static-libubsan"]
NEW_SYMBOLS = ("gsc_setup_contribute", "gsc_setup_verify_contribution", "gsc_debug_scale_points")


@pytest.fixture(scope="module", params=["plain", "asan_ubsan"])
def check_exe(request):
    exe = os.path.join(BUILD, "phase2_check_" + request.param)
    os.makedirs(BUILD, exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC] + (SAN if request.param != "plain" else []) +
                          ["-o", exe, os.path.join(ROOT, "tests", "native", "phase2_check.cpp"), os.path.join(CSRC, "host_ciphers.cpp")])
    return exe


def test_walk_splice_and_record(check_exe):
    pk, vk = golden_bytes("pk.chacha20"), golden_bytes("vk.chacha20")
    mixed = keyraw.rewrite_pk(pk, lambda name, i: i < 40 and i % 3 == 0)
    paths = []
    for tag, b in (("pk", pk), ("vk", vk), ("mixed", mixed)):
        paths.append(os.path.join(BUILD, "phase2_check." + tag))
        open(paths[-1], "wb").write(b)
    env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([check_exe] + paths, capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0 and "PHASE2-OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    rep = dict(l.split("=", 1) for l in out.stdout.split() if "=" in l)
    ps = {name: el for name, _, _, el in keyraw.pk_sections(pk)}
    vs = {name: el for name, _, _, el in keyraw.vk_sections(vk)}
    assert int(rep["pk.Z"]) == len(ps["g1.Z"]) and int(rep["pk.K"]) == len(ps["g1.K"])
    assert int(rep["pk.g1"]) == 3 + sum(len(ps[n]) for n in ("g1.A", "g1.B", "g1.Z", "g1.K")) and int(rep["pk.g2"]) == 2 + len(ps["g2.B"])
    assert int(rep["vk.g1"]) == 3 + len(vs["g1.K"]) and int(rep["vk.g2"]) == 3
    assert int(rep["pk.delta1"]) == ps["g1.delta"][0][0] and int(rep["pk.delta2"]) == ps["g2.delta"][0][0]
    assert int(rep["vk.delta1"]) == vs["g1.delta"][0][0] and int(rep["vk.delta2"]) == vs["g2.delta"][0][0]
    assert int(rep["pk.Z0"]) == ps["g1.Z"][0][0] and int(rep["pk.K0"]) == ps["g1.K"][0][0]
    assert int(rep["pk.truncations"]) > 1500 and int(rep["vk.truncations"]) == len(vk)
    assert int(rep["pk.count_edits"]) >= 30 and int(rep["vk.count_edits"]) >= 13
    # a spliced key is compressed wherever it was rewritten: 64 bytes back for the raw delta (its G2 twin is i = 0 too: 64 more), 32 per raw Z / K
    raw_rewritten = 1 + 2 * 14      # delta; Z and K elements 0, 3, ..., 39
    assert int(rep["mixed.bytes"]) - int(rep["mixed.spliced"]) == 32 * raw_rewritten + 64
    # the record's challenge, the seeded scalars and the affine addition against Python
    h_prev, dprev = bytes(range(32)), bytes(255 - i for i in range(64))
    delta, T = bytes(range(64, 128)), bytes(range(128, 192))
    c = hashlib.sha256(b"gsc-phase2-v1" + h_prev + dprev + delta + T).digest()[:31]
    assert rep["challenge"] == (b"\x00" + c).hex()
    seed = bytes(3 * i + 1 for i in range(32))
    for label in ("x", "k"):
        want = int.from_bytes(hashlib.sha256(b"gsc-phase2-" + label.encode() + seed).digest(), "big") % keyraw.R
        assert rep["seeded." + label] == want.to_bytes(32, "big").hex()
    g = (1, 2)
    g2 = keyraw.g1_add(g, g)
    assert rep["G+G"] == keyraw.enc_g1(g2, True).hex() and rep["G+2G"] == keyraw.enc_g1(keyraw.g1_add(g, g2), True).hex()


def test_refused_files_exit_cleanly(check_exe):
    bad = os.path.join(BUILD, "phase2_check.bad")
    open(bad, "wb").write(golden_bytes("vk.chacha20"))      # a vk where the pk belongs
    out = subprocess.run([check_exe, bad, bad], capture_output=True, text=True, timeout=60)
    assert out.returncode == 3 and out.stdout.startswith("REFUSED pk: "), out.stdout + out.stderr


def test_new_symbols_are_exported_and_declared():
    lib = os.path.join(ROOT, "gnark-symmetric-crypto_amd", "libprove.so")
    if not os.path.exists(lib):
        import __graft_entry__
        __graft_entry__.build()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    header = open(os.path.join(ROOT, "include", "libprove.h")).read()
    exports = open(os.path.join(CSRC, "exports.map")).read()
    assert "gsc_*" in exports.split("local:")[0]                       # the map's global pattern covers them
    for s in NEW_SYMBOLS:
        assert " T %s\n" % s in syms, s
        assert "extern int %s(" % s in header, s
    assert "#define GSC_CONTRIBUTION_BYTES 224" in header
    import gsc_loader
    g = gsc_loader.load()
    assert set(NEW_SYMBOLS) <= set(g.EXPORTS) and g.CONTRIBUTION_BYTES == 224


_NO_HOOKS = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
import gsc_loader
g = gsc_loader.load()
L = g.lib()
pk, vk = open(sys.argv[2], "rb").read(), open(sys.argv[3], "rb").read()
s1, k1 = g._slice(pk); s2, k2 = g._slice(vk)
p, v, np_, nv = C.c_void_p(0x1234), C.c_void_p(0x1234), C.c_size_t(7), C.c_size_t(7)
rec = C.create_string_buffer(b"\xAA" * 224, 224)
rc = L.gsc_setup_contribute(s1, s2, bytes(32), C.byref(p), C.byref(np_), C.byref(v), C.byref(nv), rec)
print("RC", rc, p.value, v.value, np_.value, nv.value, rec.raw == bytes(224))
"""


def test_a_seeded_contribution_needs_the_test_hooks(tmp_path):
    """-1, the outputs NULL / 0 and the record zeroed, before the keys are looked at or a device is asked for (HIP_VISIBLE_DEVICES hides any)"""
    lib = os.path.join(ROOT, "gnark-symmetric-crypto_amd", "libprove.so")
    if not os.path.exists(lib):
        import __graft_entry__
        __graft_entry__.build()
    paths = []
    for name in ("pk.chacha20", "vk.chacha20"):
        paths.append(str(tmp_path / name)); open(paths[-1], "wb").write(golden_bytes(name))
    env = {k: v for k, v in os.environ.items() if k != "GSC_ENABLE_TEST_HOOKS"}
    env.update(HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", _NO_HOOKS, ROOT] + paths, capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    line = [l for l in out.stdout.splitlines() if l.startswith("RC ")][0]
    assert line == "RC -1 None None 0 0 True", out.stdout
    assert "gsc_setup_contribute with a caller-supplied seed refused: test hooks are disabled" in out.stdout
