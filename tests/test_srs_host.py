"""CPU tests of the powers file's host side (csrc/srs.hpp: the header, the section offsets, the slots).
tests/native/srs_check.cpp is built with g++, once plainly and once under AddressSanitizer + UBSan (a stand-alone program run as its own
process: this is a parser of caller bytes), and driven with a valid L = 2 file that a Python model (tests/srsmodel.py) writes from known
(tau, alpha, beta): every truncation, a wrong magic, L edited against the length, trailing bytes, L = 0 and L = 25, elements with flag bits and
all-zero elements.  What it prints is compared with the model's own offsets.  Then the C-ABI: the new symbols are exported and declared, and
the test hook refuses without the test-hook environment before a device is asked for."""
import os
import subprocess
import sys

import pytest

import srsmodel
from conftest import ROOT, golden_bytes

CSRC = os.path.join(ROOT, "gnark-symmetric-crypto_amd", "csrc")
BUILD = os.path.join(ROOT, "build")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-static-libasan", "-static-libubsan"]
NEW_SYMBOLS = ("gsc_srs_verify", "gsc_setup_from_srs", "gsc_debug_srs_generate", "gsc_debug_group_idft", "gsc_debug_column_sums")
L, TAU, ALPHA, BETA = 2, 0x1234567, 0xabcdef01, 0x31415926


@pytest.fixture(scope="module", params=["plain", "asan_ubsan"])
def check_exe(request):
    exe = os.path.join(BUILD, "srs_check_" + request.param)
    os.makedirs(BUILD, exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC] + (SAN if request.param != "plain" else []) +
                          ["-o", exe, os.path.join(ROOT, "tests", "native", "srs_check.cpp"), os.path.join(CSRC, "formats.cpp")])
    return exe


@pytest.fixture(scope="module")
def valid_file():
    return srsmodel.write(L, TAU, ALPHA, BETA)


def _run(exe, data, name, *more):
    path = os.path.join(BUILD, name)
    open(path, "wb").write(data)
    env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    return subprocess.run([exe, path] + list(more), capture_output=True, text=True, timeout=600, env=env)


def test_term_lists_of_the_chacha_circuit(check_exe, valid_file):
    """the three matrices by wire against a second walk in the check program: every column's term count and sums; the cut into segments
    covers every term once; the coefficient table's signs and magnitudes.
    The matrices hold 33 601 + 57 168 + 55 417 = 146 186 terms: the terms of the R1C instructions, which is what groth16_setup walks (the keys made
    from these lists equal gsc_setup's byte for byte, tests/test_gpu_setup_from_srs.py).  The 167 059 of DESIGN.md §3.2 is the solver's count of
    the terms it evaluates (the hints' inputs, 31 625 terms here, are part of its work and no rows of the matrices): a figure about the solver's
    program, not about L, R and O, so the totals here are pinned against the second walk instead."""
    r1cs = os.path.join(BUILD, "srs_check.r1cs.chacha20")
    open(r1cs, "wb").write(golden_bytes("r1cs.chacha20"))
    out = _run(check_exe, valid_file, "srs_check.valid", r1cs)
    assert out.returncode == 0 and "SRS-OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    rep = dict(l.split("=", 1) for l in out.stdout.split() if "=" in l)
    assert [int(rep[m + ".terms"]) for m in "LRO"] == [33601, 57168, 55417] and int(rep["terms.total"]) == 146186
    assert [int(rep[m + ".longest"]) for m in "LRO"] == [849, 22768, 12025] == [int(rep[m + ".wire0"]) for m in "LRO"]      # the ONE wire
    assert int(rep["hint.terms"]) == 31625 and int(rep["coefficients"]) == 40
    assert {int(rep[m + ".columns"]) for m in "LRO"} == {23281}
    for m in "LRO":
        assert 1 <= int(rep[m + ".longest"]) <= int(rep[m + ".terms"]) and int(rep[m + ".segments"]) >= -(-int(rep[m + ".longest"]) // 256)
    # 0: no bits; 1: one bit; r - 1: one bit, negative; 2; r - 2; a 34-bit value
    assert rep["meta"] == "0,1,10001,2,10002,22"


def test_walk_offsets_slots_and_refusals(check_exe, valid_file):
    out = _run(check_exe, valid_file, "srs_check.valid")
    assert out.returncode == 0 and "SRS-OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    rep = dict(l.split("=", 1) for l in out.stdout.split() if "=" in l)
    lay, N = srsmodel.layout(L), 1 << L
    assert len(valid_file) == lay["bytes"] == 1612
    assert (int(rep["L"]), int(rep["N"]), int(rep["bytes"])) == (L, N, lay["bytes"])
    for key, sec in (("tau1", "tauG1"), ("tau2", "tauG2"), ("alpha1", "alphaG1"), ("beta1", "betaG1"), ("beta2", "betaG2")):
        assert int(rep[key]) == lay[sec]
    assert int(rep["g1"]) == 4 * N - 1 and int(rep["g2"]) == N + 1
    # the slots are the sections of each group laid end to end, as the model wrote them
    pts = srsmodel.points(L, TAU, ALPHA, BETA)
    import keyraw
    want1 = b"".join(keyraw.enc_g1(p, True) for sec in ("tauG1", "alphaG1", "betaG1") for p in pts[sec])
    want2 = b"".join(keyraw.enc_g2(p, True) for sec in ("tauG2", "betaG2") for p in pts[sec])
    assert rep["g1slots"] == want1.hex() and rep["g2slots"] == want2.hex()
    assert (rep["name.first"], rep["name.alpha0"], rep["name.betalast"], rep["name.g2last"]) == ("tauG1[0]", "alphaG1[0]", "betaG1[%d]" % (N - 1), "betaG2")
    assert int(rep["truncations"]) == len(valid_file)                       # lengths 0 .. len - 1, each refused
    assert "trailing_bytes" in rep["trailing"] and "magic" in rep["magic"] and "length_does_not_match_L" in rep["L.edited"] and "L_outside_[1,_24]" in rep["L.range"]
    assert rep["g1.zero"] == "srs:_betaG1[%d]_is_the_point_at_infinity" % (N - 1) and rep["g2.zero"] == "srs:_betaG2_is_the_point_at_infinity"
    N24 = 1 << 24
    assert int(rep["bytes24"]) == 12 + 64 * (4 * N24 - 1) + 128 * (N24 + 1)


@pytest.mark.parametrize("case", ["empty", "header_only", "magic", "L0", "L25", "L3", "trailing", "compressed"])
def test_refused_files_exit_cleanly(check_exe, valid_file, case):
    b = bytearray(valid_file)
    if case == "empty":
        b = bytearray()
    elif case == "header_only":
        b = b[:12]
    elif case == "magic":
        b[7] = ord("2")
    elif case in ("L0", "L25", "L3"):
        b[8:12] = int(case[1:]).to_bytes(4, "big")
    elif case == "trailing":
        b += b"\x00"
    else:
        b[srsmodel.offset(L, "alphaG1", 1)] |= 0x80
    out = _run(check_exe, bytes(b), "srs_check." + case)
    assert out.returncode == 3 and out.stdout.startswith("REFUSED srs: "), out.stdout + out.stderr


def test_new_symbols_are_exported_and_declared():
    lib = os.path.join(ROOT, "gnark-symmetric-crypto_amd", "libprove.so")
    if not os.path.exists(lib):
        import __graft_entry__
        __graft_entry__.build()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    header = open(os.path.join(ROOT, "include", "libprove.h")).read()
    for s in NEW_SYMBOLS:
        assert " T %s\n" % s in syms, s
        assert "extern int %s(" % s in header, s
    assert "NOT snarkjs' .ptau" in header and "gscsrs01" in header
    import gsc_loader
    g = gsc_loader.load()
    assert set(NEW_SYMBOLS) <= set(g.EXPORTS)
    for w in ("srs_verify", "setup_from_srs", "debug_srs_generate", "debug_group_idft", "debug_column_sums"):
        assert callable(getattr(g, w)), w


_NO_HOOKS = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
import gsc_loader
g = gsc_loader.load()
L = g.lib()
p, n = C.c_void_p(0x1234), C.c_size_t(7)
rc = L.gsc_debug_srs_generate(2, bytes(32), C.byref(p), C.byref(n))
print("RC", rc, p.value, n.value)
print("IDFT", L.gsc_debug_group_idft(0, 1, bytes(128), C.create_string_buffer(128), C.create_string_buffer(2)))
print("COLS", L.gsc_debug_column_sums(0, 0, None, 0, (C.c_uint32 * 1)(0), None, None, 0, None, None, None))
pk, vk, a, b = C.c_void_p(0x1234), C.c_void_p(0x1234), C.c_size_t(7), C.c_size_t(7)
s1, k1 = g._slice(b"x"); s2, k2 = g._slice(b"y")
print("SETUP", L.gsc_setup_from_srs(s1, s2, bytes(32), C.byref(pk), C.byref(a), C.byref(vk), C.byref(b)), pk.value, vk.value, a.value, b.value)
s, keep = g._slice(open(sys.argv[2], "rb").read())
print("HEADER", L.gsc_srs_verify(s))
"""


def test_the_generator_hook_needs_the_test_hooks_and_a_bad_header_needs_no_device(tmp_path, valid_file):
    """-1 and the outputs NULL / 0 before a device is asked for (HIP_VISIBLE_DEVICES hides any); a file refused by the host walker is
    refused (0, rule 1 on stdout) without a device too"""
    lib = os.path.join(ROOT, "gnark-symmetric-crypto_amd", "libprove.so")
    if not os.path.exists(lib):
        import __graft_entry__
        __graft_entry__.build()
    bad = str(tmp_path / "srs.truncated")
    open(bad, "wb").write(valid_file[:-1])
    env = {k: v for k, v in os.environ.items() if k != "GSC_ENABLE_TEST_HOOKS"}
    env.update(HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", _NO_HOOKS, ROOT, bad], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert "RC -1 None 0" in lines and "HEADER 0" in lines and "IDFT -1" in lines and "COLS -1" in lines and "SETUP -1 None None 0 0" in lines, out.stdout
    for hook in ("gsc_debug_srs_generate", "gsc_debug_group_idft", "gsc_debug_column_sums", "gsc_setup_from_srs with a caller-supplied seed"):
        assert hook + " refused: test hooks are disabled" in out.stdout, hook
    assert "gsc_srs_verify: rule 1: srs: truncated (the length does not match L)" in out.stdout
