"""CPU tests of the sigma ceremony's host side (csrc/sigma.hpp on csrc/phase2.hpp: the walk's commitment-key marks, rule 2's comparison, the
splice, the record).  tests/native/sigma_check.cpp is built with g++, once plainly and once under AddressSanitizer + UBSan (a
stand-alone program run as its own process: these are parsers of caller bytes), and driven with a synthetic pair (tests/sigmamodel.py), the
AES-128 test pair and the golden ChaCha20 pair.  What it prints is compared with Python's own walk (tests/keyraw.py) and hashlib.  Then the
C-ABI: the four symbols are exported, declared and in the loader, and a seeded contribution without the test hooks is refused before anything
else happens."""
import hashlib
import os
import subprocess
import sys

import pytest

import keyraw
import sigmamodel
from conftest import ROOT, golden_bytes

CSRC = os.path.join(ROOT, "gnark-symmetric-crypto_amd", "csrc")
BUILD = os.path.join(ROOT, "build")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-static-libasan", "-static-libubsan"]
NEW_SYMBOLS = ("gsc_pedersen_verify", "gsc_setup_contribute_sigma", "gsc_setup_verify_sigma_contribution", "gsc_setup_verify_from_srs")
N = 65


@pytest.fixture(scope="module", params=["plain", "asan_ubsan"])
def check_exe(request):
    exe = os.path.join(BUILD, "sigma_check_" + request.param)
    os.makedirs(BUILD, exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC] + (SAN if request.param != "plain" else []) +
                          ["-o", exe, os.path.join(ROOT, "tests", "native", "sigma_check.cpp"), os.path.join(CSRC, "host_ciphers.cpp")])
    return exe


@pytest.fixture(scope="module")
def small():
    return sigmamodel.build(N)


def _secs(sections, key):
    return {name: el for name, _, _, el in sections(key)}


def _mixed(small):
    """the synthetic pair with every third BasisExpSigma element, one Basis element, one A element, G and GSigmaNeg raw"""
    pk = keyraw.rewrite_pk(small.pk, lambda name, i: (name == "ped.sigma" and i % 3 == 0) or (name, i) in (("ped.basis", 1), ("g1.A", 0)))
    vk = keyraw.rewrite_vk(small.vk, lambda name, i: name in ("ped.g", "ped.gsn"))
    return pk, vk


def test_walk_marks_splice_and_record(check_exe, small, aes_keys):
    _, apk, avk = aes_keys["aes128"]
    mpk, mvk = _mixed(small)
    paths = []
    for tag, b in (("small.pk", small.pk), ("small.vk", small.vk), ("aes.pk", apk), ("aes.vk", avk), ("none.pk", golden_bytes("pk.chacha20")),
                   ("none.vk", golden_bytes("vk.chacha20")), ("mixed.pk", mpk), ("mixed.vk", mvk)):
        paths.append(os.path.join(BUILD, "sigma_check." + tag))
        open(paths[-1], "wb").write(b)
    env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([check_exe] + paths, capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0 and "SIGMA-OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    rep = dict(l.split("=", 1) for l in out.stdout.split() if "=" in l)
    # the marks against Python's walk: the synthetic pair, the AES-128 pair; the ChaCha20 pair has no commitment key
    for tag, pk, vk in (("small", small.pk, small.vk), ("big", apk, avk)):
        ps, vs = _secs(keyraw.pk_sections, pk), _secs(keyraw.vk_sections, vk)
        assert rep[tag + ".pk.ped"] == "1" and rep[tag + ".vk.ped"] == "1"
        assert int(rep[tag + ".pk.n"]) == len(ps["ped.basis"]) == len(ps["ped.sigma"]) > 0
        assert int(rep[tag + ".pk.basis0"]) == ps["ped.basis"][0][0] and int(rep[tag + ".pk.basis_last"]) == ps["ped.basis"][-1][0]
        assert int(rep[tag + ".pk.sigma0"]) == ps["ped.sigma"][0][0] and int(rep[tag + ".pk.sigma_last"]) == ps["ped.sigma"][-1][0]
        assert int(rep[tag + ".vk.g"]) == vs["ped.g"][0][0] and int(rep[tag + ".vk.gsn"]) == vs["ped.gsn"][0][0]
    assert rep["none.pk.ped"] == "0" and rep["none.vk.ped"] == "0" and "none.pk.n" not in rep
    # keyraw and the native walk read the synthetic files identically
    ps, vs = _secs(keyraw.pk_sections, small.pk), _secs(keyraw.vk_sections, small.vk)
    assert int(rep["small.pk.g1"]) == sum(len(el) for nm, el in ps.items() if nm[:2] != "g2") and int(rep["small.pk.g2"]) == 2 + len(ps["g2.B"])
    assert int(rep["small.vk.g1"]) == 3 + len(vs["g1.K"]) and int(rep["small.vk.g2"]) == 5
    assert int(rep["small.pk.n"]) == N and int(rep["small.j0"]) == small.j0 == 1 and int(rep["small.infinities"]) == small.b.count(0) == 3
    # every truncation and every edited count of the commitment-key tail was refused (the program checks; here: that it tried them all)
    assert int(rep["pk.truncations"]) == 4 + 2 * (4 + 32 * N) and int(rep["vk.truncations"]) == 12 + 128
    assert int(rep["pk.count_edits"]) >= 18 and int(rep["vk.count_edits"]) >= 18
    # a spliced key is compressed wherever it was rewritten: 32 bytes back per raw BasisExpSigma element, 64 for the raw GSigmaNeg; the raw
    # Basis, A and G elements stay raw
    assert len(mpk) - len(small.pk) == 32 * (len(range(0, N, 3)) + 2) and len(mvk) - len(small.vk) == 128
    assert int(rep["mixed.pk.bytes"]) - int(rep["mixed.pk.spliced"]) == 32 * len(range(0, N, 3))
    assert int(rep["mixed.vk.bytes"]) - int(rep["mixed.vk.spliced"]) == 64
    assert int(rep["same_outside.compared"]) > 300
    # the record's challenge and the seeded scalars against hashlib
    h_prev, base = bytes(range(32)), bytes(255 - i for i in range(64))
    new, T = bytes(range(64, 128)), bytes(range(128, 192))
    assert rep["challenge"] == sigmamodel.challenge(h_prev, base, new, T).to_bytes(32, "big").hex()
    assert rep["challenge"] == (b"\x00" + hashlib.sha256(b"gsc-sigma-v1" + h_prev + base + new + T).digest()[:31]).hex()
    assert rep["challenge.phase2"] == (b"\x00" + hashlib.sha256(b"gsc-phase2-v1" + h_prev + base + new + T).digest()[:31]).hex()
    seed = bytes(5 * i + 2 for i in range(32))
    x, k = sigmamodel.seeded(seed)
    assert rep["seeded.x"] == x.to_bytes(32, "big").hex() and rep["seeded.k"] == k.to_bytes(32, "big").hex()
    assert x == int.from_bytes(hashlib.sha256(b"gsc-sigma-x" + seed).digest(), "big") % keyraw.R
    assert rep["-G"] == keyraw.enc_g1((1, keyraw.P - 2), True).hex()


def test_the_model_is_a_pedersen_key_on_discrete_logarithms(small):
    assert small.relation_on_logarithms() and small.j0 == 1
    ps, vs = _secs(keyraw.pk_sections, small.pk), _secs(keyraw.vk_sections, small.vk)
    for j in (0, 1, 2, 3, N // 2, N - 2, N - 1):
        o, sz = ps["ped.basis"][j]
        st, p = keyraw.decode_g1(small.pk[o:o + sz])
        assert (st, p) == ((2, None) if small.b[j] == 0 else (0, keyraw.g1_mul((1, 2), small.b[j])))
        o, sz = ps["ped.sigma"][j]
        assert keyraw.decode_g1(small.pk[o:o + sz])[1] == (None if small.b[j] == 0 else keyraw.g1_mul(p, small.sigma))
    assert small.b[2] == small.b[3] != 0
    o, sz = vs["ped.gsn"][0]
    st, q = keyraw.decode_g2(small.vk[o:o + sz])
    o, sz = vs["ped.g"][0]
    st2, g = keyraw.decode_g2(small.vk[o:o + sz])
    assert st == 0 and st2 == 0 and keyraw.g2_add(q, keyraw.g2_mul(g, small.sigma)) is None
    # the model's contribution: every byte outside BasisExpSigma / GSigmaNeg stays, the Schnorr equation holds on the record's integers
    x, k = sigmamodel.seeded(bytes(range(32)))
    pk2, vk2, rec = sigmamodel.contribution(small, x, k)
    assert len(pk2) == len(small.pk) and len(vk2) == len(small.vk) and len(rec) == 224
    p2 = _secs(keyraw.pk_sections, pk2)
    assert pk2[:p2["ped.sigma"][0][0]] == small.pk[:ps["ped.sigma"][0][0]] and vk2[:-64] == small.vk[:-64] and vk2 != small.vk
    z, c = int.from_bytes(rec[192:], "big"), sigmamodel.challenge(rec[:32], keyraw.enc_g1(sigmamodel.g1(small.sigma * small.b[1]), True), rec[64:128], rec[128:192])
    base = sigmamodel.g1(small.sigma * small.b[1])
    assert keyraw.g1_mul(base, z) == keyraw.g1_add(keyraw.decode_g1(rec[128:192])[1], keyraw.g1_mul(keyraw.decode_g1(rec[64:128])[1], c))


def test_refused_files_exit_cleanly(check_exe):
    bad = os.path.join(BUILD, "sigma_check.bad")
    open(bad, "wb").write(golden_bytes("vk.chacha20"))      # a vk where the pk belongs
    out = subprocess.run([check_exe] + [bad] * 6, capture_output=True, text=True, timeout=60)
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
    assert "#define GSC_SIGMA_CONTRIBUTION_BYTES 224" in header
    assert "a distributed sigma is not part of this library" not in header
    import gsc_loader
    g = gsc_loader.load()
    assert set(NEW_SYMBOLS) <= set(g.EXPORTS) and g.SIGMA_CONTRIBUTION_BYTES == 224
    for f in ("pedersen_verify", "setup_contribute_sigma", "setup_verify_sigma_contribution", "setup_verify_from_srs"):
        assert callable(getattr(g, f))
    for s in NEW_SYMBOLS:
        getattr(g.lib(), s)


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
rc = L.gsc_setup_contribute_sigma(s1, s2, bytes(32), C.byref(p), C.byref(np_), C.byref(v), C.byref(nv), rec)
print("RC", rc, p.value, v.value, np_.value, nv.value, rec.raw == bytes(224))
"""


def test_a_seeded_sigma_contribution_needs_the_test_hooks(tmp_path, small):
    """-1, the outputs NULL / 0 and the record zeroed, before the keys are looked at or a device is asked for (HIP_VISIBLE_DEVICES hides any)"""
    lib = os.path.join(ROOT, "gnark-symmetric-crypto_amd", "libprove.so")
    if not os.path.exists(lib):
        import __graft_entry__
        __graft_entry__.build()
    paths = []
    for name, b in (("pk", small.pk), ("vk", small.vk)):
        paths.append(str(tmp_path / name)); open(paths[-1], "wb").write(b)
    env = {k: v for k, v in os.environ.items() if k != "GSC_ENABLE_TEST_HOOKS"}
    env.update(HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", _NO_HOOKS, ROOT] + paths, capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    line = [l for l in out.stdout.splitlines() if l.startswith("RC ")][0]
    assert line == "RC -1 None None 0 0 True", out.stdout
    assert "gsc_setup_contribute_sigma with a caller-supplied seed refused: test hooks are disabled" in out.stdout
