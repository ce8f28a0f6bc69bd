"""CPU tests of the GPU verifier's host side and of its per-thread arithmetic (no GPU needed):
- the new symbols are declared in include/libprove.h, exported by libprove.so and wrapped in Python;
- the shared host rules (csrc/verify_common) produce the public-input windows of a Python restatement of verifiers.go's input order,
  and every item their pre-check rejects is rejected by libverify.so too;
- csrc/verify_dev.hpp (the device code of k_verify.hip) compiled for the host gives libverify.so's verdicts."""
import os
import random
import struct
import subprocess

import pytest

from conftest import KAT, ROOT, golden_bytes

CSRC = os.path.join(ROOT, "gnark-symmetric-crypto_amd", "csrc")
NEW = ["gsc_verify_init", "gsc_verify_raw", "VerifyBatch", "gsc_debug_pairing"]


def _build(name, sources, hip_headers=False):
    exe = os.path.join(ROOT, "build", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-I", CSRC, "-o", exe] + sources
    if hip_headers:
        cmd[1:1] = ["-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include"]
    subprocess.check_call(cmd)
    return exe


@pytest.fixture(scope="module")
def common_check():
    exe = _build("verify_common_check", [os.path.join(ROOT, "tests", "native", "verify_common_check.cpp"), os.path.join(CSRC, "verify_common.cpp"),
                                         os.path.join(CSRC, "json.cpp")])
    p = subprocess.Popen([exe], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
    yield lambda line: (p.stdin.write(line + "\n"), p.stdin.flush(), p.stdout.readline().strip())[2]
    p.stdin.close(); p.wait(timeout=30)


def test_new_symbols_declared_exported_and_wrapped(gsc):
    header = open(os.path.join(ROOT, "include", "libprove.h")).read()
    for sym in NEW:
        assert "extern" in header and (" " + sym + "(") in header, sym
        assert sym in gsc.EXPORTS, sym
    assert "VerifyBatch" in open(os.path.join(CSRC, "exports.map")).read()
    if not os.path.exists(gsc.LIB_PATH):
        gsc.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", gsc.LIB_PATH]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(NEW) <= exported
    for fn in ("verify_init", "verify_raw", "verify_batch", "debug_pairing"):
        assert callable(getattr(gsc, fn))


def _windows_py(algo, sig):
    """verifiers.go's public inputs, restated, folded into the 144 byte windows of the device tables."""
    ct, nonce, ctr, pt = sig[:64], sig[64:76], sig[76:80], sig[80:144]
    if algo == 0:
        words = [int.from_bytes(ctr, "little")] + [int.from_bytes(nonce[4 * i:4 * i + 4], "little") for i in range(3)]
        words += [int.from_bytes(pt[4 * i:4 * i + 4], "big") for i in range(16)] + [int.from_bytes(ct[4 * i:4 * i + 4], "big") for i in range(16)]
        bits = [(w >> b) & 1 for w in words for b in range(32)]
        assert len(bits) == 1152
        return bytes(sum(bits[8 * j + t] << t for t in range(8)) for j in range(144))
    vals = list(nonce) + [int.from_bytes(ctr, "big")] + list(pt) + list(ct)
    assert len(vals) == 141
    return bytes(vals[:12]) + vals[12].to_bytes(4, "little") + bytes(vals[13:])


def test_window_indices_match_verifiers_go_order(common_check):
    rnd = random.Random(7)
    for algo in (0, 1, 2):
        for _ in range(20):
            sig = rnd.randbytes(144)
            assert bytes.fromhex(common_check("W %d %s" % (algo, sig.hex()))) == _windows_py(algo, sig)
        # the window bases: ChaCha20 8 consecutive bits per window; AES one input each, the counter in four shifted windows
        for j in (0, 11, 12, 15, 16, 143):
            first, shift = map(int, common_check("B %d %d" % (algo, j)).split())
            if algo == 0:
                assert (first, shift) == (1 + 8 * j, 0)
            else:
                assert (first, shift) == ((1 + j, 0) if j < 12 else (13, 8 * (j - 12)) if j < 16 else (1 + j - 3, 0))


def _sig():
    return KAT["ciphertext"] + KAT["nonce"] + KAT["counter"].to_bytes(4, "little") + KAT["input"]


def test_host_precheck_rejections_are_libverify_rejections(gsc, common_check):
    assert gsc.init_verifier(0, golden_bytes("vk.chacha20"))
    good = bytes.fromhex(KAT["proofs"][(0, 0)])
    corpus = []
    for n in (0, 1, 32, 131, 132, 163, 165, 196):
        corpus.append(good[:n] if n <= len(good) else good + bytes(n - len(good)))
    for cnt in (1, 2, 0x01000000, 0xFFFFFFFF):
        corpus.append(good[:128] + cnt.to_bytes(4, "big") + good[132:])
        corpus.append(good[:128] + cnt.to_bytes(4, "big") + good[132:] + bytes(32))
    rejected = 0
    for proof in corpus:
        ok = common_check("S 0 %d %s" % (len(proof), (proof or b"\0").hex()))
        if ok == "0":
            rejected += 1
            assert not gsc.verify({"cipher": "chacha20", "proof": proof, "publicSignals": _sig()}), proof.hex()
    assert rejected == len(corpus)
    assert common_check("S 0 164 %s" % good.hex()) == "1"
    assert common_check("S 1 196 %s" % (good[:128] + (1).to_bytes(4, "big") + good[132:] + bytes(32)).hex()) == "1"


def _dev_check(algo, vk, items):
    exe = _build("verify_dev_check", [os.path.join(ROOT, "tests", "native", "verify_dev_check.cpp"), os.path.join(CSRC, "verify_common.cpp"),
                                      os.path.join(CSRC, "json.cpp")], hip_headers=True)
    inp = bytes([algo]) + struct.pack("<I", len(vk)) + vk + struct.pack("<I", len(items))
    for proof, sig in items:
        inp += struct.pack("<I", len(proof)) + proof[:196].ljust(196, b"\0") + sig
    out = subprocess.run([exe], input=inp, capture_output=True, timeout=600, check=True).stdout.decode().split()
    return [int(x) for x in out]


def test_device_code_on_the_host_agrees_with_libverify(gsc):
    from test_verifier import _twist_point_outside_g2
    vk = golden_bytes("vk.chacha20")
    assert gsc.init_verifier(0, vk)
    sig = _sig()
    items = []
    for h in KAT["proofs"].values():
        proof = bytes.fromhex(h)
        items.append((proof, sig))
        for pos in (0, 3, 70, 77, 100, 143):
            b = bytearray(sig); b[pos] ^= 1; items.append((proof, bytes(b)))
        for pos, bit in ((0, 0x40), (0, 0x80), (1, 1), (40, 1), (32, 0x80), (100, 1), (140, 1), (131, 1)):
            b = bytearray(proof); b[pos] ^= bit; items.append((bytes(b), sig))
        b = bytearray(proof); b[32:96] = _twist_point_outside_g2(); items.append((bytes(b), sig))
        b = bytearray(proof); b[0:32] = bytes([0x40]) + bytes(31); items.append((bytes(b), sig))       # A = infinity
    got = _dev_check(0, vk, items)
    want = [int(gsc.verify({"cipher": "chacha20", "proof": p, "publicSignals": s})) for p, s in items]
    assert got == want
    assert got[0] == 1 and sum(got) == 2


def test_device_code_refuses_a_key_with_gamma_outside_g2():
    from test_verifier import _twist_point_outside_g2
    vk = bytearray(golden_bytes("vk.chacha20")); vk[128:192] = _twist_point_outside_g2()
    _dev_check(0, golden_bytes("vk.chacha20"), [])          # builds the harness
    exe = os.path.join(ROOT, "build", "verify_dev_check")
    out = subprocess.run([exe], input=bytes([0]) + struct.pack("<I", len(vk)) + bytes(vk) + struct.pack("<I", 0), capture_output=True, timeout=600).stdout.decode()
    assert out.strip() == "key 0"
