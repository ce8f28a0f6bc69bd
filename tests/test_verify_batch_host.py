"""CPU test of the batched Groth16 check's per-thread code (csrc/verify_batch_dev.hpp, the device code of k_verify_batch.hip) built for
the host by tests/native/verify_batch_check.cpp (no GPU needed): random rho_i accept valid proofs and reject two proofs whose public
signals are swapped, which the naive sum (every rho_i = 1) accepts."""
import os
import struct
import subprocess

import pytest

from conftest import ROOT, golden_bytes

CSRC = os.path.join(ROOT, "gnark-symmetric-crypto_amd", "csrc")


@pytest.fixture(scope="module")
def batch_check():
    from test_verify_gpu_host import _build
    exe = _build("verify_batch_check", [os.path.join(ROOT, "tests", "native", "verify_batch_check.cpp"), os.path.join(CSRC, "verify_common.cpp"),
                                        os.path.join(CSRC, "json.cpp")], hip_headers=True)

    def run(algo, vk, items, ones=False):
        inp = bytes([algo, 1 if ones else 0]) + struct.pack("<I", len(vk)) + vk + struct.pack("<I", len(items))
        for proof, sig in items:
            inp += struct.pack("<I", len(proof)) + proof[:196].ljust(196, b"\0") + sig
        out = subprocess.run([exe], input=inp, capture_output=True, timeout=600, check=True).stdout.decode().split()
        assert out[0] == "ok" and out[2] == "batch", out
        return int(out[1]), int(out[3])
    return run


@pytest.fixture(scope="module")
def three_proofs(chacha_oracle, oracle):
    cs, pk, vk = chacha_oracle
    items = []
    for t in range(3):
        key, nonce, counter, pt = bytes([t + 1] * 32), bytes([t + 7] * 12), 5 + t, bytes(range(t, t + 64))
        proof, ct = oracle.prove(cs, pk, "chacha20", key, nonce, counter, pt, 0x1000 + t, 0x2000 + 3 * t)
        sig = ct + nonce + counter.to_bytes(4, "little") + pt
        assert oracle.verify(vk, "chacha20", proof, sig)
        items.append((proof, sig))
    return items


def test_random_randomizers_accept_valid_proofs(batch_check, three_proofs):
    assert batch_check(0, golden_bytes("vk.chacha20"), three_proofs) == (3, 1)


def test_swapped_public_signals_rejected_with_randomizers_accepted_by_naive_sum(batch_check, three_proofs, oracle, chacha_oracle):
    (p0, s0), (p1, s1), third = three_proofs
    swapped = [(p0, s1), (p1, s0), third]
    vk = chacha_oracle[2]
    assert not oracle.verify(vk, "chacha20", p0, s1) and not oracle.verify(vk, "chacha20", p1, s0)
    assert batch_check(0, golden_bytes("vk.chacha20"), swapped) == (3, 0)
    # control: with every rho_i = 1 the swap leaves sum L_i unchanged, so the naive check passes
    assert batch_check(0, golden_bytes("vk.chacha20"), swapped, ones=True) == (3, 1)
    assert batch_check(0, golden_bytes("vk.chacha20"), three_proofs, ones=True) == (3, 1)


def test_c_plus_p_and_c_minus_p_rejected_with_randomizers(batch_check, three_proofs):
    from test_gpu_verify import P, _add, _smul
    from test_gpu_verify_batched import _g1_decode, _with_point
    (p0, s0), (p1, s1), third = three_proofs
    pt = _smul((1, 2), 0xdeadbeefcafe, False)
    items = [(_with_point(p0, 96, _add(_g1_decode(p0[96:128]), pt, False)), s0),
             (_with_point(p1, 96, _add(_g1_decode(p1[96:128]), (pt[0], P - pt[1]), False)), s1), third]
    assert _with_point(p0, 96, _g1_decode(p0[96:128])) == p0
    assert batch_check(0, golden_bytes("vk.chacha20"), items) == (3, 0)
    assert batch_check(0, golden_bytes("vk.chacha20"), items, ones=True) == (3, 1)
