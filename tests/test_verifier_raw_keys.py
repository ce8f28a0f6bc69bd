"""CPU tests of libverify.so with raw key points: InitVerifier takes whatever gnark's VerifyingKey.ReadFrom takes — every point compressed
(WriteTo) or raw (WriteRawTo: X | Y, flag bits 00), element by element — and refuses a raw point off the curve and a raw G2 point outside the
r-torsion subgroup, as it refuses the compressed ones (tests/test_verifier.py).  Keys are rewritten by tests/keyraw.py."""
import pytest

import keyraw
from conftest import KAT, golden_bytes


@pytest.fixture(scope="module")
def raw_vk():
    vk = golden_bytes("vk.chacha20")
    raw = keyraw.raw_vk(vk)
    nk = len(dict((name, elems) for name, _, _, elems in keyraw.vk_sections(vk))["g1.K"])
    assert len(raw) == len(vk) + 32 + 3 * 64 + 32 * ((nk + 1) // 2)      # alpha, beta2, gamma2, delta2 and every second K point doubled
    return raw


def _sig():
    return KAT["ciphertext"] + KAT["nonce"] + KAT["counter"].to_bytes(4, "little") + KAT["input"]


def _kat_verdicts(gsc):
    out = []
    for hexproof in KAT["proofs"].values():
        proof = bytes.fromhex(hexproof)
        bad = bytearray(_sig()); bad[70] ^= 1
        out.append((gsc.verify({"cipher": "chacha20", "proof": proof, "publicSignals": _sig()}), gsc.verify({"cipher": "chacha20", "proof": proof, "publicSignals": bytes(bad)})))
    return out


def test_raw_verifying_key_loads_and_accepts_the_kat_proofs(gsc, raw_vk):
    assert gsc.init_verifier(0, golden_bytes("vk.chacha20"))
    want = _kat_verdicts(gsc)
    assert gsc.init_verifier(0, raw_vk)
    assert _kat_verdicts(gsc) == want == [(True, False)] * len(KAT["proofs"])
    # every point raw, and the all-compressed key again
    assert gsc.init_verifier(0, keyraw.rewrite_vk(golden_bytes("vk.chacha20"), lambda name, i: True))
    assert _kat_verdicts(gsc) == want
    assert gsc.init_verifier(0, golden_bytes("vk.chacha20"))


def _element(vk, name, i=0):
    secs = {n: elems for n, _, _, elems in keyraw.vk_sections(vk)}
    o, sz = secs[name][i]
    return o, sz


@pytest.mark.parametrize("name,index", [("g1.alpha", 0), ("g1.K", 4), ("g2.delta", 0)])
def test_raw_y_off_by_one_does_not_load(gsc, raw_vk, name, index):
    o, sz = _element(raw_vk, name, index)
    assert sz in (64, 128) and raw_vk[o] & 0xC0 == 0                      # a raw element
    bad = bytearray(raw_vk)
    y = int.from_bytes(bad[o + sz - 32:o + sz], "big")
    bad[o + sz - 32:o + sz] = ((y + 1) % keyraw.P).to_bytes(32, "big")
    assert gsc.init_verifier(0, raw_vk)
    assert not gsc.init_verifier(0, bytes(bad))
    assert gsc.init_verifier(0, golden_bytes("vk.chacha20"))


def test_raw_coordinate_not_below_p_does_not_load(gsc, raw_vk):
    o, sz = _element(raw_vk, "g1.K", 2)
    bad = bytearray(raw_vk)
    y = int.from_bytes(bad[o + 32:o + 64], "big")
    assert sz == 64 and y < keyraw.P                                      # (so y + p fits in 32 bytes)
    bad[o + 32:o + 64] = (y + keyraw.P).to_bytes(32, "big")               # the same residue, not canonical
    assert not gsc.init_verifier(0, bytes(bad))
    assert gsc.init_verifier(0, golden_bytes("vk.chacha20"))


def test_raw_gamma_outside_the_subgroup_does_not_load(gsc, raw_vk):
    bad_point = keyraw.twist_point_outside_g2()
    assert keyraw.decode_g2(keyraw.enc_g2(bad_point, True))[0] == 1 and keyraw.decode_g2(keyraw.enc_g2(keyraw.G2_GEN, True))[0] == 0
    for raw in (True, False):
        bad = keyraw.rewrite_vk(raw_vk, replace={("g2.gamma", 0): keyraw.enc_g2(bad_point, raw)})
        assert not gsc.init_verifier(0, bad), raw
    assert gsc.init_verifier(0, golden_bytes("vk.chacha20"))


def test_truncated_and_padded_raw_keys_do_not_load(gsc, raw_vk):
    o, sz = _element(raw_vk, "g1.K", 6)
    for bad in (raw_vk[:o + 40], raw_vk[:20], raw_vk + b"\x00", raw_vk[:-1]):
        assert not gsc.init_verifier(0, bad)
    assert gsc.init_verifier(0, golden_bytes("vk.chacha20"))
