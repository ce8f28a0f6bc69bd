"""Groth16 Setup from a powers file (gsc_setup_from_srs) on whole keys: in seeded (TEST) mode the keys made from the group
elements alone equal the oracle's Setup (AES-128, Pedersen sections included) and gsc_setup (ChaCha20-V3) byte for byte; in production mode
(delta = gamma = 1) the key is a deterministic function of (r1cs, file), a larger file serves a smaller circuit, and the key becomes usable
after one contribution: the production path end to end runs in child processes (tests/srs_child.py)."""
import json
import os
import subprocess
import sys

import pytest

import keyraw
import srsmodel
from conftest import ROOT, golden_bytes

pytestmark = pytest.mark.gpu

SEED = bytes([7] * 32)
G1_RAW = keyraw.enc_g1(srsmodel.G1, False)
G2_RAW = keyraw.enc_g2(srsmodel.G2, False)


@pytest.fixture(scope="module")
def chacha_files(gsc):
    return {L: gsc.debug_srs_generate(L, SEED) for L in (14, 15, 16)}


@pytest.fixture(scope="module")
def chacha_seeded(gsc):
    return gsc.setup(golden_bytes("r1cs.chacha20"), SEED)


@pytest.fixture(scope="module")
def chacha_production(gsc, chacha_files):
    return gsc.setup_from_srs(golden_bytes("r1cs.chacha20"), chacha_files[15])


def test_aes128_seeded_keys_equal_the_oracles(gsc, aes_keys):
    r1cs, opk, ovk = aes_keys["aes128"]               # oracle.setup(r1cs, bytes([1] * 32)) — see conftest.aes_keys
    seed = bytes([1] * 32)
    pk, vk = gsc.setup_from_srs(r1cs, gsc.debug_srs_generate(17, seed), seed)
    assert vk == ovk
    assert len(pk) == len(opk)
    assert pk == opk


def test_chacha_seeded_keys_equal_gsc_setup(gsc, chacha_files, chacha_seeded):
    pk, vk = gsc.setup_from_srs(golden_bytes("r1cs.chacha20"), chacha_files[15], SEED)
    assert vk == chacha_seeded[1]
    assert len(pk) == len(chacha_seeded[0])
    assert pk == chacha_seeded[0]


def test_chacha_production_key_is_deterministic_and_a_larger_file_serves(gsc, chacha_files, chacha_production):
    assert gsc.setup_from_srs(golden_bytes("r1cs.chacha20"), chacha_files[16]) == chacha_production


def test_chacha_production_key_sections(chacha_production, chacha_seeded):
    pk, vk = chacha_production
    prod = {name: [pk[o:o + s] for o, s in el] for name, _, _, el in keyraw.pk_sections(pk)}
    seeded = {name: [chacha_seeded[0][o:o + s] for o, s in el] for name, _, _, el in keyraw.pk_sections(chacha_seeded[0])}
    for name in ("g1.A", "g1.B", "g2.B", "g1.alpha", "g1.beta", "g2.beta"):
        assert prod[name] == seeded[name] and len(prod[name]) > 0, name
    assert prod["g1.delta"] == [G1_RAW] and prod["g2.delta"] == [G2_RAW]
    assert prod["g1.Z"] != seeded["g1.Z"] and prod["g1.K"] != seeded["g1.K"]
    v = {name: [vk[o:o + s] for o, s in el] for name, _, _, el in keyraw.vk_sections(vk)}
    assert v["g1.delta"] == [G1_RAW] and v["g2.delta"] == [G2_RAW] and v["g2.gamma"] == [G2_RAW]


def test_a_tampered_or_too_small_file_is_refused(gsc, capfd, chacha_files):
    r1cs = golden_bytes("r1cs.chacha20")
    other = keyraw.enc_g1(keyraw.g1_mul(srsmodel.G1, 5), True)
    bad = srsmodel.replace(chacha_files[15], 15, "alphaG1", 1000, other)
    capfd.readouterr()
    assert gsc.srs_verify(bad) is False
    assert "rule 5" in capfd.readouterr().out
    with pytest.raises(RuntimeError, match="-2"):
        gsc.setup_from_srs(r1cs, bad)
    assert "rule 5" in capfd.readouterr().out
    with pytest.raises(RuntimeError, match="-2"):
        gsc.setup_from_srs(r1cs, chacha_files[14])
    assert "too small" in capfd.readouterr().out
    with pytest.raises(RuntimeError, match="-2"):
        gsc.setup_from_srs(r1cs[:1000], chacha_files[15])


SMALL_ENGINE = {"GSC_MAX_BATCH": "128", "GSC_Z_TABLE_GB": "4", "GSC_W_TABLE_GB": "4", "GSC_ENABLE_TEST_HOOKS": "1"}
_state = {"dead": None}


def _child(tmp, algo, srs, n):
    """tests/srs_child.py in a process of its own.  After a child that aborted or ran into its time limit no further child is started."""
    if _state["dead"]:
        pytest.fail("not started: the child of '%s' aborted or ran into its time limit" % _state["dead"])
    open(os.path.join(str(tmp), "srs"), "wb").write(srs)
    env = {k: v for k, v in os.environ.items() if not k.startswith("GSC_")}
    env.update(SMALL_ENGINE)
    out = os.path.join(str(tmp), "facts.json")
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "srs_child.py"), ROOT, str(algo), str(n), out, str(tmp)], env=env, capture_output=True, text=True,
                           timeout=600)
    except subprocess.TimeoutExpired:
        _state["dead"] = str(tmp)
        raise
    if p.returncode < 0 or p.returncode in (124, 134, 137, 139):
        _state["dead"] = str(tmp)
    assert p.returncode == 0 and "CHILD-OK" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
    return json.load(open(out))


@pytest.mark.parametrize("algo,L,proof_len", [(0, 15, 164), (1, 17, 196)])
def test_the_production_path_end_to_end(gsc, tmp_path, algo, L, proof_len):
    """file -> delta = 1 key -> one contribution (checked) -> InitAlgorithm -> 70 proofs that libverify.so accepts under the contributed vk; a
    flipped public-signal bit is rejected, and the delta = 1 vk rejects every proof made under the contributed key"""
    f = _child(tmp_path, algo, gsc.debug_srs_generate(L, bytes([algo + 40] * 32)), 70)
    assert f["srs_ok"] and f["step_ok"], f
    assert f["lens"] == [proof_len] * 70 and f["new"] == [True] * 70 and f["flipped"] is False and f["old"] == [False] * 70, f
