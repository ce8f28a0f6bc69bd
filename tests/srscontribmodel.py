"""A second implementation of a contribution to a powers file (csrc/srs_contrib.hpp) for the tests: the seeded scalars, the
challenge, the 544-byte record and the contributed file, with Python integers, hashlib and tests/keyraw.py's affine group law — independent of
the library, slow, meant for small L."""
import hashlib

import keyraw
import srsmodel
from keyraw import R

NAMES = (b"tau", b"alpha", b"beta")
RECORD_BYTES = 544
SECTIONS = ("tauG1", "tauG2", "alphaG1", "betaG1", "betaG2")


def _mod_r(label, seed):
    return int.from_bytes(hashlib.sha256(label + seed).digest(), "big") % R


def scalars(seed):
    """((tau', alpha', beta'), (k_tau, k_alpha, k_beta)) of a seeded contribution"""
    return tuple(_mod_r(b"gsc-phase1-" + n, seed) for n in NAMES), tuple(_mod_r(b"gsc-phase1-k-" + n, seed) for n in NAMES)


def challenge(s, h_prev, base, new, T):
    """c_s for s = 0 / 1 / 2 (tau / alpha / beta); base, new, T: 64 raw bytes each"""
    return int.from_bytes(hashlib.sha256(b"gsc-phase1-v1" + bytes([s]) + h_prev + base + new + T).digest()[:31], "big")


def count(L, section):
    N = 1 << L
    return {"tauG1": 2 * N - 1, "tauG2": N, "alphaG1": N, "betaG1": N, "betaG2": 1}[section]


def element(srs, L, section, i=0):
    o = srsmodel.offset(L, section, i)
    return srs[o:o + (128 if section.endswith("G2") else 64)]


def point(srs, L, section, i=0):
    st, p = (keyraw.decode_g2 if section.endswith("G2") else keyraw.decode_g1)(element(srs, L, section, i))
    assert st == 0, (section, i)
    return p


def factor(section, i, secrets):
    """the scalar a contribution multiplies element i of a section by"""
    tau, alpha, beta = secrets
    t = pow(tau, i, R)
    return {"tauG1": t, "tauG2": t, "alphaG1": alpha * t % R, "betaG1": beta * t % R, "betaG2": beta}[section]


def contributed_element(srs, L, section, i, secrets):
    mul, enc = (keyraw.g2_mul, keyraw.enc_g2) if section.endswith("G2") else (keyraw.g1_mul, keyraw.enc_g1)
    return enc(mul(point(srs, L, section, i), factor(section, i, secrets)), True)


def contribute(srs, L, secrets):
    """the contributed file, every element recomputed (4N - 1 multiplications in G1, N + 1 in G2)"""
    out = srs[:12]
    for sec in SECTIONS:
        out += b"".join(contributed_element(srs, L, sec, i, secrets) for i in range(count(L, sec)))
    assert len(out) == len(srs)
    return out


BASES = (("tauG1", 1), ("alphaG1", 0), ("betaG1", 0))      # base_s in prev, new_s in next


def record(prev, nxt, L, secrets, nonces):
    h_prev = hashlib.sha256(prev).digest()
    out = h_prev + hashlib.sha256(nxt).digest()
    for s, (sec, i) in enumerate(BASES):
        base, new = element(prev, L, sec, i), element(nxt, L, sec, i)
        T = keyraw.enc_g1(keyraw.g1_mul(point(prev, L, sec, i), nonces[s]), True)
        z = (nonces[s] + challenge(s, h_prev, base, new, T) * secrets[s]) % R
        out += new + T + z.to_bytes(32, "big")
    assert len(out) == RECORD_BYTES
    return out


def proof_offset(s):
    """where proof s (new | T | z) starts in a record"""
    return 64 + 160 * s
