"""A second writer of the powers file (csrc/srs.hpp) for the tests: the format from known (tau, alpha, beta) with
tests/keyraw.py's affine group law — independent of the library, slow, meant for L = 2."""
import keyraw

MAGIC = b"gscsrs01"
G1 = (1, 2)
G2 = keyraw.G2_GEN


def layout(L):
    """byte offsets of the sections and the length of a file with N = 2^L"""
    N = 1 << L
    o = {"tauG1": 12}
    o["tauG2"] = o["tauG1"] + 64 * (2 * N - 1)
    o["alphaG1"] = o["tauG2"] + 128 * N
    o["betaG1"] = o["alphaG1"] + 64 * N
    o["betaG2"] = o["betaG1"] + 64 * N
    o["bytes"] = o["betaG2"] + 128
    return o


def offset(L, section, i=0):
    return layout(L)[section] + (128 if section.endswith("G2") else 64) * i


def points(L, tau, alpha, beta, tau_g2=None):
    """the sections as lists of affine points; tau_g2: another tau for the G2 powers (a file that must be refused)"""
    N = 1 << L
    t2 = tau if tau_g2 is None else tau_g2
    R = keyraw.R
    return {"tauG1": [keyraw.g1_mul(G1, pow(tau, i, R)) for i in range(2 * N - 1)],
            "tauG2": [keyraw.g2_mul(G2, pow(t2, i, R)) for i in range(N)],
            "alphaG1": [keyraw.g1_mul(G1, alpha * pow(tau, i, R) % R) for i in range(N)],
            "betaG1": [keyraw.g1_mul(G1, beta * pow(tau, i, R) % R) for i in range(N)],
            "betaG2": [keyraw.g2_mul(G2, beta)]}


def encode(L, pts):
    out = MAGIC + L.to_bytes(4, "big")
    for sec in ("tauG1", "tauG2", "alphaG1", "betaG1", "betaG2"):
        enc = keyraw.enc_g2 if sec.endswith("G2") else keyraw.enc_g1
        out += b"".join(enc(p, True) for p in pts[sec])
    assert len(out) == layout(L)["bytes"]
    return out


def write(L, tau, alpha, beta, tau_g2=None):
    return encode(L, points(L, tau, alpha, beta, tau_g2))


def replace(srs, L, section, i, element):
    """the file with one element replaced by the given bytes"""
    o = offset(L, section, i)
    assert len(element) == (128 if section.endswith("G2") else 64)
    return srs[:o] + element + srs[o + len(element):]
