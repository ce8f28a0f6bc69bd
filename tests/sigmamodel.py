"""Test helper: SYNTHETIC key pairs with one commitment key, and a sigma contribution to them with Python integers.

A synthetic pair is the smallest pk / vk that both key walkers (csrc/phase2.hpp walk_pk / walk_vk; tests/keyraw.py pk_sections / vk_sections)
accept: domain 4, three Z points, four wires, two K points, one commitment key of n bases.  Every point is a known multiple of the
generators: Basis_j = b_j G1, BasisExpSigma_j = sigma b_j G1, G = g G2, GSigmaNeg = -sigma g G2 (b_j = 0: the point at infinity), so the
Pedersen relation e(BasisExpSigma_j, G) e(Basis_j, GSigmaNeg) = 1 reads sigma b_j g - b_j sigma g = 0 on the discrete logarithms.  They are
no keys of any circuit: nothing can be proved with them.  contribution() is what gsc_setup_contribute_sigma must write for given x and k
(or a seed), every byte.  Nothing here calls the library."""
import hashlib

import keyraw
from keyraw import R

G1_GEN = (1, 2)
SIGMA = 0x2A5C1F0E9D8B7A69584736251403F2E1D0CFBEAD9C8B7A6958473625140312F1 % R
G = 0x1B3D5F7091B2D4F60718293A4B5C6D7E8F90A1B2C3D4E5F60718293A4B5C6D7F % R
DELTA = 0x5EED
POOL = [0x1D3 + 7 * i for i in range(24)]                         # the distinct discrete logarithms of the bases
_g1, _g2 = {}, {}


def g1(k):
    """k G1 (None: infinity), remembered: the sets share their points"""
    k %= R
    if k not in _g1:
        _g1[k] = keyraw.g1_mul(G1_GEN, k) if k else None
    return _g1[k]


def g2(k):
    k %= R
    if k not in _g2:
        _g2[k] = keyraw.g2_mul(keyraw.G2_GEN, k) if k else None
    return _g2[k]


def layout(n):
    """the discrete logarithms b_j of n bases: infinity (0) first, in the middle and last, two equal bases side by side; element 0 is
    infinite, so j0 = 1.  n = 1: one finite base."""
    if n == 1:
        return [POOL[0]]
    b = [POOL[i % len(POOL)] for i in range(n)]
    b[0] = b[n // 2] = b[n - 1] = 0
    if n > 4:
        b[3] = b[2]
    if not any(b):
        b[1] = POOL[1]
    return b


def _u32(v):
    return int(v).to_bytes(4, "big")


def _slice1(points):
    return _u32(len(points)) + b"".join(keyraw.enc_g1(p, False) for p in points)


class Pair:
    """pk, vk: the files; b: the bases' discrete logarithms; sigma, g: the commitment key's scalars"""

    def __init__(self, b, sigma=SIGMA, g=G, delta=DELTA):
        self.b, self.sigma, self.g, self.delta = list(b), sigma % R, g % R, delta % R
        nw = 4
        header = (4).to_bytes(8, "big") + b"".join(keyraw.be(v) for v in (1, 2, 3, 4, 5)) + b"\x00"
        pk = header + b"".join(keyraw.enc_g1(g1(k), False) for k in (11, 12, self.delta))
        pk += _slice1([g1(21 + i) for i in range(nw)]) + _slice1([g1(31 + i) for i in range(nw)])                      # A, B
        pk += _slice1([g1(41 + i) for i in range(3)]) + _slice1([g1(51), g1(52)])                                      # Z (domain - 1), K
        pk += keyraw.enc_g2(g2(12), False) + keyraw.enc_g2(g2(self.delta), False)
        pk += _u32(nw) + b"".join(keyraw.enc_g2(g2(31 + i), False) for i in range(nw))                                 # G2.B
        pk += nw.to_bytes(8, "big") + (2).to_bytes(8, "big") + (0).to_bytes(8, "big") + bytes(2 * nw)                 # wires, no infinite A / B
        pk += _u32(1) + _slice1([g1(k) for k in self.b]) + _slice1([g1(self.sigma * k) for k in self.b])
        self.pk = pk
        vk = keyraw.enc_g1(g1(11), False) + keyraw.enc_g1(g1(12), False) + keyraw.enc_g2(g2(12), False) + keyraw.enc_g2(g2(13), False)
        vk += keyraw.enc_g1(g1(self.delta), False) + keyraw.enc_g2(g2(self.delta), False)
        vk += _slice1([g1(61), g1(62), g1(63)])                                                                        # gamma's K
        vk += _u32(1) + _u32(0) + _u32(1) + keyraw.enc_g2(g2(self.g), False) + keyraw.enc_g2(g2(-self.sigma * self.g), False)
        self.vk = vk

    @property
    def j0(self):
        return next(j for j, k in enumerate(self.b) if k)

    def relation_on_logarithms(self):
        """sigma b_j g + b_j (-sigma g) = 0 mod r for every j: the Pedersen relation of this pair in the exponent"""
        return all((self.sigma * k * self.g + k * (-self.sigma * self.g)) % R == 0 for k in self.b)


def build(n, **kw):
    return Pair(layout(n), **kw)


def seeded(seed):
    """(x, k) of a seeded contribution"""
    return tuple(int.from_bytes(hashlib.sha256(label + seed).digest(), "big") % R for label in (b"gsc-sigma-x", b"gsc-sigma-k"))


def challenge(h_prev, base, new, T):
    return int.from_bytes(hashlib.sha256(b"gsc-sigma-v1" + h_prev + base + new + T).digest()[:31], "big")


def scaled(pair, x):
    """(pk', vk') of the contribution x: BasisExpSigma' = x BasisExpSigma, GSigmaNeg' = x GSigmaNeg, compressed; every other byte as it was"""
    pk2 = keyraw.rewrite_pk(pair.pk, replace={("ped.sigma", j): keyraw.enc_g1(g1(x * pair.sigma * k), False) for j, k in enumerate(pair.b)})
    vk2 = keyraw.rewrite_vk(pair.vk, replace={("ped.gsn", 0): keyraw.enc_g2(g2(-x * pair.sigma * pair.g), False)})
    return pk2, vk2


def contribution(pair, x, k):
    """(pk', vk', record) as gsc_setup_contribute_sigma must write them for the secret x and the nonce k"""
    pk2, vk2 = scaled(pair, x)
    j0 = pair.j0
    base, new, T = (keyraw.enc_g1(g1(m * pair.sigma * pair.b[j0]), True) for m in (1, x, k))
    h_prev = hashlib.sha256(pair.pk).digest()
    z = (k + challenge(h_prev, base, new, T) * x) % R
    return pk2, vk2, h_prev + hashlib.sha256(pk2).digest() + new + T + z.to_bytes(32, "big")
