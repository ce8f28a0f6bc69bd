"""Test helper: trapdoor verifying keys and a discrete-logarithm model of the verifier's G1 stage (gsc_debug_verify_g1, include/libprove.h).

A trapdoor key is a verifying key whose every point is a known multiple of a generator: alpha = a G1, beta = b G2, gamma = g G2, delta = d G2,
K[i] = k_i G1 (None: the point at infinity) and, for the AES shape, ped_g = s G2, ped_gsn = -sigma s G2.  A proof is the logarithms (A, B, C, D,
PoK).  Every expected G1 result is then one integer expression mod r followed by one multiplication of the generator (devref.gen_mul); the only
sums taken on points are the window tables, built incrementally with keyraw.g1_add and spot-checked against their logarithms by
tests/test_verify_g1_model_host.py.  Because B and the G2 key points are known too, the batched equation of a chunk or a part holds iff one
integer combination is 0 mod r, so the model predicts every flag as well.  Nothing here calls the library."""
import functools
import random
import struct

import devref as D
import keyraw as KR

P, R = KR.P, KR.R
NWIN, NCWIN = 144, 32
FILL = 0xA5
G1_BYTES, G2_BYTES = 65, 129
NPUB = {0: 1152, 1: 141, 2: 141}
DST = b"bsb22-commitment"


# ---- points from logarithms ----
@functools.lru_cache(maxsize=None)
def g1(k):
    """(k mod r) G1 as (x, y) integers, None for the point at infinity"""
    if k is None:
        return None
    p = D.gen_mul(0, k % R)
    return None if p is None else (p[0][0], p[1][0])


@functools.lru_cache(maxsize=None)
def g2(k):
    if k is None:
        return None
    return D.gen_mul(1, k % R)


def lg(k):
    """the logarithm of a point given as a logarithm or None (infinity)"""
    return 0 if k is None else k % R


def out_g1(p):
    """a G1 point as the hook returns it"""
    return bytes(64) + b"\1" if p is None else KR.be(p[0]) + KR.be(p[1]) + b"\0"


def out_g2(p):
    return bytes(128) + b"\1" if p is None else KR.enc_g2(p, True) + b"\0"


# ---- public inputs (csrc/verify_common.cpp public_windows, restated; and its inverse) ----
def windows_of(algo, sig):
    ct, nonce, ctr, pt = sig[:64], sig[64:76], sig[76:80], sig[80:144]
    if algo == 0:
        words = [int.from_bytes(ctr, "little")] + [int.from_bytes(nonce[4 * i:4 * i + 4], "little") for i in range(3)]
        words += [int.from_bytes(pt[4 * i:4 * i + 4], "big") for i in range(16)] + [int.from_bytes(ct[4 * i:4 * i + 4], "big") for i in range(16)]
        return bytes((w >> (8 * b)) & 0xFF for w in words for b in range(4))
    return bytes(nonce) + int.from_bytes(ctr, "big").to_bytes(4, "little") + bytes(pt) + bytes(ct)


def sig_of(algo, win):
    """the 144 signal bytes whose windows are win"""
    win = bytes(win)
    assert len(win) == NWIN
    if algo == 0:
        rev = lambda b: b"".join(b[4 * i:4 * i + 4][::-1] for i in range(len(b) // 4))
        ctr, nonce, pt, ct = win[0:4], win[4:16], rev(win[16:80]), rev(win[80:144])
    else:
        nonce, ctr, pt, ct = win[0:12], win[12:16][::-1], win[16:80], win[80:144]
    sig = ct + nonce + ctr + pt
    assert windows_of(algo, sig) == win
    return sig


def window_base(algo, j):
    """(first K index, shift) of window j: csrc/verify_common.cpp window_base"""
    if algo == 0:
        return 1 + 8 * j, 0
    if j < 12:
        return 1 + j, 0
    if j < 16:
        return 13, 8 * (j - 12)
    return 1 + j - 3, 0


# ---- keys ----
class TrapdoorKey:
    """k: the logarithms of K (None = infinity); raw: the K indices written in the raw encoding (an infinity among them is 64 zero bytes);
    raw_names: which of "alpha", "beta", "gamma", "delta", "ped_g", "ped_gsn" are raw"""

    def __init__(self, algo, a, b, g, d, k, s=None, sigma=None, raw=(), raw_names=()):
        self.algo, self.a, self.b, self.g, self.d, self.k = algo, a % R, b % R, g % R, d % R, list(k)
        self.s, self.sigma, self.raw, self.raw_names = s, sigma, frozenset(raw), frozenset(raw_names)
        self.has_commitment = s is not None
        assert len(self.k) == 1 + NPUB[algo] + (1 if self.has_commitment else 0), "key_fits"
        assert algo != 0 or not self.has_commitment

    def klog(self, i):
        return lg(self.k[i])

    def vk_bytes(self):
        """the layout csrc/verify_common.cpp parse_vk_layout reads"""
        n = self.raw_names
        out = KR.enc_g1(g1(self.a), "alpha" in n) + KR.enc_g1(g1(self.b), False) + KR.enc_g2(g2(self.b), "beta" in n) + KR.enc_g2(g2(self.g), "gamma" in n)
        out += KR.enc_g1(g1(self.d), False) + KR.enc_g2(g2(self.d), "delta" in n) + struct.pack(">I", len(self.k))
        out += b"".join(KR.enc_g1(g1(k), i in self.raw) for i, k in enumerate(self.k))
        if not self.has_commitment:
            return out + struct.pack(">II", 0, 0)
        out += struct.pack(">III", 1, 0, 1)
        return out + KR.enc_g2(g2(self.s), "ped_g" in n) + KR.enc_g2(g2(-self.sigma * self.s), "ped_gsn" in n)

    def key_status(self):
        g1s = [0, 0, 0] + [1 if g1(k) is None else 0 for k in self.k]
        return bytes(g1s + [0] * (5 if self.has_commitment else 3))

    # window tables: logarithms ...
    def entry_log(self, w, v):
        first, shift = window_base(self.algo, w)
        if self.algo == 0:
            return sum(self.klog(first + t) for t in range(8) if (v >> t) & 1) % R
        return v * (1 << shift) * self.klog(first) % R

    def centry_log(self, j, v):
        return v * (1 << (8 * j)) * self.klog(1 + NPUB[self.algo]) % R

    # ... and points, incrementally
    def table_points(self):
        out = []
        for w in range(NWIN):
            first, shift = window_base(self.algo, w)
            out += _subset_window(tuple(self.klog(first + t) for t in range(8))) if self.algo == 0 else _multiple_window(self.klog(first), shift)
        return out

    def ctable_points(self):
        return [p for j in range(NCWIN) for p in _multiple_window(self.klog(1 + NPUB[self.algo]), 8 * j)]

    def l_trace(self, win):
        """lsum's walk in logarithms: [(accumulator before window w, entry of window w)]"""
        acc, out = self.klog(0), []
        for w in range(NWIN):
            e = self.entry_log(w, win[w])
            out.append((acc, e)); acc = (acc + e) % R
        return out

    def l_public(self, win):
        t = self.l_trace(win)
        return (t[-1][0] + t[-1][1]) % R


@functools.lru_cache(maxsize=None)
def _subset_window(logs):
    """the 256 subset sums of eight points: entry v = entry (v without its lowest bit) + that bit's point"""
    pts, out = [g1(k) for k in logs], [None]
    for v in range(1, 256):
        low = (v & -v).bit_length() - 1
        out.append(KR.g1_add(out[v & (v - 1)], pts[low]))
    return out


@functools.lru_cache(maxsize=None)
def _multiple_window(log, shift):
    """v 2^shift K for v < 256, by repeated addition of 2^shift K"""
    base, out = g1(log * (1 << shift)), [None]
    for v in range(1, 256):
        out.append(KR.g1_add(out[-1], base))
    return out


def challenge(d_log):
    """hash_to_field of the uncompressed commitment; D = infinity hashes 0x40 and 63 zero bytes"""
    d = g1(d_log)
    msg = bytes([0x40]) + bytes(63) if d is None else KR.be(d[0]) + KR.be(d[1])
    return int.from_bytes(D.expand_message_xmd48(msg, DST), "big") % R


# ---- proofs ----
class Proof:
    """One column.  A, C, D, PoK (G1) and B (G2): logarithms, None = infinity.  a_point: A is this curve point of unknown logarithm (B must be
    infinity, so that the pair contributes nothing).  slots: bytes that replace the encoding of "A" / "B" / "C" / "D" / "PoK"; length: the length
    handed over; count: the commitment count word.  bad: the column must not decode (ok = 0) and why."""

    def __init__(self, name, key, win, A=None, B=None, C=None, Dc=None, PoK=None, a_point=None, slots=None, length=None, count=None, bad=None, tags=()):
        self.name, self.key, self.win, self.A, self.B, self.C, self.D, self.PoK = name, key, bytes(win), A, B, C, Dc, PoK
        self.a_point, self.slots, self.length, self.count, self.bad, self.tags = a_point, slots or {}, length, count, bad, tuple(tags)
        assert a_point is None or (A is None and B is None)
        assert key.has_commitment or Dc is None
        self.sig = sig_of(key.algo, self.win)

    ok = property(lambda self: self.bad is None)

    def slot(self):
        com = self.key.has_commitment
        e = {"A": KR.enc_g1(self.a_point or g1(self.A), False), "B": KR.enc_g2(g2(self.B), False), "C": KR.enc_g1(g1(self.C), False),
             "D": KR.enc_g1(g1(self.D), False), "PoK": KR.enc_g1(g1(self.PoK), False)}
        e.update(self.slots)
        count = (1 if com else 0) if self.count is None else self.count
        b = e["A"] + e["B"] + e["C"] + struct.pack(">I", count) + (e["D"] if com else b"") + e["PoK"]
        return b.ljust(196, b"\0"), (len(b) if self.length is None else self.length)

    def l_log(self):
        k = self.key
        acc = k.l_public(self.win)
        if k.has_commitment:
            acc += challenge(self.D) * k.klog(1 + NPUB[k.algo]) + lg(self.D)
        return acc % R

    def residue(self):
        """the exponent of the proof's own Groth16 equation: 0 iff e(A, B) = e(alpha, beta) e(L, gamma) e(C, delta)"""
        k = self.key
        return (lg(self.A) * lg(self.B) - k.a * k.b - self.l_log() * k.g - lg(self.C) * k.d) % R

    def pok_residue(self):
        k = self.key
        return (lg(self.PoK) - k.sigma * lg(self.D)) * k.s % R if k.has_commitment else 0

    def verdict(self):
        return int(self.ok and self.residue() == 0 and self.pok_residue() == 0)


def valid_c(key, win, A, B, Dc=None):
    """C = (A B - a b - L g) / d: the proof (A, B, C, D, sigma D) then verifies"""
    probe = Proof("probe", key, win, A, B, 0, Dc)
    return (lg(A) * lg(B) - key.a * key.b - probe.l_log() * key.g) * pow(key.d, -1, R) % R


# ---- one call of the hook ----
def words(v):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(4)]


class Case:
    """proofs: the columns; rho, t: one 128-bit integer per column; ends: part ends or (); ra_only: None, or the columns whose rho A is compared
    (the large case)"""

    def __init__(self, name, key, proofs, rho, t, ends=(), ra_only=None, claims=()):
        self.name, self.key, self.proofs, self.rho, self.t, self.ends, self.ra_only, self.claims = name, key, list(proofs), list(rho), list(t), tuple(ends), ra_only, list(claims)
        assert len(self.rho) == len(self.t) == len(self.proofs)

    n = property(lambda self: len(self.proofs))

    def inputs(self):
        slots = [p.slot() for p in self.proofs]
        rnd = [w for r, t in zip(self.rho, self.t) for w in words(r) + words(t)]
        return b"".join(s for s, _ in slots), [l for _, l in slots], b"".join(p.sig for p in self.proofs), rnd

    # the sums of proofs [lo, hi) in logarithms: (sum rho over ok, sum rho L, sum rho C, sum t D, sum t PoK, sum rho A B)
    def sums(self, lo, hi):
        com = self.key.has_commitment
        s = [0] * 6
        for i in range(lo, hi):
            p = self.proofs[i]
            if not p.ok:
                continue
            r, t = self.rho[i], self.t[i]
            s[0] += r; s[1] += r * _l_log(p); s[2] += r * lg(p.C); s[5] += r * lg(p.A) * lg(p.B)
            if com:
                s[3] += t * lg(p.D); s[4] += t * lg(p.PoK)
        return s

    def fixed_logs(self, lo, hi):
        """-(sum rho) alpha, -sum rho L, -sum rho C, sum t PoK, sum t D, and whether the equation holds"""
        k, s = self.key, self.sums(lo, hi)
        fx = [-s[0] * k.a % R, -s[1] % R, -s[2] % R, s[4] % R, s[3] % R]
        total = s[5] + fx[0] * k.b + fx[1] * k.g + fx[2] * k.d
        if k.has_commitment:
            total += fx[3] * k.s - fx[4] * k.sigma * k.s
        return fx, int(total % R == 0), s[0]

    def expected(self, fill=FILL):
        k, n, com = self.key, self.n, self.key.has_commitment
        f1, f2 = bytes([fill]) * G1_BYTES, bytes([fill]) * G2_BYTES
        g1b, g2b = [], []
        for i, p in enumerate(self.proofs):
            if p.ok:
                g1b += [out_g1(p.a_point or g1(p.A)), out_g1(g1(p.C)), out_g1(g1(_l_log(p))), out_g1(g1(p.D)) if com else f1, out_g1(g1(p.PoK))]
                g2b.append(out_g2(g2(p.B)))
            else:
                g1b += [f1] * 5; g2b.append(f2)
            if self.ra_only is not None and i not in self.ra_only:
                g1b.append(None)
            elif not p.ok:
                g1b.append(out_g1(None))
            elif p.a_point:
                g1b.append(out_g1(KR.g1_mul(p.a_point, self.rho[i]) if self.rho[i] else None))
            else:
                g1b.append(out_g1(g1(self.rho[i] * lg(p.A)) if p.A is not None else None))
        fx, flag, _ = self.fixed_logs(0, n)
        want = {"key_status": k.key_status(), "ok": bytes(int(p.ok) for p in self.proofs), "g1": g1b, "g2": b"".join(g2b),
                "fixed": b"".join(out_g1(g1(v)) if com or j < 3 else out_g1(None) for j, v in enumerate(fx)), "flag": bytes([flag])}
        want["okv"] = want["ok"]
        pf, prho, pflag = [], [], []
        for j, end in enumerate(self.ends):
            fx, flag, rs = self.fixed_logs(self.ends[j - 1] if j else 0, end)
            pf += [out_g1(g1(v)) if com or q < 3 else f1 for q, v in enumerate(fx)]
            prho.append(tuple((rs >> (32 * c)) & 0xFFFFFFFF for c in range(5))); pflag.append(flag)
        want.update(pfixed=b"".join(pf), prho=prho, pflag=bytes(pflag))
        return want

    def expected_tables(self, fill=FILL):
        k = self.key
        ct = b"".join(out_g1(p) for p in k.ctable_points()) if k.has_commitment else bytes([fill]) * (NCWIN * 256 * G1_BYTES)
        return b"".join(out_g1(p) for p in k.table_points()), ct


def _l_log(p):
    """p.l_log(), remembered on the key: the large case repeats a few columns thousands of times"""
    cache = p.key.__dict__.setdefault("_l_cache", {})
    at = (p.win, p.D)
    if at not in cache:
        cache[at] = p.l_log()
    return cache[at]


def mismatches(case, got, want):
    """(field, index, column name) of every difference between the hook's answer and expected()"""
    bad = []
    for key in ("ok", "okv", "flag", "pflag"):
        bad += [(key, i, case.proofs[i].name if key in ("ok", "okv") else "") for i in range(len(want[key])) if got[key][i:i + 1] != want[key][i:i + 1]]
    assert len(got["ok"]) == case.n
    assert got["key_status"][:len(want["key_status"])] == want["key_status"], "key_status"
    names = ("A", "C", "L", "D", "PoK", "ra")
    for q, w in enumerate(want["g1"]):
        if w is not None and got["g1"][G1_BYTES * q:G1_BYTES * (q + 1)] != w:
            bad.append((names[q % 6], q // 6, case.proofs[q // 6].name))
    for i in range(case.n):
        if got["g2"][G2_BYTES * i:G2_BYTES * (i + 1)] != want["g2"][G2_BYTES * i:G2_BYTES * (i + 1)]:
            bad.append(("B", i, case.proofs[i].name))
    for key in ("fixed", "pfixed"):
        bad += [(key, q, "") for q in range(len(want[key]) // G1_BYTES) if got[key][G1_BYTES * q:G1_BYTES * (q + 1)] != want[key][G1_BYTES * q:G1_BYTES * (q + 1)]]
    bad += [("prho", j, "") for j, w in enumerate(want["prho"]) if tuple(got["prho"][j]) != w]
    return bad


def table_mismatches(got, want):
    return [(q // 256, q % 256) for q in range(len(want) // G1_BYTES) if got[G1_BYTES * q:G1_BYTES * (q + 1)] != want[G1_BYTES * q:G1_BYTES * (q + 1)]]


# ---------------------------------------------------------------- the case table ----------------------------------------------------------------
RHO_EDGES = (1, 1 << 127, (1 << 128) - 1)
PART_ENDS = (1, 3, 66, 130, 195, 324)      # parts of 1, 2, 63, 64, 65 and 129 proofs; every boundary but the first lies inside a block of 64
BLOCK = 64


def _rl(rnd):
    return rnd.randrange(1, R)


@functools.lru_cache(maxsize=None)
def keys():
    """name -> TrapdoorKey: ChaCha20 plain and with collisions, AES-128 plain, with collisions, and with L = infinity through the commitment"""
    rnd = random.Random(0x61)
    a, b, g, d = (_rl(rnd) for _ in range(4))
    base = [_rl(rnd) for _ in range(1153)]
    out = {"chacha_plain": TrapdoorKey(0, a, b, g, d, base, raw=range(0, 1153, 3), raw_names=("alpha", "gamma"))}
    k = list(base)
    k[1] = k[0]; k[9] = -(k[0] + k[1]) % R                    # lsum: acc == entry at window 0, acc == -entry at window 1
    k[42] = k[41]; k[50] = -k[49] % R                         # windows 5 and 6: two equal, two opposite points
    k[64] = -sum(k[57:64]) % R                                # window 7: the full subset is the point at infinity
    k[66] = None; k[67] = None                                # window 8: infinity, compressed and raw
    out["chacha_coll"] = TrapdoorKey(0, a, b, g, d, k, raw=(0, 9, 42, 67, 1152), raw_names=("beta", "delta"))
    ak = [_rl(rnd) for _ in range(143)]
    s, sigma = _rl(rnd), _rl(rnd)
    out["aes_plain"] = TrapdoorKey(1, a, b, g, d, ak, s=s, sigma=sigma, raw=range(1, 143, 5), raw_names=("delta", "ped_gsn"))
    k = list(ak)
    k[3] = None; k[142] = R - 1                               # window 2 holds nothing but infinity; the commitment base is -G
    out["aes_coll"] = TrapdoorKey(1, a, b, g, d, k, s=s, sigma=sigma, raw=(3, 13, 142), raw_names=("ped_g",))
    # k_0 chosen after D and the windows: k_0 + sum + c k_c + D = 0
    k = list(ak); k[0] = 0
    probe = TrapdoorKey(1, a, b, g, d, k, s=s, sigma=sigma)
    k[0] = -(probe.l_public(LINF_WIN) + challenge(LINF_D) * probe.klog(142) + LINF_D) % R
    out["aes_linf"] = TrapdoorKey(1, a, b, g, d, k, s=s, sigma=sigma, raw=(0,), raw_names=("alpha",))
    return out


LINF_WIN = bytes((37 * j + 11) % 256 for j in range(NWIN))
LINF_D = 0x1234567890abcdef1234567890abcdef


def _largest_x_point():
    x = P - 1
    while KR.sqrt_fp(KR.g1_rhs(x)) is None:
        x -= 1
    return x, KR.sqrt_fp(KR.g1_rhs(x))


def _off_curve_x():
    x = 4
    while KR.sqrt_fp(KR.g1_rhs(x)) is not None:
        x += 1
    return x


class Columns:
    """the named columns of one key"""

    def __init__(self, key, seed):
        self.key, self.rnd = key, random.Random(seed)
        self.com = key.has_commitment
        self.valid, self.other, self.bad = [], [], []
        self._build()

    def win(self):
        return bytes(self.rnd.randrange(256) for _ in range(NWIN))

    def dlog(self):
        return _rl(self.rnd) if self.com else None

    def make(self, name, A, B, win=None, Dc="random", C="valid", PoK="sigma", tags=()):
        """C "valid": the C that makes the proof verify;  B "solve": the B that does, for the given C"""
        key = self.key
        win = self.win() if win is None else win
        Dc = self.dlog() if Dc == "random" else (Dc if self.com else None)
        if B == "solve":
            l = Proof("probe", key, win, 0, 0, 0, Dc).l_log()
            B = (key.a * key.b + l * key.g + lg(C) * key.d) * pow(lg(A), -1, R) % R
        elif C == "valid":
            C = valid_c(key, win, A, B, Dc)
        if PoK == "sigma":
            PoK = key.sigma * Dc % R if self.com and Dc is not None else None
        return Proof(name, key, win, A, B, C, Dc, PoK, tags=tags)

    def _build(self):
        key, rnd, com = self.key, self.rnd, self.com
        v = self.valid
        for i in range(3):
            v.append(self.make("ordinary%d" % i, _rl(rnd), _rl(rnd)))
        o = v[0]
        v.append(Proof("both_signs", key, o.win, -o.A % R, -o.B % R, o.C, o.D, o.PoK, tags=("neg_y",)))
        v.append(self.make("A_inf", None, _rl(rnd), tags=("A_inf",)))
        v.append(self.make("B_inf", _rl(rnd), None))
        v.append(self.make("C_inf", _rl(rnd), "solve", C=None, tags=("C_inf",)))
        p = _largest_x_point()
        w = self.win(); dl = self.dlog()
        v.append(Proof("largest_x", key, w, None, None, valid_c(key, w, None, None, dl), dl, key.sigma * dl % R if com else None, a_point=p))
        if com:
            v.append(self.make("D_PoK_inf", _rl(rnd), _rl(rnd), Dc=None, tags=("D_inf", "PoK_inf")))
            x = self.make("x", _rl(rnd), _rl(rnd))
            self.other.append(Proof("PoK_inf_alone", key, x.win, x.A, x.B, x.C, x.D, None, tags=("PoK_inf",)))
            self.other.append(Proof("D_inf_alone", key, x.win, x.A, x.B, x.C, None, x.PoK, tags=("D_inf",)))
        else:
            x = v[1]
            self.other.append(Proof("PoK_finite_unused", key, x.win, x.A, x.B, x.C, None, _rl(rnd)))      # decoded, in no sum: still valid
        self.other.append(Proof("all_inf", key, self.win(), None, _rl(rnd), None, None, None, tags=("A_inf", "C_inf") + (("D_inf", "PoK_inf") if com else ())))
        x = v[2]
        self.other.append(Proof("wrong_C", key, x.win, x.A, x.B, (x.C + 1) % R, x.D, x.PoK))
        w = bytearray(x.win); w[143] ^= 1
        self.other.append(Proof("wrong_public_byte", key, bytes(w), x.A, x.B, x.C, x.D, x.PoK))
        # the degenerate walks of lsum the key was made for
        if key is keys()["chacha_coll"]:
            w = bytearray(self.win()); w[0] = 1; w[1] = 2
            v.append(self.make("lsum_acc_eq_entry", _rl(rnd), _rl(rnd), win=bytes(w), tags=(("lsum_eq", 0),)))
            w = bytearray(self.win()); w[0] = 1; w[1] = 1
            v.append(self.make("lsum_acc_neg_entry", _rl(rnd), _rl(rnd), win=bytes(w), tags=(("lsum_neg", 1),)))
            v.append(self.make("L_inf", _rl(rnd), _rl(rnd), win=bytes([1, 1]) + bytes(142), tags=("L_inf", ("lsum_neg", 1))))
            w = bytearray(self.win()); w[8] = 0b110; w[7] = 255; w[5] = 3; w[6] = 3
            v.append(self.make("entries_at_infinity", _rl(rnd), _rl(rnd), win=bytes(w), tags=(("entry_inf", 8), ("entry_inf", 7), ("entry_inf", 6))))
        if key is keys()["aes_coll"]:
            w = bytearray(self.win()); w[2] = 0x37; w[12:16] = b"\xff\xff\xff\xff"
            v.append(self.make("counter_ff_entry_inf", _rl(rnd), _rl(rnd), win=bytes(w), tags=(("entry_inf", 2),)))
        if key is keys()["aes_linf"]:
            v.append(self.make("L_inf_commit", _rl(rnd), _rl(rnd), win=LINF_WIN, Dc=LINF_D, tags=("L_inf",)))
        # columns that must not decode, each a copy of a valid one with one thing wrong
        x = v[1]
        flagged = lambda xv, f: bytes([xv.to_bytes(32, "big")[0] | f]) + xv.to_bytes(32, "big")[1:]
        bad = lambda name, why, **kw: self.bad.append(Proof(name, key, x.win, x.A, x.B, x.C, x.D, x.PoK, bad=why, **kw))
        bad("x_ge_p", "A: x = p", slots={"A": flagged(P, 0x80)})
        bad("off_curve", "C: x^3 + 3 is no square", slots={"C": flagged(_off_curve_x(), 0xC0)})
        bad("flag_00", "A: flag bits 00", slots={"A": KR.be(g1(x.A)[0])})
        bad("inf_stray_bit", "PoK: infinity flag with a stray bit", slots={"PoK": bytes([0x40]) + bytes(30) + b"\1"})
        bad("B_outside_g2", "B: on the twist, outside the subgroup", slots={"B": KR.enc_g2(KR.twist_point_outside_g2(), False)})
        bad("short", "a byte short: proof_shape_ok", length=(196 if com else 164) - 1)
        bad("count_word", "the commitment count of the other shape: proof_shape_ok", count=0 if com else 1)
        if com:
            bad("D_off_curve", "D: x^3 + 3 is no square", slots={"D": flagged(_off_curve_x(), 0x80)})

    def all(self):
        """every column, the undecodable ones each between two that decode"""
        out = []
        for i, p in enumerate(self.valid + self.other):
            out += [p] + self.bad[i:i + 1]
        assert len(out) == len(self.valid) + len(self.other) + len(self.bad)
        return out

    def negated_c(self, p):
        """a valid proof with p's windows and commitment and C = -p.C: the two rho C terms cancel under equal rho, the rho L terms are equal"""
        return self.make(p.name + "_negC", _rl(self.rnd), "solve", win=p.win, Dc=p.D, C=-lg(p.C) % R)

    def negated_d(self, p):
        """a valid proof with D = -p.D (and so PoK = -p.PoK): the t D and t PoK terms cancel under equal t"""
        return self.make(p.name + "_negD", _rl(self.rnd), _rl(self.rnd), win=p.win, Dc=-p.D % R)


@functools.lru_cache(maxsize=None)
def columns(key_name):
    return Columns(keys()[key_name], sorted(keys()).index(key_name) + 100)


def _randomizers(rnd, n, shift):
    out = []
    for i in range(n):
        q = (i + shift) % 5
        out.append(RHO_EDGES[q] if q < 3 else rnd.getrandbits(128) | 1)
    return out


def _block_collisions(cols, proofs, rho, t, base, half, claims, where):
    """equal and opposite terms `half` positions apart from `base` on: P + P and P + (-P) in the first level of a tree of width 2 half"""
    v = cols.valid
    proofs[base + 5] = proofs[base + 5 + half] = v[0]
    proofs[base + 6], proofs[base + 6 + half] = v[1], cols.negated_c(v[1])
    for q in (5, 6, 7):
        rho[base + q + half] = rho[base + q]; t[base + q + half] = t[base + q]
    claims += [(where, 0, base + 5, base + 5 + half, "dbl"), (where, 1, base + 5, base + 5 + half, "dbl"), (where, 1, base + 6, base + 6 + half, "inf"), (where, 0, base + 6, base + 6 + half, "dbl")]
    if cols.com:
        proofs[base + 7], proofs[base + 7 + half] = v[2], cols.negated_d(v[2])
        claims += [(where, 2, base + 5, base + 5 + half, "dbl"), (where, 3, base + 5, base + 5 + half, "dbl"), (where, 2, base + 7, base + 7 + half, "inf"), (where, 3, base + 7, base + 7 + half, "inf")]


def _cancelling_pair(cols, rho_value):
    """two proofs that fail alone, C off by +e and -e: under equal rho the errors cancel and the batched equation holds"""
    x, y = cols.valid[0], cols.valid[1]
    e = 0xC0FFEE
    mk = lambda p, c, name: Proof(name, p.key, p.win, p.A, p.B, c % R, p.D, p.PoK)
    return [mk(x, x.C + e, "cancel_plus"), mk(y, y.C - e, "cancel_minus")], [rho_value, rho_value]


@functools.lru_cache(maxsize=None)
def case(key_name, shape):
    """shape: an int n (one chunk of the key's columns in rotation, with the tree collisions of block 0 when n >= 64), "valid66" (valid proofs
    and a cancelling pair: flag 1), "parts" (PART_ENDS) or "large" (4097 proofs, 65 blocks)"""
    cols, key = columns(key_name), keys()[key_name]
    rnd = random.Random("%s/%s" % (key_name, shape))
    claims = []
    if shape == "large":
        return _large_case(key_name, cols, rnd)
    if shape == "parts":
        return _parts_case(key_name, cols, rnd)
    if shape == "valid66":
        n = 66
        proofs = [cols.valid[i % len(cols.valid)] for i in range(n)]
        rho, t = _randomizers(rnd, n, 0), _randomizers(rnd, n, 2)
        pair, pr = _cancelling_pair(cols, (1 << 128) - 1)
        proofs[20], proofs[65] = pair; rho[20], rho[65] = pr
        claims += [("cancel", 0, n), ("rho_carry_chunk",)]
        _block_collisions(cols, proofs, rho, t, 0, 32, claims, "block_tree")
        return Case("%s/valid66" % key_name, key, proofs, rho, t, claims=claims)
    n = int(shape)
    every = cols.all()
    proofs = [every[i % len(every)] for i in range(n)] if n > 1 else [cols.valid[0]]
    rho, t = _randomizers(rnd, n, 1), _randomizers(rnd, n, 3)
    if n >= 64:
        _block_collisions(cols, proofs, rho, t, 0, 32, claims, "block_tree")
    if n > 2:
        claims.append(("not_ok_mid_block", 1))
    return Case("%s/%d" % (key_name, n), key, proofs, rho, t, claims=claims)


def _parts_case(key_name, cols, rnd):
    key, ends, claims = cols.key, PART_ENDS, []
    n = ends[-1]
    v, every = cols.valid, cols.all()
    proofs = [v[i % len(v)] for i in range(n)]
    rho, t = _randomizers(rnd, n, 0), _randomizers(rnd, n, 1)
    deg = [p for p in v if "L_inf" in p.tags] or [p for p in v if "A_inf" in p.tags]
    proofs[0] = deg[0]                                             # part 0: a degenerate valid proof alone
    pair, pr = _cancelling_pair(cols, (1 << 128) - 1)              # part 1: invalid one by one, valid together; sum rho carries into word 4
    proofs[1:3] = pair; rho[1:3] = pr
    claims += [("cancel", 1, 3), ("rho_carry_part", 1), ("part_tree", 1, 1, 2, "plain")]
    proofs[3] = cols.bad[0]                                        # part 2 (63): its first proof has no ok, lane 63 holds nothing
    rho[3] = (1 << 128) - 1
    claims += [("not_ok_part_first", 2), ("width", 2, 64), ("empty_lane", 2, 63)]
    _block_collisions(cols, proofs, rho, t, 66, 32, claims, "part_tree")      # part 3 (64): lanes l and l + 32
    claims.append(("width", 3, 64))
    for i in range(130, 195):                                      # part 4 (65): every column, the undecodable ones between valid neighbours
        proofs[i] = every[(i - 130) % len(every)]
    claims += [("two_in_lane", 4, 0), ("not_ok_mid_block", 131)]
    claims += [("two_in_lane", 5, 0), ("width", 5, 64), ("width", 0, 1), ("width", 1, 2), ("rho_carry_part", 5)]      # part 5 (129): valid
    return Case("%s/parts" % key_name, key, proofs, rho, t, ends=ends, claims=claims)


def _large_case(key_name, cols, rnd):
    """4097 proofs = 65 blocks: lane 0 of k_verify_batch_sum takes blocks 0 and 64.  Block 33 repeats block 1 (P + P between lanes 1 and 33),
    block 34 holds block 2's proofs with C negated (P + (-P)); a few columns do not decode; everything else is valid, so the flag is 1."""
    key, n, claims = cols.key, 4097, []
    v = cols.valid
    partner = [cols.negated_c(p) for p in v]
    proofs = [v[i % len(v)] for i in range(n)]
    rho, t = _randomizers(rnd, n, 0), _randomizers(rnd, n, 1)
    for q in range(BLOCK):
        proofs[33 * BLOCK + q] = proofs[BLOCK + q]; rho[33 * BLOCK + q] = rho[BLOCK + q]
        proofs[34 * BLOCK + q] = partner[(2 * BLOCK + q) % len(v)]; rho[34 * BLOCK + q] = rho[2 * BLOCK + q]
    special = [10, 2047, 2048, 4000, 4096]
    for j, i in enumerate(special[:4]):
        proofs[i] = cols.bad[j % len(cols.bad)]
    claims += [("lane_tree", 0, 1, 33, "dbl"), ("lane_tree", 1, 1, 33, "dbl"), ("lane_tree", 0, 2, 34, "dbl"), ("lane_tree", 1, 2, 34, "inf"), ("two_partials",),
               ("rho_carry_chunk",), ("not_ok_mid_block", 10)]
    ra_only = frozenset([i for i in range(n) if i % BLOCK in (0, BLOCK - 1)] + special)
    return Case("%s/large" % key_name, key, proofs, rho, t, ra_only=ra_only, claims=claims)


CASES = [(k, s) for k in ("chacha_plain", "chacha_coll", "aes_plain", "aes_coll", "aes_linf") for s in (1, 63, 64, 65, 130, "valid66", "parts")] + [("chacha_plain", "large")]
WHY = ("lsum_eq", "lsum_neg", "entry_inf", "L_inf", "table_dbl", "table_neg", "table_full_inf", "K_inf", "A_inf", "C_inf", "D_inf", "PoK_inf", "block_tree_dbl", "block_tree_inf",
       "part_tree_dbl", "part_tree_inf", "lane_tree_dbl", "lane_tree_inf", "two_partials", "width_1", "width_2", "width_64", "empty_lane", "two_in_lane",
       "rho_carry_chunk", "rho_carry_part", "rho_edges", "not_ok_mid_block", "not_ok_part_first", "cancel")


def claim_width(count):
    w = 1
    while w < 64 and w < count:
        w <<= 1
    return w


def reached(c):
    """the items of WHY that case c reaches, each CONFIRMED on the model's own logarithms (an assertion fails where a claim does not hold)"""
    key, got = c.key, set()
    term = lambda j, i: (c.rho[i] * (_l_log(c.proofs[i]) if j == 0 else lg(c.proofs[i].C)) if j < 2 else c.t[i] * lg(c.proofs[i].D if j == 2 else c.proofs[i].PoK)) % R
    part = lambda q: (c.ends[q - 1] if q else 0, c.ends[q])
    for i, p in enumerate(c.proofs):
        if not p.ok:
            continue
        trace = key.l_trace(p.win)
        for tag in p.tags:
            if isinstance(tag, tuple) and tag[0] == "lsum_eq":
                acc, e = trace[tag[1]]; assert acc == e != 0, (p.name, tag); got.add("lsum_eq")
            elif isinstance(tag, tuple) and tag[0] == "lsum_neg":
                acc, e = trace[tag[1]]; assert (acc + e) % R == 0 != e, (p.name, tag); got.add("lsum_neg")
            elif isinstance(tag, tuple) and tag[0] == "entry_inf":
                assert trace[tag[1]][1] == 0 and p.win[tag[1]] != 0, (p.name, tag); got.add("entry_inf")
            elif tag == "L_inf":
                assert _l_log(p) == 0, p.name; got.add("L_inf")
            elif tag in ("A_inf", "C_inf", "D_inf", "PoK_inf"):
                assert getattr(p, tag[:-4]) is None and (key.has_commitment or tag in ("A_inf", "C_inf")), (p.name, tag); got.add(tag)
    if c.rho and {1, 1 << 127, (1 << 128) - 1} <= set(c.rho) and (not key.has_commitment or {1, 1 << 127, (1 << 128) - 1} <= set(c.t)):
        got.add("rho_edges")
    for cl in c.claims:
        kind = cl[0]
        if kind in ("block_tree", "part_tree") and cl[-1] in ("dbl", "inf"):
            _, j, i1, i2, how = cl
            assert c.proofs[i1].ok and c.proofs[i2].ok and term(j, i1) != 0
            assert (term(j, i1) - term(j, i2)) % R == 0 if how == "dbl" else (term(j, i1) + term(j, i2)) % R == 0, cl
            if kind == "block_tree":
                assert i1 // BLOCK == i2 // BLOCK and i2 == i1 + 32
            else:
                q = [q for q in range(len(c.ends)) if part(q)[0] <= i1 < part(q)[1]][0]
                lo, hi = part(q)
                assert hi - lo <= 64 and i2 < hi and i2 - i1 == claim_width(hi - lo) // 2, cl
            got.add("%s_%s" % (kind, how))
        elif kind == "part_tree":
            pass
        elif kind == "lane_tree":
            _, j, b1, b2, how = cl
            nblk = (c.n + BLOCK - 1) // BLOCK
            tot = lambda b: sum(term(j, i) for i in range(BLOCK * b, min(c.n, BLOCK * (b + 1))) if c.proofs[i].ok) % R
            assert b2 == b1 + 32 < 64 and nblk > b2 and b1 + 64 >= nblk and tot(b1) != 0
            assert (tot(b1) - tot(b2)) % R == 0 if how == "dbl" else (tot(b1) + tot(b2)) % R == 0, cl
            got.add("lane_tree_" + how)
        elif kind == "two_partials":
            assert (c.n + BLOCK - 1) // BLOCK > 64; got.add(kind)
        elif kind == "width":
            lo, hi = part(cl[1]); assert claim_width(hi - lo) == cl[2]; got.add("width_%d" % cl[2])
        elif kind == "empty_lane":
            lo, hi = part(cl[1]); assert hi - lo <= cl[2] < claim_width(hi - lo); got.add(kind)
        elif kind == "two_in_lane":
            lo, hi = part(cl[1]); assert hi - lo > 64 + cl[2]; got.add(kind)
        elif kind == "rho_carry_chunk":
            assert c.sums(0, c.n)[0] >> 128; got.add(kind)
        elif kind == "rho_carry_part":
            assert c.sums(*part(cl[1]))[0] >> 128; got.add(kind)
        elif kind == "not_ok_mid_block":
            i = cl[1]; assert not c.proofs[i].ok and c.proofs[i - 1].ok and c.proofs[i + 1].ok and 0 < i % BLOCK < BLOCK - 1 and c.rho[i] != 0; got.add(kind)
        elif kind == "not_ok_part_first":
            lo, hi = part(cl[1]); assert not c.proofs[lo].ok and c.proofs[lo + 1].ok and c.rho[lo] != 0; got.add(kind)
        elif kind == "cancel":
            lo, hi = cl[1], cl[2]
            assert sum(1 for p in c.proofs[lo:hi] if p.ok and p.residue() != 0) >= 2 and c.fixed_logs(lo, hi)[1] == 1; got.add(kind)
        else:
            raise AssertionError(cl)
    # the keys' own collisions, in the table builders
    if key.algo == 0:
        for w in range(NWIN):
            ks = [key.klog(1 + 8 * w + t) for t in range(8)]
            if any(ks[i] == ks[j] != 0 for i in range(8) for j in range(i)):
                got.add("table_dbl")
            if any((ks[i] + ks[j]) % R == 0 != ks[i] for i in range(8) for j in range(i)):
                got.add("table_neg")
            if sum(ks) % R == 0 and all(ks):
                got.add("table_full_inf")
    if any(k is None for k in key.k):
        got.add("K_inf")
    return got
